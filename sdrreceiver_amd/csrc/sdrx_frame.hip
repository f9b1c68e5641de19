// sdrx_frame.hip -- the per-frame launch sequence: how a raw frame reaches the device (staging, DC-bias ingest), which kernels
// run on it in which order on which stream (enqueue_frame, the software pipeline), and the ABI calls that start a frame.
// How its payloads come back is sdrx_delivery.hip.  A fragment of sdrx.hip's translation unit.

namespace {

hipEvent_t get_event(sdrx_ctx *c)
{
    if (!c->tm.pool.empty()) {
        hipEvent_t e = c->tm.pool.back();
        c->tm.pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess)
        return nullptr; // the launch is then simply not timed
    return e;
}

void drain_events(sdrx_ctx *c)
{
    for (auto &te : c->tm.pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, te.a, te.b) == hipSuccess) {
            c->tm.ms[te.kind] += ms;
            c->tm.n[te.kind] += 1;
            c->tm.bytes[te.kind] += te.bytes;
        }
        c->tm.pool.push_back(te.a);
        c->tm.pool.push_back(te.b);
    }
    c->tm.pending.clear();
}

struct Bracket { // RAII: event pair around one launch when timing is on, on the launch's stream
    sdrx_ctx *c;
    hipStream_t st;
    TimedEvent te{};
    bool on;
    Bracket(sdrx_ctx *ctx, hipStream_t stream, int kind, int64_t bytes) : c(ctx), st(stream), on(ctx->tm.on)
    {
        if (!on)
            return;
        te.kind = kind;
        te.bytes = bytes;
        te.a = get_event(c);
        te.b = get_event(c);
        if (!te.a || !te.b) {
            on = false;
            return;
        }
        (void)hipEventRecord(te.a, st);
    }
    ~Bracket()
    {
        if (!on)
            return;
        (void)hipEventRecord(te.b, st);
        c->tm.pending.push_back(te);
    }
};

// The kernel variants this context runs, as compile-time constants: fn(EXACT, ROT, METER, PARK), each a std::bool_constant, from
// option "exact" -- 1 the exact arithmetic, 0 the tolerance arithmetic (NCO as rotations), 2 the robust one (exact NCO, FMA mixer
// and filters; mix.hip, nco_mix) --, option "meter" and option "park".  Every launch of a kernel that has variants goes through
// here, so these twelve combinations are all that is ever instantiated: there is no (EXACT, ROT) = (1, 1) kernel.
template <class F>
void with_variant(const sdrx_ctx *c, F fn)
{
    auto arith = [&](auto meter, auto park) {
        if (c->opt_exact == 1)
            fn(std::true_type(), std::false_type(), meter, park);
        else if (c->opt_exact == 2)
            fn(std::false_type(), std::false_type(), meter, park);
        else
            fn(std::false_type(), std::true_type(), meter, park);
    };
    auto meter = [&](auto park) {
        if (c->opt_meter)
            arith(std::true_type(), park);
        else
            arith(std::false_type(), park);
    };
    if (c->opt_park)
        meter(std::true_type());
    else
        meter(std::false_type());
}
// Option park: the flag words of one kernel's descriptors (sdrx_ctx::Park: `first` = where that kernel's words begin in d_act);
// empty with the option off.
template <bool PARK>
ParkArg<PARK> park_arg(const sdrx_ctx *c, size_t first)
{
    ParkArg<PARK> P;
    if constexpr (PARK)
        P.act = c->park.d_act + first;
    return P;
}

// Where the ingest kernels leave a frame in tile layout: the first buffer of the route sdrx_finalize planned (plan_ingest_route).
float4 *ingest_dest(sdrx_ctx *c) { return reinterpret_cast<float4 *>(c->route.ingest_out); }

// Resampler: the staged input-rate frame of the next frame (c->frame_no) -> the tree's raw frame, on the context's stream
// behind the ingest kernel that staged it, inside that kernel's KIND_INGEST bracket.  The history slot of the previous frame's
// parity is read, this frame's written (resample.hip).  Off: nothing.
void resample_launch(sdrx_ctx *c)
{
    if (!c->rs.on)
        return;
    const ResamplePlan &P = c->rs.plan;
    const int p = (int)(c->frame_no & 1ull);
    ResampleArgs A;
    A.stage = c->rs.d_stage;
    A.hist_prev = c->rs.d_hist + (size_t)(p ^ 1) * kRsHist;
    A.hist_next = c->rs.d_hist + (size_t)p * kRsHist;
    A.taps = reinterpret_cast<const float4 *>(c->rs.d_taps.get());
    A.out = reinterpret_cast<float4 *>(c->d_raw_tiled.get());
    A.n_in = P.n_in, A.n_out = P.n_out;
    A.L = P.L, A.M = P.M, A.T = P.T;
    hipLaunchKernelGGL(k_resample, dim3((P.n_out + kRsChunk - 1) / kRsChunk), dim3(256), c->rs.lds_bytes, c->st.stream, A);
}

// Front stage: one k_front_halfband launch per stage for the next frame (c->frame_no), on the context's stream behind the ingest
// kernel that staged its input, inside that kernel's KIND_INGEST bracket and in front of resample_launch.  `real_words`: the
// frame's 16-bit words on the device where stage 1 is the real one (format `fmt`), else null.  Every stage reads the history
// slot of the previous frame's parity and writes this frame's (front.hip).  Off: nothing.
void front_launch(sdrx_ctx *c, const void *real_words = nullptr, int fmt = -1)
{
    if (!c->fr.on)
        return;
    const FrontPlan &P = c->fr.plan;
    const int p = (int)(c->frame_no & 1ull);
    for (int s = 1; s <= P.stages; ++s) {
        FrontArgs A;
        const bool real = s == 1 && P.real;
        A.in = real ? real_words : static_cast<const void *>(c->fr.d_in[s - 1].get());
        float2 *hist = c->fr.d_hist + (size_t)(s - 1) * 2 * kFrHist;
        A.hist_prev = hist + (size_t)(p ^ 1) * kFrHist;
        A.hist_next = hist + (size_t)p * kFrHist;
        A.taps = c->fr.d_taps;
        A.out = reinterpret_cast<float4 *>(s < P.stages ? c->fr.d_in[s].get() : c->route.front_out);
        A.n_out = (int)front_stage_out(P, s), A.n_in = 2 * A.n_out;
        A.K = P.K;
        auto k = !real ? k_front_halfband<kFrontComplex> : fmt == SDRX_FMT_RS16 ? k_front_halfband<kFrontRS16> : k_front_halfband<kFrontRU12>;
        hipLaunchKernelGGL(k, dim3((A.n_out + kFrTile - 1) / kFrTile), dim3(256), 0, c->st.stream, A);
    }
}

// Impulse blanker: k_blank and k_blank_step for the next frame (c->frame_no), on the context's stream behind the ingest kernel that
// staged it, inside that kernel's KIND_INGEST bracket and in front of front_launch.  Out of place: from the blanker's staging
// frame to the route's blank_out.  The state chains on the device in stream order.  Off: nothing.
void blank_launch(sdrx_ctx *c)
{
    if (!c->bl.on)
        return;
    const int p = (int)(c->frame_no & 1ull);
    const BlankCfg &B = c->bl.cfg;
    hipLaunchKernelGGL(k_blank, dim3(blank_workgroups(c->in_frame)), dim3(kBlankThreads), 0, c->st.stream, reinterpret_cast<const float4 *>(c->bl.d_stage.get()),
                       reinterpret_cast<float4 *>(c->route.blank_out), c->in_frame, B.ratio, B.floor, B.guard, c->bl.d_state.get());
    hipLaunchKernelGGL(k_blank_step, dim3(1), dim3(kBlankThreads), 0, c->st.stream, c->bl.d_state.get(), c->bl.rec.dev<BlankRecord>(p), (long long)c->frame_no,
                       c->in_frame, B.rank_q16, B.guard, B.ratio, B.floor);
    c->bl.ran(p, c->frame_no);
}

// IQ balance correction: k_iqbal and k_iqbal_step for the next frame (c->frame_no), on the context's stream behind the ingest
// kernel that staged it, inside that kernel's KIND_INGEST bracket and in front of blank_launch.  In place, on what the ingest
// kernel wrote (ingest_dest).  The pair chains on the device in stream order.  Off: nothing.
void iqbal_launch(sdrx_ctx *c)
{
    if (!c->iq.on)
        return;
    const int p = (int)(c->frame_no & 1ull);
    const IqCfg &Q = c->iq.cfg;
    hipLaunchKernelGGL(k_iqbal, dim3(iq_workgroups(c->in_frame)), dim3(kIqThreads), 0, c->st.stream, ingest_dest(c), c->in_frame, c->iq.d_state.get());
    hipLaunchKernelGGL(k_iqbal_step, dim3(1), dim3(64), 0, c->st.stream, c->iq.d_state.get(), c->iq.rec.dev<IqRecord>(p), (long long)c->frame_no, c->in_frame,
                       Q.mu, Q.min_power);
    c->iq.ran(p, c->frame_no);
}

// Spur canceller: k_notch_corr, k_notch_step and k_notch_apply for the next frame (c->frame_no), on the context's stream behind the
// last kernel of the ingest chain and in front of the shift's, inside the same KIND_INGEST bracket.  In place on the tree's raw
// frame.  Phase, increment and amplitude of every tone chain on the device in stream order.  Off: nothing.
void notch_launch(sdrx_ctx *c)
{
    if (!c->nt.on)
        return;
    const NotchCfg &N = c->nt.cfg;
    const int p = (int)(c->frame_no & 1ull), n = c->root_frame, K = (int)N.n_tones;
    const float2 *tab = c->shift_tables_dev();
    float4 *buf = reinterpret_cast<float4 *>(c->d_raw_tiled.get());
    if (K > 0)
        hipLaunchKernelGGL(k_notch_corr, dim3(notch_workgroups(n)), dim3(kNtThreads), 0, c->st.stream, buf, n, K, c->nt.d_state.get(), tab, c->nt.d_c.get());
    hipLaunchKernelGGL(k_notch_step, dim3(1), dim3(64), 0, c->st.stream, c->nt.d_state.get(), c->nt.d_c.get(), c->nt.d_used.get(), c->nt.rec.dev<NotchRecord>(p),
                       (long long)c->frame_no, n, K, N.mu, N.afc_gain, N.min_coherence, N.max_pull);
    if (K > 0)
        hipLaunchKernelGGL(k_notch_apply, dim3(notch_workgroups(n)), dim3(kNtThreads), 0, c->st.stream, buf, n, K, c->nt.d_state.get(), tab, c->nt.d_used.get());
    c->nt.ran(p, c->frame_no);
}

// Frequency shift: k_shift and k_shift_step for the next frame (c->frame_no), on the context's stream behind the last kernel of
// the ingest chain, inside its KIND_INGEST bracket.  In place on the tree's raw frame (root_frame samples), in front of
// everything that reads it.  Phase and increment chain on the device in stream order.  Off: nothing.
void shift_launch(sdrx_ctx *c)
{
    if (!c->sh.on)
        return;
    const int p = (int)(c->frame_no & 1ull);
    hipLaunchKernelGGL(k_shift, dim3(shift_workgroups(c->root_frame)), dim3(kShThreads), 0, c->st.stream, reinterpret_cast<float4 *>(c->d_raw_tiled.get()),
                       c->root_frame, c->sh.d_state.get(), c->shift_tables_dev());
    hipLaunchKernelGGL(k_shift_step, dim3(1), dim3(64), 0, c->st.stream, c->sh.d_state.get(), c->sh.rec.dev<ShiftRecord>(p), (long long)c->frame_no, c->root_frame);
    c->sh.ran(p, c->frame_no);
}

// The ingest chain of the next frame (c->frame_no) behind the kernel that staged it, inside that kernel's KIND_INGEST bracket: the
// one place that says in which order the stages run.  Every stage that is off launches nothing.  `real_words`, `fmt`: the frame's
// 16-bit words where the first front stage is the real one (front_launch) -- nothing staged a complex frame then, and the IQ
// balance and the blanker launch nothing: blank_plan and iqbal_plan refuse them in front of a real first stage.
void ingest_chain_launch(sdrx_ctx *c, const void *real_words = nullptr, int fmt = -1)
{
    iqbal_launch(c);
    blank_launch(c);
    front_launch(c, real_words, fmt);
    resample_launch(c);
    notch_launch(c);
    shift_launch(c);
}

int queue_fixed_part(sdrx_ctx *c, int p, hipStream_t st); // (sdrx_delivery.hip)
int queue_payloads(sdrx_ctx *c, int p, hipStream_t st);

// The VFO spectra of tree levels lo..hi, whose streams hold frame frames[l] (frames == nullptr: all hold frame f): behind the
// launch that wrote those streams, before anything can overwrite them (frame f + 2 -- the next writer of that parity -- is
// queued behind this launch on the same stream, or waits for ev_tail).  Nothing enabled: nothing is launched.
void spectrum_launch(sdrx_ctx *c, hipStream_t st, int lo, int hi, unsigned long long f, const unsigned long long *frames)
{
    if (c->spec.n_desc == 0)
        return;
    const int first = c->spec.level_begin[(size_t)lo], last = c->spec.level_begin[(size_t)hi + 1];
    if (last <= first)
        return;
    SpecArgs A;
    memset(&A, 0, sizeof A);
    for (int l = 0; l < kMaxLevels; ++l)
        A.frame_level[l] = frames ? frames[l] : f;
    const float *hann = reinterpret_cast<const float *>(c->spec.d_tw + kSpecN);
    hipLaunchKernelGGL(k_spectrum, dim3(last - first), dim3(kSpecThreads), 0, st, c->spec.d_desc + first, A, c->spec.d_tw, hann);
}

// The raw spectrum at sdrj's cadence: `if (count == 4) {emit fftData(samples); count = 0;} count++` once per frame, on the
// frame as the parent-less VFOs get it -- queued first in the frame's own sequence, so that a caller's device frame or the
// tile-layout copy of a DC-corrected one is read before anything else may overwrite it.
void spectrum_raw_step(sdrx_ctx *c, const void *raw, int raw_mode)
{
    if (!c->spec.raw_on)
        return;
    const bool due = c->spec.raw_count == 4;
    if (due)
        c->spec.raw_count = 0;
    c->spec.raw_count++;
    if (!due)
        return;
    SpecArgs A;
    memset(&A, 0, sizeof A);
    A.raw = raw_mode == kRawTiled ? static_cast<const void *>(c->d_raw_tiled) : raw;
    A.raw_mode = raw_mode;
    const float *hann = reinterpret_cast<const float *>(c->spec.d_tw + kSpecN);
    hipLaunchKernelGGL(k_spectrum, dim3(1), dim3(kSpecThreads), 0, c->st.stream, c->spec.d_desc + c->spec.n_desc, A, c->spec.d_tw, hann);
}

// Option watch: the sources of groups g_lo..g_hi (0: the raw frame, 1 + l: the streams of tree level l) that have a watched
// leaf -- one k_watch_psd workgroup per (source, segment), then one k_watch_bands wave per watched leaf of those sources, then
// the drift estimate (sdrx_set_drift) and the band scan (sdrx_set_scan) of those sources that have one.
// Not bracketed: sdrx_get_kernel_times keeps its SDRX_NKERNELS kinds.  Nothing watched: nothing is launched.
void watch_launch_groups(sdrx_ctx *c, hipStream_t st, int g_lo, int g_hi, const WatchArgs &A)
{
    const sdrx_ctx::Watch &W = c->watch;
    const int s0 = W.seg_begin[(size_t)g_lo], s1 = W.seg_begin[(size_t)g_hi + 1];
    const int l0 = W.leaf_begin[(size_t)g_lo], l1 = W.leaf_begin[(size_t)g_hi + 1];
    if (s1 <= s0 || l1 <= l0)
        return;
    const float *hann = reinterpret_cast<const float *>(W.d_tw + kSpecN);
    hipLaunchKernelGGL(k_watch_psd, dim3(s1 - s0), dim3(kSpecThreads), 0, st, W.d_src(), W.d_seg() + s0, A, W.d_tw, hann);
    const int per = kWatchLeafThreads / 64;
    hipLaunchKernelGGL(k_watch_bands, dim3((l1 - l0 + per - 1) / per), dim3(kWatchLeafThreads), 0, st, W.d_src(), W.d_leaf() + l0, l1 - l0, A,
                       W.rec.dev<WatchRecord>(0), W.rec.dev<WatchRecord>(1));
    // option wake: one k_watch_wake workgroup per leaf of those sources that is under the device's control, on the records
    // k_watch_bands has just left -- the decision for the frame those sources hold, and on a change of state the leaf's flag
    // words and state regions (where this call sits in the frame: the argument above enqueue_frame).  Nothing before the first
    // sdrx_set_wake that switched a leaf on; not bracketed either.
    const sdrx_ctx::Wake &K = c->wake;
    if (K.n_ctl > 0) {
        const int w0 = K.begin[(size_t)g_lo], w1 = K.begin[(size_t)g_hi + 1];
        if (w1 > w0)
            hipLaunchKernelGGL(k_watch_wake, dim3(w1 - w0), dim3(kWakeThreads), 0, st, W.d_src(), K.d_leaf, K.d_state, K.d_list + w0, K.d_fill, A,
                               W.rec.dev<WatchRecord>(0), W.rec.dev<WatchRecord>(1), K.rec.dev<WakeRecord>(0), K.rec.dev<WakeRecord>(1));
    }
    // drift estimate: one k_watch_drift workgroup per (source of those groups with a template, block of shifts), on the PSD
    // k_watch_psd has just left.  Nothing before the first sdrx_set_drift; not bracketed either.
    const sdrx_ctx::Drift &D = c->drift;
    if (!D.begin.empty()) {
        const int b0 = D.begin[(size_t)g_lo], b1 = D.begin[(size_t)g_hi + 1];
        if (b1 > b0)
            hipLaunchKernelGGL(k_watch_drift, dim3(b1 - b0), dim3(kSpecThreads), 0, st, D.d_src(), D.d_blk(W.n_src_slots) + b0, A, D.rec.dev<DriftRecord>(0),
                               D.rec.dev<DriftRecord>(1));
    }
    // band scan: one k_watch_scan workgroup per source of those groups with the scan on, on the same PSD.  Nothing before the
    // first sdrx_set_scan; not bracketed either.
    const sdrx_ctx::Scan &S = c->scan;
    if (S.begin.empty())
        return;
    const int c0 = S.begin[(size_t)g_lo], c1 = S.begin[(size_t)g_hi + 1];
    if (c1 > c0)
        hipLaunchKernelGGL(k_watch_scan, dim3(c1 - c0), dim3(kSpecThreads), 0, st, S.d_src() + c0, A, S.rec.dev<ScanRecord>(0), S.rec.dev<ScanRecord>(1));
}
// ... of the VFO streams of tree levels lo..hi, where spectrum_launch reads them (the same frames per level)
void watch_launch(sdrx_ctx *c, hipStream_t st, int lo, int hi, unsigned long long f, const unsigned long long *frames)
{
    if (c->watch.src_ids.empty())
        return;
    WatchArgs A;
    memset(&A, 0, sizeof A);
    for (int l = 0; l < kMaxLevels; ++l)
        A.frame_level[l] = frames ? frames[l] : f;
    watch_launch_groups(c, st, 1 + lo, 1 + hi, A);
}
// ... and of the raw frame, where spectrum_raw_step reads it: first in the frame's own sequence
void watch_raw_step(sdrx_ctx *c, const void *raw, int raw_mode)
{
    if (c->watch.src_ids.empty())
        return;
    WatchArgs A;
    memset(&A, 0, sizeof A);
    A.raw = raw_mode == kRawTiled ? static_cast<const void *>(c->d_raw_tiled) : raw;
    A.raw_mode = raw_mode;
    A.frame_raw = c->frame_no;
    watch_launch_groups(c, c->st.stream, 0, 0, A);
}

// Option squelch: the gate of frame `frame`, on the stream -- and behind the launch -- that completed its payloads and meter
// records: decide + scan (one workgroup), then the gather of the open leaves into d_pack[p] (squelch.hip).  Not bracketed:
// sdrx_get_kernel_times keeps its SDRX_NKERNELS kinds.  PRE (option preroll): the two launches in their second form -- the gather
// also reads frame - 1's payloads in d_pay[p ^ 1]; AUTO (option squelch_auto): the scan with the floor records, the gather as without.
template <bool PRE, bool AUTO, bool PARK>
void launch_gate(sdrx_ctx *c, hipStream_t ts, unsigned long long frame)
{
    const int n = (int)c->publish_order.size();
    const int p = (int)(frame & 1ull);
    unsigned char *dir = c->d_pay[p] + c->sq.dir_off;
    SqPre<PRE> X;
    SqAut<AUTO> A;
    if constexpr (PRE)
        X = {c->sq.d_prev, c->d_pay[p ^ 1]};
    if constexpr (AUTO)
        A = {c->sq.d_auto};
    hipLaunchKernelGGL((k_squelch_scan<PRE, AUTO, PARK>), dim3(1), dim3(kSqThreads), 0, ts, c->sq.d_leaves, c->sq.d_cfg, c->sq.d_hang, c->d_pay[p], dir, n,
                       (long long)frame, X, A, park_arg<PARK>(c, c->park.o_sq));
    hipLaunchKernelGGL(k_squelch_gather<PRE>, dim3(n, c->sq.tiles, PRE ? 2 : 1), dim3(256), 0, ts, c->sq.d_leaves, c->d_pay[p], dir, c->sq.d_pack[p], X);
}
void squelch_gate(sdrx_ctx *c, hipStream_t ts, unsigned long long frame)
{
    if (!c->opt_squelch || c->publish_order.empty())
        return;
    auto form = [&](auto PARK) {
        if (c->opt_preroll)
            c->opt_squelch_auto ? launch_gate<true, true, PARK()>(c, ts, frame) : launch_gate<true, false, PARK()>(c, ts, frame);
        else
            c->opt_squelch_auto ? launch_gate<false, true, PARK()>(c, ts, frame) : launch_gate<false, false, PARK()>(c, ts, frame);
    };
    if (c->opt_park)
        form(std::true_type());
    else
        form(std::false_type());
}

// Option agc: the gain step of frame `frame` (agc.hip), on the stream -- and behind the launch -- that completed its meter
// records, directly behind its gate: wherever squelch_gate is called.  It writes the gains frame + 1 demodulates with: every
// launch that reads a gain for frame + 1 comes behind it (the argument above enqueue_frame).  Not bracketed, like the gate.
void agc_step(sdrx_ctx *c, hipStream_t ts, unsigned long long frame)
{
    if (!c->opt_agc || c->agc.n == 0)
        return;
    const int p = (int)(frame & 1ull);
    AgcRecord *rec = reinterpret_cast<AgcRecord *>(c->d_pay[p] + c->agc.rec_off);
    const dim3 grid((c->agc.n + kAgcThreads - 1) / kAgcThreads);
    if (c->opt_park)
        hipLaunchKernelGGL(k_agc_step<true>, grid, dim3(kAgcThreads), 0, ts, c->agc.d_leaves, c->agc.d_cfg, c->agc.d_quiet, c->d_pay[p], rec, c->agc.n,
                           park_arg<true>(c, 0));
    else
        hipLaunchKernelGGL(k_agc_step<false>, grid, dim3(kAgcThreads), 0, ts, c->agc.d_leaves, c->agc.d_cfg, c->agc.d_quiet, c->d_pay[p], rec, c->agc.n,
                           park_arg<false>(c, 0));
}

// One block-per-tile launch of the leaf tail (late decimation / demodulation / long audio low-pass / compress) for `frame`:
// `n_blocks` entries of the work list `w` (k_lpf_long with option meter: and of the record offsets `mrel`).
void launch_block_list(sdrx_ctx *c, const LaunchB &L, hipStream_t ts, unsigned long long frame, const BlockWork *w, const int *mrel, int n_blocks)
{
    Bracket b(c, ts, bracket_kind(L.kind), L.alg_bytes);
    const dim3 grid(n_blocks);
    const unsigned char *desc = c->arena + L.off_desc;
    with_variant(c, [&](auto EXACT, auto, auto METER, auto PARK) {
        if (L.kind == KIND_LATE_DEC && c->late4)
            hipLaunchKernelGGL((k_late_decimate4<EXACT(), PARK()>), grid, dim3(64), L.lds_bytes, ts, reinterpret_cast<const K2aVfo *>(desc), w, frame,
                               park_arg<PARK()>(c, c->park.o_2a));
        else if (L.kind == KIND_LATE_DEC)
            hipLaunchKernelGGL((k_late_decimate<EXACT(), PARK()>), grid, dim3(256), L.lds_bytes, ts, reinterpret_cast<const K2aVfo *>(desc), w, frame,
                               park_arg<PARK()>(c, c->park.o_2a));
        else if (L.kind == KIND_DEMOD)
            hipLaunchKernelGGL((k_usb_demod<EXACT(), METER(), PARK()>), grid, dim3(256), 0, ts, reinterpret_cast<const K2Vfo *>(desc), w, frame,
                               park_arg<PARK()>(c, c->park.o_2));
        else if (L.kind == KIND_LPF_LONG)
            hipLaunchKernelGGL((k_lpf_long<EXACT(), METER(), PARK()>), grid, dim3(256), L.lds_bytes, ts, reinterpret_cast<const K4Vfo *>(desc), w, frame, mrel,
                               park_arg<PARK()>(c, c->park.o_4));
        else if (L.kind == KIND_DETECT_AM) { // the carrier's partials of every block, then the blocks themselves
            hipLaunchKernelGGL((k_env_sum<PARK()>), grid, dim3(kDetThreads), 0, ts, reinterpret_cast<const K5Vfo *>(desc), w, frame, park_arg<PARK()>(c, c->park.o_5));
            hipLaunchKernelGGL((k_detect<kDetAm, METER(), PARK()>), grid, dim3(kDetThreads), 0, ts, reinterpret_cast<const K5Vfo *>(desc), w, frame,
                               park_arg<PARK()>(c, c->park.o_5));
        } else if (L.kind == KIND_DETECT_FM)
            hipLaunchKernelGGL((k_detect<kDetFm, METER(), PARK()>), grid, dim3(kDetThreads), 0, ts, reinterpret_cast<const K5Vfo *>(desc), w, frame,
                               park_arg<PARK()>(c, c->park.o_5));
        else if (L.kind == KIND_DETECT_AM_POST) { // the same two passes, the second one through the post-detection filter
            hipLaunchKernelGGL((k_env_sum<PARK()>), grid, dim3(kDetThreads), 0, ts, reinterpret_cast<const K5Vfo *>(desc), w, frame, park_arg<PARK()>(c, c->park.o_5));
            hipLaunchKernelGGL((k_detect_post<kDetAm, METER(), PARK()>), grid, dim3(kDetThreads), 0, ts, reinterpret_cast<const K5Vfo *>(desc),
                               reinterpret_cast<const K5Post *>(c->arena + c->off_k5post), w, frame, park_arg<PARK()>(c, c->park.o_5));
        } else if (L.kind == KIND_DETECT_FM_POST)
            hipLaunchKernelGGL((k_detect_post<kDetFm, METER(), PARK()>), grid, dim3(kDetThreads), 0, ts, reinterpret_cast<const K5Vfo *>(desc),
                               reinterpret_cast<const K5Post *>(c->arena + c->off_k5post), w, frame, park_arg<PARK()>(c, c->park.o_5));
        else
            hipLaunchKernelGGL((k_compress<METER(), PARK()>), grid, dim3(256), 0, ts, reinterpret_cast<const K3Vfo *>(desc), w, frame,
                               park_arg<PARK()>(c, c->park.o_3));
    });
}
// ... the whole list finalize built
void launch_block_kernel(sdrx_ctx *c, const LaunchB &L, hipStream_t ts, unsigned long long frame)
{
    launch_block_list(c, L, ts, frame, reinterpret_cast<const BlockWork *>(c->arena + L.off_work),
                      c->opt_meter ? reinterpret_cast<const int *>(c->arena + L.off_mrel) : nullptr, L.n_blocks);
}

// One k_mix_decimate launch of a tree level for `frame`: `n_work` entries of the work list `w`.
void launch_mix_list(sdrx_ctx *c, const Launch1 &L, unsigned long long frame, const K1Work *w, int n_work, const void *raw, int raw_mode)
{
    Bracket b(c, c->st.stream, L.kind, L.alg_bytes);
    const K1Vfo *k1 = reinterpret_cast<const K1Vfo *>(c->arena + c->off_k1vfo);
    const void *lraw = L.level == 0 ? raw : nullptr;
    const int lmode = L.level == 0 ? raw_mode : kRawTiled;
    with_variant(c, [&](auto EXACT, auto ROT, auto METER, auto PARK) {
        if (L.level == 0)
            hipLaunchKernelGGL((k_mix_decimate<EXACT(), 0, ROT(), METER(), PARK()>), dim3(n_work), dim3(64), L.lds_bytes, c->st.stream, k1, w, frame, lraw, lmode,
                               park_arg<PARK()>(c, 0));
        else
            hipLaunchKernelGGL((k_mix_decimate<EXACT(), 1, ROT(), METER(), PARK()>), dim3(n_work), dim3(64), L.lds_bytes, c->st.stream, k1, w, frame, lraw, lmode,
                               park_arg<PARK()>(c, 0));
    });
}

// One step of the frame pipeline: every in-flight frame (and the new one, if `have_new`) moves through
// the tree level it has reached -- ONE k_mix_levels launch over the contiguous range of those levels --
// and the frame that thereby leaves the last level gets its leaf tail (late decimation, demodulation,
// compress) right behind that launch.
// With LevelPlan::tail the demodulation of that frame is one more stage instead: it runs inside the NEXT step's launch
// (k_levels_tail), its long audio low-pass (k_lpf_long) right behind that launch; the late decimation and compress stay
// behind the launch that finished the frame's levels.
int pipeline_step(sdrx_ctx *c, bool have_new, const void *raw, int raw_mode)
{
    const LevelPlan &P = c->fp;
    const int n_levels = (int)P.part_begin.size();
    if (have_new)
        c->pipe.push_back({c->frame_no, 0});
    if (c->pipe.empty())
        return SDRX_OK;
    LevelArgs A;
    memset(&A, 0, sizeof A);
    A.raw = raw;
    A.raw_mode = raw_mode;
    int lo = n_levels, hi = -1;
    bool dm = false;             // the oldest frame is due for its demodulation (P.tail only)
    unsigned long long f_dm = 0;
    for (const InFlight &q : c->pipe) {
        if (q.next == n_levels) {
            dm = true;
            f_dm = q.f;
            continue;
        }
        lo = std::min(lo, q.next);
        hi = std::max(hi, q.next);
        A.frame_level[q.next] = q.f;
    }
    const K1Vfo *k1 = reinterpret_cast<const K1Vfo *>(c->arena + c->off_k1vfo);
    const K1Work *items = reinterpret_cast<const K1Work *>(c->arena + P.off_items);
    const int *item_level = reinterpret_cast<const int *>(c->arena + P.off_item_level);
    int64_t bytes = dm ? P.dm_bytes : 0;
    for (int j = lo; j <= hi; ++j)
        bytes += P.part_bytes[(size_t)j];
    if (!P.tail) {
        const int first = std::min(P.part_begin[(size_t)lo], P.part_begin[(size_t)hi]), last = std::max(P.part_end[(size_t)lo], P.part_end[(size_t)hi]);
        Bracket b(c, c->st.stream, lo != hi ? KIND_LEVELS : lo == 0 ? KIND_MIX_ROOT : KIND_MIX_SUB, bytes);
        const int *list = reinterpret_cast<const int *>(c->arena + P.off_list) + first;
        const dim3 grid(last - first);
        with_variant(c, [&](auto EXACT, auto ROT, auto METER, auto PARK) {
            hipLaunchKernelGGL((k_mix_levels<EXACT(), ROT(), METER(), PARK()>), grid, dim3(64), P.lds_bytes, c->st.stream, k1, items, item_level, list, A,
                               park_arg<PARK()>(c, 0));
        });
    } else {
        // the list is [level n-1 | ... | level 0 | demodulation]: the range runs from the deepest level with a frame to the
        // demodulation (or to the shallowest level with a frame); levels inside it without a frame (the pipeline draining)
        // are masked out by `active`
        LevelTailArgs T;
        memset(&T, 0, sizeof T);
        T.L = A;
        T.frame_tail = f_dm;
        T.lds_wave = P.lds_wave;
        T.active = dm ? 1 << kMaxLevels : 0;
        for (int j = lo; j <= hi; ++j)
            T.active |= 1 << j;
        const int first = hi >= 0 ? P.wg_begin[(size_t)hi] : P.dm_begin, last = dm ? P.dm_end : P.wg_end[(size_t)lo];
        Bracket b(c, c->st.stream, hi < 0 || lo != hi || dm ? KIND_LEVELS : lo == 0 ? KIND_MIX_ROOT : KIND_MIX_SUB, bytes);
        const TailWg *wgs = reinterpret_cast<const TailWg *>(c->arena + P.off_wgs) + first;
        const LaunchB &D = *std::find_if(c->lb.begin(), c->lb.end(), [](const LaunchB &L) { return L.kind == KIND_DEMOD; });
        const K2Vfo *k2 = reinterpret_cast<const K2Vfo *>(c->arena + D.off_desc);
        const BlockWork *dwork = reinterpret_cast<const BlockWork *>(c->arena + D.off_work);
        const dim3 grid(last - first);
        with_variant(c, [&](auto EXACT, auto ROT, auto METER, auto PARK) {
            hipLaunchKernelGGL((k_levels_tail<EXACT(), ROT(), METER(), PARK()>), grid, dim3(256), P.tail_lds, c->st.stream, k1, items, item_level, wgs, k2, dwork,
                               T, park_arg<PARK()>(c, c->park.o_2));
        });
    }
    if (dm)
        for (const LaunchB &L : c->lb)
            if (L.kind == KIND_LPF_LONG)
                launch_block_kernel(c, L, c->st.stream, f_dm);
    if (dm) { // that launch completed frame f_dm's payloads and records: its gate, and its gain step
        squelch_gate(c, c->st.stream, f_dm);
        agc_step(c, c->st.stream, f_dm);
    }
    if (hi >= 0) {
        spectrum_launch(c, c->st.stream, lo, hi, 0, A.frame_level);
        if (!c->opt_wake) // (option wake: behind the leaf tail below -- the argument above enqueue_frame)
            watch_launch(c, c->st.stream, lo, hi, 0, A.frame_level);
    }
    if (dm)
        c->pipe.erase(c->pipe.begin());
    for (InFlight &q : c->pipe)
        q.next++;
    if (!c->pipe.empty() && c->pipe.front().next == n_levels) { // the oldest frame has passed its last level: its leaf tail, now
        const unsigned long long f = c->pipe.front().f;
        for (const LaunchB &L : c->lb)
            if (!P.tail || (L.kind != KIND_DEMOD && L.kind != KIND_LPF_LONG))
                launch_block_kernel(c, L, c->st.stream, f);
        if (!P.tail) {
            squelch_gate(c, c->st.stream, f);
            agc_step(c, c->st.stream, f);
            c->pipe.erase(c->pipe.begin());
        }
    }
    if (hi >= 0 && c->opt_wake) // the watch of the streams this step wrote, with its wake: behind the tail, gate and step of the
                                // frame that has just left the last level, in front of the next step's launch
        watch_launch(c, c->st.stream, lo, hi, 0, A.frame_level);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(c, SDRX_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    return SDRX_OK;
}

// run every in-flight frame to its end
int pipeline_flush(sdrx_ctx *c)
{
    while (!c->pipe.empty()) {
        const int rc = pipeline_step(c, false, nullptr, kRawTiled);
        if (rc)
            return rc;
    }
    return SDRX_OK;
}

// One frame: [wait for the tail of frame f-2] -> ingest -> one k_mix_decimate launch per tree level on
// `stream`; then the leaf tail (late decimation, demodulation, compress) -- on `tail_stream` behind an
// event when the pipeline option is on, so that it runs beside the NEXT frame's levels -- and, for a
// frame that came through sdrx_submit*, the payload copy on `copy_stream` behind the tail.
//
// What makes the two-stream form safe (frame f, parity p = f & 1):
//   * the leaf streams of parity p are written by the levels of f and read by the tail of f: the tail
//     waits for ev_levels[p]; their next writer is frame f+2, whose levels wait for ev_tail[p] first;
//   * the history prefix of the parity-(p^1) leaf streams is written by the tail of f and read by the
//     tail of f+1: same stream, in order (the levels of f+1 write only the data part behind it);
//   * half-band state, NCO tables and the parents' streams are touched by the levels only;
//   * d_pay[p] is written by the tail of f and read by the copy of f; its next writer is the tail of
//     f+2, which the host does not submit before frame f was delivered (SDRX_MAX_IN_FLIGHT = 2).
//   * option squelch: d_pack[p] and the directory (inside d_pay[p]) are written by the gate of f, behind its tail on the
//     tail's stream, and read by the two copies of f -- queue_fixed_part at submit, queue_payloads from sdrx_wait
//     (sdrx_delivery.hip) -- the same argument: their next writer is the gate of f+2.  hang_left is one array: gates run in
//     frame order on one stream.
//   * option preroll: the gate of f also READS the payloads of f-1 in d_pay[p ^ 1], whose next writer is frame f+1 -- every
//     launch that writes a payload of f+1 must come behind the gate of f.  prev_open is one array, as hang_left.  Path by path:
//       - one launch per level, one stream (below, !pipe): tail(f), gate(f), levels(f+1), tail(f+1) in order, whichever kernel
//         writes the payloads (fuse_demod leaves write theirs in the levels);
//       - two streams (pipe): the tails and gates of all frames are in order on tail_stream, and without fuse_demod only the
//         tail writes d_pay.  With fuse_demod leaves the levels of f+1 on `stream` write it, and they wait only for ev_tail of
//         f-1: with preroll they also wait for ev_tail[p ^ 1], recorded behind the gate of f (preroll_fused below) -- which
//         takes the overlap away for exactly that combination;
//       - pipeline_step with k_mix_levels: the launch of step k runs level l of frame k-l, then the block kernels and the gate
//         of the frame g that left the last level.  Block kernels of g+1 come in step k+1: behind gate(g).  A fuse_demod leaf
//         on level n-1 writes g's payload in step k and g+1's in step k+1: behind gate(g).  One on level n-2 writes g+1's payload
//         in step k's launch, BEFORE gate(g): with preroll such a tree does not use the software pipeline (build_level_plan);
//       - pipeline_step with k_levels_tail: the demodulation blocks of f ride in the launch of the step after f's last level,
//         then k_lpf_long(f), gate(f), and only then the compress / late-decimation launches of f+1 in the same step; the
//         demodulation of f+1 is in the next step's launch.  fuse_demod leaves of f+1 would write their payload inside the
//         launch that carries f's demodulation, before gate(f): with preroll a tree with such leaves keeps k_mix_levels +
//         k_usb_demod in every arithmetic (build_level_plan; the rule option meter has for the exact one);
//       - paths mix only through pipeline_flush, which runs every gate still outstanding, in frame order, on `stream`; the
//         two-stream form never enters pipeline_step.  sdrx_fetch, queue_fixed_part and queue_payloads read d_pack and the
//         directory only.
//   * option agc: the step of f (agc_step, directly behind the gate of f wherever that is launched) reads the meter records of
//     f and WRITES the gain floats in the K2Vfo / K4Vfo descriptors -- the value frame f+1 demodulates with.  It must come
//     behind every launch that completes a meter record of f (the gate's own condition) and in front of every launch that reads
//     a gain for f+1; no launch may still read a gain for f (all of them completed f's records, so they are in front).  quiet_run
//     is one array, as hang_left.  The step's record goes to d_pay[p] beside the meter records: next writer the step of f+2.
//     Who reads a gain: k_usb_demod / the demodulation blocks of k_levels_tail, k_lpf_long, and the mix waves of fuse_demod
//     leaves.  Path by path, as for preroll:
//       - one launch per level, one stream: tail(f), gate(f), step(f), levels(f+1), tail(f+1) in order;
//       - two streams (pipe): tails, gates and steps of all frames are in order on tail_stream, and without fuse_demod only the
//         tail reads gains.  With fuse_demod leaves the levels of f+1 on `stream` read them: they wait for ev_tail[p ^ 1],
//         recorded behind the step of f (the wait preroll has) -- which takes the overlap away for that combination;
//       - pipeline_step with k_mix_levels: the block kernels of g+1 come in step k+1, behind step(g).  A fuse_demod leaf on level
//         n-1 demodulates g in step k's launch and g+1 in step k+1's: behind step(g).  One on level n-2 demodulates g+1 in step
//         k's launch, in FRONT of step(g): with agc such a tree does not use the software pipeline (build_level_plan);
//       - pipeline_step with k_levels_tail: the demodulation blocks of f ride in the launch of the step after f's last level,
//         then k_lpf_long(f), gate(f), step(f); the demodulation of f+1 is in the next step's launch, k_lpf_long(f+1) behind
//         that.  fuse_demod leaves of f+1 would demodulate inside the launch that carries f's demodulation, in front of
//         step(f): with agc a tree with such leaves keeps k_mix_levels + k_usb_demod (build_level_plan);
//       - pipeline_flush runs every step still outstanding behind its gate, in frame order; sdrx_set_gains, sdrx_set_agc and
//         sdrx_set_active drain first, and their job kernels run on `stream` behind everything.  The catch-up of frame K-1
//         (sdrx_set_active) launches no step: the leaf was parked in K-1, which is no observation.
//   * option wake: the wake step of frame f for a leaf (k_watch_wake, behind k_watch_bands on the leaf's source: wherever
//     watch_launch_groups is called) WRITES the leaf's flag words (Park::d_act, item_level[]), and when the leaf wakes its state
//     regions of both parities, its gate words (hang_left, prev_open, the floor record), quiet_run and K1Vfo::origin.  The source
//     of frame f is complete before the leaf's own mix items of f run, so the step can sit -- and must sit -- in two places at
//     once: BEHIND every launch that reads one of those words for frame f-1 (the leaf's mix items, block kernels, gate and AGC
//     step) and IN FRONT of every launch that reads one for frame f.  Flags and origin reach the later launches through the
//     constant path, as the gains of the AGC step and the jobs of k_vfo_retune do: a kernel boundary on one stream, or an
//     event between two.  The step's record goes to a buffer of the frame's parity: next writer the step of f+2.  Path by path:
//       - one launch per level, one stream: the raw watch with its wake stays in front of level 0 (watch_raw_step: the
//         parent-less leaves run in level 0), and the watch of level l's streams, with its wake, comes directly behind level l's
//         launch -- in front of level l+1, where the children of those streams run.  Everything of f-1 (levels, tail, gate,
//         step) is in front of all of it, the tail, gate and step of f behind all of it.  The watch_launch at the end has nothing
//         left; records and PSDs are what they were (the same streams, complete, read by the same kernels);
//       - two streams (pipe): the tail, gate and step of f-1 on tail_stream read words the wake steps of f write on `stream`:
//         the levels of f also wait for ev_tail[p ^ 1] (the wait preroll_fused has), for every tree.  The overlap of the tail
//         with the next frame's levels is lost for this option.  The tail of f waits for ev_levels[p], recorded behind the
//         last wake step of f;
//       - pipeline_step with k_mix_levels: step k's launch runs level l of frame k-l; the leaves all sit on the last level
//         n-1 (build_level_plan: any other tree runs one launch per level under this option), so their sources are the level
//         n-2 streams, which hold frame k-n+2 behind step k's launch, and their items of that frame run in step k+1's launch.
//         The watch with its wake therefore goes to the END of the step: behind the block kernels, gate and step of the
//         frame k-n+1 that has just left the last level (they read the words as the wake of that frame left them), in front of
//         step k+1's launch.  A one-level tree does not use pipeline_step;
//       - pipeline_step with k_levels_tail: not used under this option (build_level_plan) -- the demodulation of frame g rides in
//         the launch that also runs the last level of g+1, one flag word cannot serve both;
//       - pipeline_flush steps levels that hold a frame; a leaf's source level holds none once its frame has passed, so no
//         wake step runs twice for a frame.  sdrx_set_wake, sdrx_set_active and the other setters drain first.
int enqueue_frame(sdrx_ctx *c, const void *raw, int raw_mode, bool egress)
{
    const int p = (int)(c->frame_no & 1ull);
    const bool pipe = c->opt_pipeline != 0;
    if (pipe && c->st.tail_recorded[p])
        HIPCHK(c, hipStreamWaitEvent(c->st.stream, c->st.ev_tail[p], 0));
    if (pipe && (((c->opt_preroll || c->opt_agc) && c->sq.preroll_fused) || c->opt_wake) && c->st.tail_recorded[p ^ 1])
        // the levels write d_pay[p], which the previous gate reads -- and read the gains its step writes; option wake: the wake
        // steps of this frame write the flag words and state regions the previous tail, gate and step read
        HIPCHK(c, hipStreamWaitEvent(c->st.stream, c->st.ev_tail[p ^ 1], 0));
    if (c->tiled_ingest() && raw_mode != kRawTiled) {
        // With any stage of the ingest chain on, a natural-order frame (cf32, or a shared context's bytes) is at the input rate:
        // one layout pass into the route's first buffer, then the chain (ingest_chain_launch), in front of everything that reads
        // the tree's raw frame.  (A frame of integer samples came through enqueue_samples_device, which did both: kRawTiled.)
        Bracket b(c, c->st.stream, KIND_INGEST, 0);
        const int n_pairs = c->in_frame / 2;
        if (raw_mode == kRawF32)
            hipLaunchKernelGGL(k_ingest_f32, dim3((n_pairs + 255) / 256), dim3(256), 0, c->st.stream, reinterpret_cast<const float4 *>(raw), ingest_dest(c),
                               n_pairs);
        else
            hipLaunchKernelGGL(k_ingest_samples<SDRX_FMT_CU8>, dim3((n_pairs + 255) / 256), dim3(256), 0, c->st.stream,
                               reinterpret_cast<const unsigned *>(raw), ingest_dest(c), n_pairs);
        ingest_chain_launch(c);
        raw_mode = kRawTiled;
    }
    spectrum_raw_step(c, raw, raw_mode);
    watch_raw_step(c, raw, raw_mode);
    // A few parent-less VFOs (the reference's 2-3 mains) read the caller's frame as it is; a wide
    // level 0 (the flat workloads) is bandwidth bound and wants coalesced reads: one layout pass
    // natural order -> tile layout first.
    if (raw_mode != kRawTiled && !c->root_direct) {
        Bracket b(c, c->st.stream, KIND_INGEST, 0);
        const int n_pairs = c->root_frame / 2;
        if (raw_mode == kRawF32)
            hipLaunchKernelGGL(k_ingest_f32, dim3((n_pairs + 255) / 256), dim3(256), 0, c->st.stream,
                               reinterpret_cast<const float4 *>(raw), reinterpret_cast<float4 *>(c->d_raw_tiled.get()), n_pairs);
        else
            hipLaunchKernelGGL(k_ingest_samples<SDRX_FMT_CU8>, dim3((n_pairs + 255) / 256), dim3(256), 0, c->st.stream,
                               reinterpret_cast<const unsigned *>(raw), reinterpret_cast<float4 *>(c->d_raw_tiled.get()), n_pairs);
        raw_mode = kRawTiled;
    }
    const bool shared_launches = c->fp.usable && c->opt_fuse && !pipe && !egress;
    if (!shared_launches)
        if (int rc = pipeline_flush(c))
            return rc;
    if (shared_launches) {
        // Frames that stay on the device and are queued back to back share launches: level l of frame
        // k - l runs in the launch that frame k enters with, and the frame that leaves the last level
        // gets its leaf tail right behind it.  (A frame whose payloads must leave now -- sdrx_process*,
        // sdrx_submit* -- runs through its own launches below: nothing to overlap it with.)
        const int rc = pipeline_step(c, true, raw, raw_mode);
        if (rc)
            return rc;
        if (!c->opt_frame_pipeline)
            if (int rc2 = pipeline_flush(c))
                return rc2;
        c->frame_no++;
        c->pending_fetch = true;
        return SDRX_OK;
    }
    for (const Launch1 &L : c->l1) {
        launch_mix_list(c, L, c->frame_no, reinterpret_cast<const K1Work *>(c->arena + L.off_work), L.n_work, raw, raw_mode);
        if (c->opt_wake) // the watch of the streams this level wrote, with its wake: in front of the level their children run in
            watch_launch(c, c->st.stream, L.level, L.level, c->frame_no, nullptr);
    }
    hipStream_t ts = pipe ? c->st.tail_stream : c->st.stream;
    if (pipe) {
        HIPCHK(c, hipEventRecord(c->st.ev_levels[p], c->st.stream));
        HIPCHK(c, hipStreamWaitEvent(ts, c->st.ev_levels[p], 0));
    }
    for (const LaunchB &L : c->lb)
        launch_block_kernel(c, L, ts, c->frame_no);
    squelch_gate(c, ts, c->frame_no);
    agc_step(c, ts, c->frame_no);
    spectrum_launch(c, ts, 0, c->n_levels - 1, c->frame_no, nullptr);
    if (!c->opt_wake) // (option wake: every level's watch is behind its own launch above)
        watch_launch(c, ts, 0, c->n_levels - 1, c->frame_no, nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(c, SDRX_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    if (pipe || egress) {
        HIPCHK(c, hipEventRecord(c->st.ev_tail[p], ts));
        c->st.tail_recorded[p] = pipe;
    }
    // How the payloads leave (measured, traced: profiles/README.md round 5; tools/copy_overlap_probe.hip).  Normally queued here,
    // behind the frame's last kernel: hipMemcpyAsync on a copy stream, which the runtime hands to an SDMA engine -- the kernels of
    // the next frame run beside it, config 3 from host floats goes at PCIe speed (0.30 ms per pipelined frame = the 15 MB copy).
    // A frame that carries the DC-bias recurrence did not get to run beside a copy queued that way (0.59-0.82 ms per frame,
    // about the SUM of its parts), nor beside a copy kernel of ours (a kernel cannot retire beside one): for those frames the copy
    // is issued by sdrx_wait, when the host has seen the frame's last kernel end -- 0.34 ms per frame.  (The float path would lose
    // by that, 0.38 vs 0.30: between two waits the copy engine idles.)
    // Option squelch: how much leaves is a device result.  Here only the fixed-size part -- meter records and directory -- is
    // queued behind the gate (queue_fixed_part); sdrx_wait reads packed_bytes from it and issues the one copy of the packed payloads
    // (queue_payloads: the owed-copy form, whatever kind of frame this is).
    hipStream_t cs = p ? c->st.copy_stream2 : c->st.copy_stream;
    if (egress && c->opt_squelch) {
        HIPCHK(c, hipStreamWaitEvent(cs, c->st.ev_tail[p], 0));
        if (int rc = queue_fixed_part(c, p, cs))
            return rc;
        HIPCHK(c, hipEventRecord(c->sq.ev_dir[p], cs));
        c->copy_owed[p] = true;
    } else if (egress && c->long_frame) {
        c->copy_owed[p] = true;
    } else if (egress) {
        HIPCHK(c, hipStreamWaitEvent(cs, c->st.ev_tail[p], 0));
        if (int rc = queue_payloads(c, p, cs))
            return rc;
        HIPCHK(c, hipEventRecord(c->st.ev_copied[p], cs));
    }
    c->in_flight += egress;
    c->frame_no++;
    c->pending_fetch = !egress;
    return SDRX_OK;
}

// every frame handed to the context is complete and every stream of the context idle afterwards
int drain(sdrx_ctx *c)
{
    if (int rc = pipeline_flush(c))
        return rc;
    for (hipStream_t st : {c->st.stream, c->st.tail_stream, c->st.copy_stream, c->st.copy_stream2})
        HIPCHK(c, hipStreamSynchronize(st));
    drain_events(c);
    return SDRX_OK;
}


// the device buffers of host-fed frames, both parities: all four hold `n_complex` samples, or (an allocation failed) none exists
int ensure_raw(sdrx_ctx *c, size_t n_complex)
{
    hipError_t e = hipSuccess;
    for (int p = 0; p < 2 && e == hipSuccess; ++p)
        if ((e = c->d_raw[p].reserve(n_complex)) == hipSuccess)
            e = c->d_raw_u8[p].reserve(n_complex * 2);
    if (e == hipSuccess)
        return SDRX_OK;
    for (int p = 0; p < 2; ++p) {
        c->d_raw[p].reset();
        c->d_raw_u8[p].reset();
    }
    return fail(c, SDRX_EHIP, "no device memory for the frame buffers: %s", hipGetErrorString(e));
}

bool real_format(int fmt) { return fmt == SDRX_FMT_RS16 || fmt == SDRX_FMT_RU12; }

// `fmt`: the format of the frame's samples, -1 for cf32
int check_frame_call(sdrx_ctx *c, const char *what, const void *ptr, int n_complex, bool sync_call, int fmt = -1)
{
    if (c && c->broken)
        return fail(c, SDRX_EHIP, "%s: injected fault (SDRX_FAULT_WAIT): the context is unusable", what);
    if (!c)
        return SDRX_EINVAL;
    if (!ptr)
        return fail(c, SDRX_EINVAL, "%s: null frame pointer", what);
    if (!c->finalized)
        return fail(c, SDRX_ESTATE, "%s before sdrx_finalize", what);
    if (real_format(fmt) != (c->fr.on && c->fr.plan.real != 0))
        return fail(c, SDRX_EINVAL,
                    real_format(fmt) ? "%s: fmt must be SDRX_FMT_CU8 (0), SDRX_FMT_CS8 (1) or SDRX_FMT_CS16 (2) here: the real formats SDRX_FMT_RS16 (3) "
                                       "and SDRX_FMT_RU12 (4) need a front stage with real_input = 1 (sdrx_set_front)"
                                     : "%s: this context's front stage takes real samples (SDRX_FMT_RS16, SDRX_FMT_RU12) only",
                    what);
    if (n_complex != c->in_frame && c->fr.on)
        return fail(c, SDRX_EINVAL, "frame of %d samples: with a front stage of %d half-band(s) a frame has %d (%d behind it)", n_complex, c->fr.plan.stages,
                    c->in_frame, c->fr.plan.n0);
    if (n_complex != c->in_frame && c->rs.on)
        return fail(c, SDRX_EINVAL, "frame of %d samples: with the resampler %d -> %d S/s a frame has %d (for the VFOs' %d)", n_complex, c->rs.plan.fs_in,
                    c->rs.plan.fs_out, c->in_frame, c->root_frame);
    if (n_complex != c->root_frame && !c->rs.on && !c->fr.on)
        return fail(c, SDRX_EINVAL, "frame of %d samples, VFOs were initialised for %d (vfo::init samplesPerBuffer)", n_complex,
                    c->root_frame);
    if (sync_call && c->in_flight > 0)
        return fail(c, SDRX_ESTATE, "%s: %d submitted frame(s) not yet delivered -- call sdrx_wait first", what, c->in_flight);
    if (!sync_call && c->in_flight >= SDRX_MAX_IN_FLIGHT)
        return fail(c, SDRX_ESTATE, "%s: %d frames in flight -- call sdrx_wait before submitting another", what, c->in_flight);
    HIPCHK(c, hipSetDevice(c->device));
    return SDRX_OK;
}

// host frame -> the library's pinned staging buffer of this frame parity -> device.  The pinned buffer's
// previous user is frame f-2, which has been delivered (at most two frames are in flight), so its copy is
// long done; the device buffer is written and read on `stream` only, in order.
int stage_host_frame(sdrx_ctx *c, const void *src, size_t bytes, void *dst_dev)
{
    const int p = (int)(c->frame_no & 1ull);
    hipError_t e = c->h_in[0].reserve((size_t)c->in_frame * sizeof(float2)); // both pinned buffers, or none
    if (e == hipSuccess)
        e = c->h_in[1].reserve((size_t)c->in_frame * sizeof(float2));
    if (e != hipSuccess) {
        c->h_in[0].reset();
        c->h_in[1].reset();
        return fail(c, SDRX_EHIP, "no pinned memory for the frame staging: %s", hipGetErrorString(e));
    }
    memcpy(c->h_in[p], src, bytes);
    for (auto &r : c->shared_readers[p]) // whoever shared frame f-2 of this buffer has read it before it is overwritten
        if (r.pending) {
            HIPCHK(c, hipStreamWaitEvent(c->st.stream, r.ev, 0));
            r.pending = false;
        }
    // (the runtime moves host-to-device copies with the DMA engine: concurrent with kernels.  A copy kernel reading the pinned
    // buffer over PCIe instead measured slower, 0.353 vs 0.302 ms per pipelined frame on config 3: it sits in the compute
    // stream's way)
    HIPCHK(c, hipMemcpyAsync(dst_dev, c->h_in[p], bytes, hipMemcpyHostToDevice, c->st.stream));
    HIPCHK(c, hipEventRecord(c->st.ev_staged[p], c->st.stream)); // (for a context that shares this frame: sdrx_submit_shared)
    return SDRX_OK;
}

int enqueue_f32(sdrx_ctx *c, const float *iq, int n_complex, bool egress)
{
    int rc = ensure_raw(c, (size_t)c->in_frame);
    if (rc)
        return rc;
    float2 *dst = c->d_raw[c->frame_no & 1ull];
    rc = stage_host_frame(c, iq, (size_t)n_complex * sizeof(float2), dst);
    if (rc)
        return rc;
    rc = enqueue_frame(c, dst, kRawF32, egress);
    if (rc == SDRX_OK)
        c->last_raw = c->tiled_ingest() ? kRawTiled : kRawF32; // (resampler, front stage: the tree's frame is their output, in the tile layout)
    return rc;
}

// The kernels that read a frame of integer samples (ingest.hip), by format (include/sdrx.h SDRX_FMT_*): one template's instances.
struct SampleKernels {
    void (*ingest)(const unsigned *, float4 *, int);
    void (*products)(const unsigned *, float *, int, int);
    void (*apply)(const unsigned *, const float *, float4 *, int, int);
    void (*block_sums)(const unsigned *, int, const double *, double2 *);
    void (*dc_fast)(const unsigned *, float4 *, int, const float *, float *, const double *, const double2 *);
};
template <int FMT>
SampleKernels sample_kernels_of()
{
    return {k_ingest_samples<FMT>, k_dc_products<FMT>, k_dc_apply<FMT>, k_dc_block_sums<FMT>, k_ingest_dc_fast<FMT>};
}
const SampleKernels &sample_kernels(int fmt)
{
    static const SampleKernels K[3] = {sample_kernels_of<SDRX_FMT_CU8>(), sample_kernels_of<SDRX_FMT_CS8>(), sample_kernels_of<SDRX_FMT_CS16>()};
    return K[fmt];
}
bool known_format(int fmt) { return fmt == SDRX_FMT_CU8 || fmt == SDRX_FMT_CS8 || fmt == SDRX_FMT_CS16 || real_format(fmt); }
size_t sample_bytes(int fmt, int n_complex) { return (size_t)n_complex * (fmt == SDRX_FMT_CS16 ? 4 : 2); } // (real formats: 2 bytes a real sample)

// Option adc_meter: the statistics of the next frame's integer samples as they lie at `dev_samples` (format `fmt`), on the
// context's stream in front of everything that converts them -- one k_adc_meter launch, its record into the frame parity's
// slot, and the host's note that this slot now belongs to that frame.  Called wherever a frame of integer samples enters a
// context: enqueue_samples_device, and the group's dongle bytes without DC removal (group_enqueue).  Not bracketed:
// sdrx_get_kernel_times keeps its SDRX_NKERNELS kinds, and k_ingest stays the conversion.  Option off: nothing.
void adc_meter_launch(sdrx_ctx *c, const void *dev_samples, int n_complex, int fmt)
{
    if (!c->opt_adc_meter)
        return;
    static void (*const K[5])(const unsigned *, int, long long, AdcPartial *, unsigned *, AdcRecord *, int, int) = {
        k_adc_meter<SDRX_FMT_CU8>, k_adc_meter<SDRX_FMT_CS8>, k_adc_meter<SDRX_FMT_CS16>, k_adc_meter<SDRX_FMT_RS16>, k_adc_meter<SDRX_FMT_RU12>};
    const int p = (int)(c->frame_no & 1ull);
    const int nb = (n_complex + kAdcWg - 1) / kAdcWg; // workgroups = partials
    if ((size_t)nb > c->adc.d_part.count()) // (never: every frame has in_frame samples, what adc_setup sized for)
        return;
    const int per = (nb + kAdcThreads - 1) / kAdcThreads, cnt = (nb + per - 1) / per; // the last workgroup's merge: partials per thread, threads
    hipLaunchKernelGGL(K[fmt], dim3(nb), dim3(kAdcThreads), 0, c->st.stream, reinterpret_cast<const unsigned *>(dev_samples), n_complex,
                       (long long)c->frame_no, c->adc.d_part.get(), c->adc.d_count.get(), c->adc.rec.dev<AdcRecord>(p), per, cnt);
    c->adc.note[p].frame = c->frame_no;
    c->adc.note[p].fmt = fmt;
}

// What the DC-bias removal of this context's frames holds on the device, by the first frame that asks for it (nothing once it
// exists: the options and the frame length are fixed): the accumulator, and the fast scan's table or the exact removal's work
// buffer and counters.  All of it or -- the caller resets dc's device part on an error -- none.
int dc_first_use(sdrx_ctx *c, int n_complex, int nchunks)
{
    if (!c->dc.d_state) {
        HIPCHK(c, c->dc.d_state.alloc(4));
        HIPCHK(c, hipMemsetAsync(c->dc.d_state, 0, 4 * sizeof(float), c->st.stream)); // `static cpx_typef avept=0`, sdrj.cpp:279
    }
    if (c->opt_dc_blocked && !c->dc.d_tab) {
        // powers of the decay A = (float)(1 - 1e-6): [0..16] A^k, [32..95] A^(16 l), [96 + k] A^(1024 k)
        const double A = (double)(1.0f - 0.000001f);
        std::vector<double> tab(96 + (size_t)nchunks + 1 + 2 * (size_t)nchunks + 2, 0.0);
        for (int k = 0; k <= 16; ++k)
            tab[(size_t)k] = std::pow(A, k);
        for (int l = 0; l < 64; ++l)
            tab[32 + (size_t)l] = std::pow(A, 16.0 * l);
        for (int k = 0; k <= nchunks; ++k)
            tab[96 + (size_t)k] = std::pow(A, 1024.0 * k);
        c->dc.tab_sums = (96 + (size_t)nchunks + 1 + 1) & ~(size_t)1; // 16-byte aligned double2[]
        HIPCHK(c, c->dc.d_tab.alloc(tab.size()));
        HIPCHK(c, hipMemcpy(c->dc.d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (!c->opt_dc_blocked) {
        const int stride = (int)align_up((size_t)n_complex + kDcPad, 64);
        if (c->dc.work_stride < stride) {
            HIPCHK(c, c->dc.d_work.reserve(4 * (size_t)stride)); // P[2][stride] | A[2][stride]
            HIPCHK(c, hipMemsetAsync(c->dc.d_work, 0, sizeof(float) * 4 * (size_t)stride, c->st.stream));
            c->dc.work_stride = stride;
        }
        if (c->opt_dc_speculative && !c->dc.d_counters) {
            HIPCHK(c, c->dc.d_counters.alloc(4));
            HIPCHK(c, hipMemsetAsync(c->dc.d_counters, 0, 4 * sizeof(unsigned long long), c->st.stream));
        }
    }
    return SDRX_OK;
}

// `dev_bytes`: the frame's integer samples in format `fmt` (dongle bytes, int8 or int16), already on this context's device and
// complete in the order of c->st.stream.  Sample conversion (+ the DC-bias IIR with this context's own accumulator, the one
// accumulator whatever the format) and the frame itself.  Dongle bytes without DC removal go to level 0 as they are (kRawU8);
// the signed formats always enter through an ingest pass into the tile layout, as every DC-corrected frame does.
int enqueue_samples_device(sdrx_ctx *c, const void *dev_bytes, int n_complex, int fmt, int correct_dc, bool egress)
{
    if (real_format(fmt)) {
        // Real samples: the ADC meter reads the same memory as pairs (even samples arm I, odd samples arm Q); stage 1 of the
        // front stage converts the words itself -- no conversion kernel, no DC removal (frame_call_fmt refused it).
        adc_meter_launch(c, dev_bytes, n_complex / 2, fmt);
        {
            Bracket b(c, c->st.stream, KIND_INGEST, 0);
            ingest_chain_launch(c, dev_bytes, fmt);
        }
        const int rc = enqueue_frame(c, dev_bytes, kRawTiled, egress);
        if (rc == SDRX_OK)
            c->last_raw = kRawTiled;
        return rc;
    }
    const SampleKernels &K = sample_kernels(fmt);
    adc_meter_launch(c, dev_bytes, n_complex, fmt); // (option adc_meter: the samples as they arrived, in front of everything)
    int mode = kRawU8;
    const int nchunks = (n_complex + kChunk - 1) / kChunk;
    if (correct_dc)
        if (int rc = dc_first_use(c, n_complex, nchunks)) {
            static_cast<sdrx_ctx::DcDevice &>(c->dc) = sdrx_ctx::DcDevice();
            return rc;
        }
    if (correct_dc && !c->opt_dc_blocked) {
        // products (parallel) -> the two recurrences (one wave each, nearly alone with their dependent chain) -> subtract (parallel)
        float *Pp = c->dc.d_work, *Ap = c->dc.d_work + 2 * (size_t)c->dc.work_stride;
        const int words = n_complex / 2;
        Bracket b(c, c->st.stream, KIND_INGEST, 0);
        hipLaunchKernelGGL(K.products, dim3((words + 255) / 256), dim3(256), 0, c->st.stream, reinterpret_cast<const unsigned *>(dev_bytes), Pp,
                           n_complex, c->dc.work_stride);
        if (c->opt_dc_speculative) {
            // one workgroup per component, dc_waves consecutive 1024-sample blocks per step
            auto chain = c->dc.waves >= 8 ? k_dc_chain_spec<8> : c->dc.waves >= 4 ? k_dc_chain_spec<4> : c->dc.waves >= 2 ? k_dc_chain_spec<2> : k_dc_chain_spec<1>;
            const int waves = c->dc.waves >= 8 ? 8 : c->dc.waves >= 4 ? 4 : c->dc.waves >= 2 ? 2 : 1;
            hipLaunchKernelGGL(chain, dim3(2), dim3(64 * waves), 0, c->st.stream, Pp, Ap, n_complex, c->dc.work_stride, c->dc.d_state, c->dc.d_counters,
                               kDcMaxIter);
        } else {
            hipLaunchKernelGGL(k_dc_chain, dim3(2), dim3(64), 0, c->st.stream, Pp, Ap, n_complex, c->dc.work_stride, c->dc.d_state);
        }
        hipLaunchKernelGGL(K.apply, dim3((words + 255) / 256), dim3(256), 0, c->st.stream, reinterpret_cast<const unsigned *>(dev_bytes), Ap,
                           ingest_dest(c), n_complex, c->dc.work_stride);
        ingest_chain_launch(c);
        mode = kRawTiled;
    } else if (correct_dc) {
        Bracket b(c, c->st.stream, KIND_INGEST, 0);
        const int par = (int)(c->dc.frames++ & 1ull);
        double2 *sums = reinterpret_cast<double2 *>(c->dc.d_tab + c->dc.tab_sums);
        hipLaunchKernelGGL(K.block_sums, dim3(nchunks), dim3(64), 0, c->st.stream, reinterpret_cast<const unsigned *>(dev_bytes), n_complex,
                           c->dc.d_tab, sums);
        hipLaunchKernelGGL(K.dc_fast, dim3(nchunks), dim3(64), 0, c->st.stream, reinterpret_cast<const unsigned *>(dev_bytes),
                           ingest_dest(c), n_complex, c->dc.d_state + 2 * par, c->dc.d_state + 2 * (par ^ 1), c->dc.d_tab, sums);
        ingest_chain_launch(c);
        mode = kRawTiled;
    } else if (fmt != SDRX_FMT_CU8 || c->tiled_ingest()) { // (resampler, front stage, blanker, IQ balance, notch, shift: they read the tile layout, so bytes take the pass too)
        Bracket b(c, c->st.stream, KIND_INGEST, 0);
        const int n_pairs = n_complex / 2;
        hipLaunchKernelGGL(K.ingest, dim3((n_pairs + 255) / 256), dim3(256), 0, c->st.stream, reinterpret_cast<const unsigned *>(dev_bytes),
                           ingest_dest(c), n_pairs);
        ingest_chain_launch(c);
        mode = kRawTiled;
    }
    c->long_frame = correct_dc && !c->opt_dc_blocked;
    const int rc = enqueue_frame(c, dev_bytes, mode, egress);
    c->long_frame = false;
    if (rc == SDRX_OK)
        c->last_raw = mode;
    return rc;
}

// host samples -> this frame parity's device buffer -> enqueue_samples_device.  Dongle bytes land in d_raw_u8 (which
// sdrx_get_raw and sdrx_submit_shared read after a frame without DC removal); the signed formats, up to 4 bytes a sample, in
// the cf32 buffer of that parity, which is twice as large as they need and has no other use in such a frame.
int enqueue_samples(sdrx_ctx *c, const void *samples, int n_complex, int fmt, int correct_dc, bool egress)
{
    int rc = ensure_raw(c, (size_t)c->in_frame);
    if (rc)
        return rc;
    const int p = (int)(c->frame_no & 1ull);
    void *dst = fmt == SDRX_FMT_CU8 ? static_cast<void *>(c->d_raw_u8[p]) : static_cast<void *>(c->d_raw[p]);
    rc = stage_host_frame(c, samples, sample_bytes(fmt, n_complex), dst);
    return rc ? rc : enqueue_samples_device(c, dst, n_complex, fmt, correct_dc, egress);
}

// What the *_fmt calls check on top of check_frame_call / group_check: the format, and for device frames the alignment the
// 16-byte loads of the DC kernels ask for.  nullptr: fine.
const char *bad_samples(int fmt, const void *dev_ptr)
{
    if (!known_format(fmt))
        return "fmt must be SDRX_FMT_CU8 (0), SDRX_FMT_CS8 (1), SDRX_FMT_CS16 (2), or with a real front stage SDRX_FMT_RS16 (3) or SDRX_FMT_RU12 (4)";
    if (dev_ptr && (reinterpret_cast<uintptr_t>(dev_ptr) & 15u))
        return "device samples must be 16-byte aligned";
    return nullptr;
}

} // namespace

extern "C" {

int sdrx_process_device(sdrx_ctx *c, const void *dev_iq, int n_complex)
{
    int rc = check_frame_call(c, "sdrx_process_device", dev_iq, n_complex, true);
    if (rc)
        return rc;
    c->last_raw = c->tiled_ingest() ? kRawTiled : -1; // (resampler, front stage: the tree's frame is the context's own, they wrote it)
    return enqueue_frame(c, dev_iq, kRawF32, false);
}

int sdrx_submit_device(sdrx_ctx *c, const void *dev_iq, int n_complex)
{
    int rc = check_frame_call(c, "sdrx_submit_device", dev_iq, n_complex, false);
    if (rc)
        return rc;
    c->last_raw = c->tiled_ingest() ? kRawTiled : -1;
    return enqueue_frame(c, dev_iq, kRawF32, true);
}

int sdrx_submit(sdrx_ctx *c, const float *iq, int n_complex)
{
    int rc = check_frame_call(c, "sdrx_submit", iq, n_complex, false);
    return rc ? rc : enqueue_f32(c, iq, n_complex, true);
}

// The frame `src` staged LAST (host floats or dongle bytes handed to sdrx_process* / sdrx_submit* of `src`) once
// more, through the tree of `c` -- two contexts on one device fed the same raw frame, as sdrj::demodData feeds
// every main VFO the same `samples` (sdrj.cpp:288-294) -- without a second host-to-device copy: `c` waits for
// src's upload event and reads src's device buffer.  That buffer is per frame parity: it stays untouched until
// `src` stages the frame after next, by which time the caller must have waited for this one on `c`.
// `same_as` (may be null): host cf32 the caller believes to BE that frame -- compared byte for byte with src's pinned staging
// copy first; SDRX_DIFFERENT and nothing queued when it is not.
static int submit_shared(sdrx_ctx *c, sdrx_ctx *src, const char *what, bool sync_call, const float *same_as = nullptr, int same_n = 0)
{
    if (!c || !src || c == src)
        return c ? fail(c, SDRX_EINVAL, "%s: needs another context as the source", what) : SDRX_EINVAL;
    if (c->tiled_ingest() || src->tiled_ingest())
        return fail(c, SDRX_ESTATE, "%s: a context with a resampler, a front stage, a blanker, an IQ balance correction, a spur canceller or a frequency shift (sdrx_set_resampler, "
                                    "sdrx_set_front, sdrx_set_blanker, sdrx_set_iq_balance, sdrx_set_notch, sdrx_set_shift) shares no frames", what);
    if (!src->finalized || src->frame_no == 0 || (src->last_raw != kRawF32 && src->last_raw != kRawU8))
        return fail(c, SDRX_ESTATE, "%s: the source context has staged no host frame (floats or bytes without DC removal) yet", what);
    if (src->device != c->device)
        return fail(c, SDRX_EINVAL, "%s: the source context lives on device %d, this one on %d", what, src->device, c->device);
    const int p = (int)((src->frame_no - 1) & 1ull);
    if (same_as) {
        if (src->last_raw != kRawF32 || same_n != src->root_frame || !src->h_in[p] ||
            memcmp(src->h_in[p], same_as, (size_t)same_n * sizeof(float2)) != 0)
            return SDRX_DIFFERENT;
    }
    const void *frame = src->last_raw == kRawF32 ? (const void *)src->d_raw[p] : (const void *)src->d_raw_u8[p];
    int rc = check_frame_call(c, what, frame, src->root_frame, sync_call);
    if (rc)
        return rc;
    if (src->last_raw == kRawU8 && !c->root_direct)
        return fail(c, SDRX_EUNSUPPORTED, "%s: a wide level 0 (more than 4 parent-less VFOs) shares float frames only", what);
    // src's NEXT upload into this buffer (its frame after next) must not overtake this context's kernels: an event behind
    // them, which src's staging waits for.  One event per (reader, parity), acquired BEFORE anything is queued -- a failure
    // here leaves no frame in flight -- and re-recorded for every shared frame (a source that never restages, or a reader
    // fed through sdrx_process_device, does not pile events up).
    sdrx_ctx::SharedReader *slot = nullptr;
    for (auto &r : src->shared_readers[p])
        if (r.who == c)
            slot = &r;
    if (!slot) {
        hipEvent_t e = nullptr;
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        src->shared_readers[p].push_back({c, e, false});
        slot = &src->shared_readers[p].back();
    }
    HIPCHK(c, hipStreamWaitEvent(c->st.stream, src->st.ev_staged[p], 0));
    c->last_raw = -1; // (not this context's buffer: sdrx_get_raw is served by `src`)
    const int src_raw = src->last_raw;
    rc = enqueue_frame(c, frame, src_raw, true);
    if (rc)
        return rc;
    if (hipEventRecord(slot->ev, c->st.stream) == hipSuccess)
        slot->pending = true;
    else
        (void)hipStreamSynchronize(c->st.stream); // (the frame IS queued: order it the blunt way rather than report a failure)
    return SDRX_OK;
}

int sdrx_submit_shared(sdrx_ctx *c, sdrx_ctx *src) { return submit_shared(c, src, "sdrx_submit_shared", false); }

int sdrx_process_shared(sdrx_ctx *c, sdrx_ctx *src)
{
    const int rc = submit_shared(c, src, "sdrx_process_shared", true);
    return rc ? rc : sdrx_wait(c);
}

int sdrx_submit_if_same(sdrx_ctx *c, sdrx_ctx *src, const float *iq, int n_complex)
{
    if (!iq)
        return c ? fail(c, SDRX_EINVAL, "sdrx_submit_if_same: null frame pointer") : SDRX_EINVAL;
    return submit_shared(c, src, "sdrx_submit_if_same", false, iq, n_complex);
}

int sdrx_process_if_same(sdrx_ctx *c, sdrx_ctx *src, const float *iq, int n_complex)
{
    if (!iq)
        return c ? fail(c, SDRX_EINVAL, "sdrx_process_if_same: null frame pointer") : SDRX_EINVAL;
    const int rc = submit_shared(c, src, "sdrx_process_if_same", true, iq, n_complex);
    return rc ? rc : sdrx_wait(c);
}

int sdrx_in_flight(sdrx_ctx *c) { return c ? c->in_flight : SDRX_EINVAL; }


int sdrx_sync(sdrx_ctx *c)
{
    if (!c)
        return SDRX_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    return drain(c);
}

int sdrx_process(sdrx_ctx *c, const float *iq, int n_complex)
{
    int rc = check_frame_call(c, "sdrx_process", iq, n_complex, true);
    if (rc)
        return rc;
    rc = enqueue_f32(c, iq, n_complex, true);
    return rc ? rc : sdrx_wait(c);
}

// ---- one front door for integer samples (SDRX_FMT_*): host frames, and frames already on the device ------------------------
static int frame_call_fmt(sdrx_ctx *c, const char *what, const void *ptr, int n_complex, int fmt, const void *dev_ptr, bool sync_call, int correct_dc)
{
    const int rc = check_frame_call(c, what, ptr, n_complex, sync_call, known_format(fmt) ? fmt : -1);
    if (rc)
        return rc;
    if (const char *why = bad_samples(fmt, dev_ptr))
        return fail(c, SDRX_EINVAL, "%s: %s", what, why);
    if (real_format(fmt) && correct_dc)
        return fail(c, SDRX_EINVAL, "%s: no DC removal for real samples (DC lands at the edge of the output band, where the stages behind discard it)", what);
    return SDRX_OK;
}

// A host frame through the call `what`: the four entry points below.  The *_u8 calls are the format SDRX_FMT_CU8 under their
// own name: that format passes bad_samples, and a host frame has no alignment to test, so their checks are check_frame_call's.
static int host_samples_call(sdrx_ctx *c, const char *what, const void *ptr, int n_complex, int fmt, int correct_dc, bool sync_call)
{
    int rc = frame_call_fmt(c, what, ptr, n_complex, fmt, nullptr, sync_call, correct_dc);
    if (rc)
        return rc;
    rc = enqueue_samples(c, ptr, n_complex, fmt, correct_dc, true);
    return rc || !sync_call ? rc : sdrx_wait(c);
}

int sdrx_submit_u8(sdrx_ctx *c, const uint8_t *bytes, int n_complex, int correct_dc)
{
    return host_samples_call(c, "sdrx_submit_u8", bytes, n_complex, SDRX_FMT_CU8, correct_dc, false);
}

int sdrx_process_u8(sdrx_ctx *c, const uint8_t *bytes, int n_complex, int correct_dc)
{
    return host_samples_call(c, "sdrx_process_u8", bytes, n_complex, SDRX_FMT_CU8, correct_dc, true);
}

int sdrx_submit_fmt(sdrx_ctx *c, const void *iq, int n_complex, int fmt, int correct_dc)
{
    return host_samples_call(c, "sdrx_submit_fmt", iq, n_complex, fmt, correct_dc, false);
}

int sdrx_process_fmt(sdrx_ctx *c, const void *iq, int n_complex, int fmt, int correct_dc)
{
    return host_samples_call(c, "sdrx_process_fmt", iq, n_complex, fmt, correct_dc, true);
}

// (the samples are the caller's: where the frame went to level 0 as it lies -- dongle bytes without DC removal -- sdrx_get_raw
// and sdrx_submit_shared have no buffer of this context to serve; every other frame left its floats in the tile layout)
static int device_frame_fmt(sdrx_ctx *c, const void *dev_iq, int n_complex, int fmt, int correct_dc, bool egress)
{
    const int rc = enqueue_samples_device(c, dev_iq, n_complex, fmt, correct_dc, egress);
    if (rc == SDRX_OK && c->last_raw == kRawU8)
        c->last_raw = -1;
    return rc;
}

int sdrx_process_device_fmt(sdrx_ctx *c, const void *dev_iq, int n_complex, int fmt, int correct_dc)
{
    const int rc = frame_call_fmt(c, "sdrx_process_device_fmt", dev_iq, n_complex, fmt, dev_iq, true, correct_dc);
    return rc ? rc : device_frame_fmt(c, dev_iq, n_complex, fmt, correct_dc, false);
}

int sdrx_submit_device_fmt(sdrx_ctx *c, const void *dev_iq, int n_complex, int fmt, int correct_dc)
{
    const int rc = frame_call_fmt(c, "sdrx_submit_device_fmt", dev_iq, n_complex, fmt, dev_iq, false, correct_dc);
    return rc ? rc : device_frame_fmt(c, dev_iq, n_complex, fmt, correct_dc, true);
}

} // extern "C"
