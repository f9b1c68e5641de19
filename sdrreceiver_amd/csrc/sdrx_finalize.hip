// sdrx_finalize.hip -- sdrx_finalize: from the list of VFOs to a tree that can run (rates and taps, HBM placement, the work
// lists of every launch, allocation and upload).  A fragment of sdrx.hip's translation unit.
// ================================================================================ sdrx_finalize
// = vfo::init for every node (vfo.cpp:60-176) plus everything the launches need, in phases that hand a `Built` to each
// other: derive_nodes (rates, tap designs, tree levels, which leaves take the fused late decimation) -> plan_buffers (HBM
// placement) -> build_mix_work (the (VFO, time segment) items of the mix/decimate launches) -> build_tail_work (the
// block-per-tile launches of the leaf tail) -> build_level_plan (k_mix_levels' list) -> allocate_and_upload.
namespace {

// A segment that starts inside the frame starts from zero filter state.  An output of stage d with
// index j (counted from the segment's first sample) depends on the inputs 2^d j - 10 (2^d - 1) ... 2^d j,
// so it is exact once j >= 10 - 10 / 2^d: the first ceil(..) outputs of a segment are warm-up and are
// not emitted.  Returned in input samples, rounded up to a multiple of 16 (the emit test of the
// register stages is per lane = per 16 samples); always a multiple of 2^d.
int warmup_samples(int d)
{
    if (d <= 0)
        return 0;
    const int vd = (10 * ((1 << d) - 1) + (1 << d) - 1) >> d;        // ceil(10 (2^d - 1) / 2^d)
    int w = vd << d;
    while (w & 15)
        w += 1 << d;
    return w;
}


struct Built { // host copies of what goes to the arena, and where
    ArenaPlan plan;
    std::map<std::vector<float>, size_t> tap_offsets; // identical tap sets are stored once
    size_t pay = 0;                                   // bytes of the packed payload buffer
    std::vector<std::vector<K1Work>> works;           // mix/decimate items per tree level
    std::vector<int> level_count, level_maxd;
    std::vector<K2aVfo> d2a;
    std::vector<K2Vfo> d2;
    std::vector<K3Vfo> d3;
    std::vector<K4Vfo> d4;
    std::vector<K5Vfo> d5;
    std::vector<K5Post> d5p; // (empty unless some detector leaf has a post-detection filter; then one entry per K5Vfo)
    std::vector<BlockWork> w2a, w2, w3, w4, w5am, w5fm; // (the detector leaves' blocks: one list per kind, one descriptor array)
    std::vector<BlockWork> w5amp, w5fmp;                // (... and of the leaves with a post-detection filter)
    size_t o5p = 0, ow5amp = 0, ow5fmp = 0;
    std::vector<int> n2a, n2, n3, n4, n5; // node index of each descriptor
    size_t o2a = 0, o2 = 0, o3 = 0, o4 = 0, o5 = 0, ow2a = 0, ow2 = 0, ow3 = 0, ow4 = 0, ow5am = 0, ow5fm = 0;
    std::vector<K1Work> all_items; // k_mix_levels: every level's items in one array ...
    std::vector<int> all_item_level, llist; // ... their levels, and the launch list over them
    std::vector<TailWg> tail_wgs;           // k_levels_tail's workgroup list (LevelPlan::tail)
    std::vector<int> mrel4; // option meter: byte offset from the leaf's payload to the record of each k_lpf_long block (w4)
    size_t off_nco_jobs = 0;

    size_t place_taps(const std::vector<float> &t)
    {
        auto it = tap_offsets.find(t);
        if (it != tap_offsets.end())
            return it->second;
        const size_t o = plan.take(t.size() * sizeof(float));
        tap_offsets.emplace(t, o);
        return o;
    }
};

// Does this leaf run its /5 or /6 low-pass inside the mix wave (late_item)?  d = 0 below a parent (a tile-layout input),
// and the tap count the geometry was laid out for -- which is what vfo::init's design formula yields at every rate.
int fused_late_of(const sdrx_ctx *c, const Node &n)
{
    if (!c->opt_fuse_late || !n.leaf || !n.d.demod_usb || n.d.decimate_count != 0 || n.d.parent_id < 0)
        return 0;
    if (n.d.late_decimate == 5 && (int)n.dec.size() == LateGeom<5>::kTaps && n.d.samples_per_buffer >= LateGeom<5>::kChunkLen)
        return 5;
    if (n.d.late_decimate == 6 && (int)n.dec.size() == LateGeom<6>::kTaps && n.d.samples_per_buffer >= LateGeom<6>::kChunkLen)
        return 6;
    return 0;
}

// Does this leaf demodulate inside its mix wave (demod_chunk, demod.hip)?  The reference's 48 kS/s sub VFO: two half-band
// stages below a parent (a tile-layout input, 256 stream samples per 1024-sample chunk), no late decimation, an audio low-pass of
// at most kDmMaxLpf taps (the 10 kHz filter at 48 kS/s has 47).  Everything else keeps k_usb_demod.
bool fused_demod_of(const sdrx_ctx *c, const Node &n)
{
    return c->opt_fuse_demod && n.leaf && n.d.demod_usb && n.d.late_decimate == 0 && n.d.decimate_count == 2 && n.d.parent_id >= 0 &&
           !n.long_lpf && (int)n.lpf.size() <= kDmMaxLpf && n.d.samples_per_buffer >= kChunk;
}
constexpr int kDemodStateFloats = 256; // K2Vfo::state: QO | QE | I | U at 64-float strides

// ---- per-node derived quantities: everything vfo::init computes (vfo.cpp:60-176)
int derive_nodes(sdrx_ctx *c)
{
    const int N = (int)c->nodes.size();
    c->root_frame = 0;
    int max_level = 0;
    for (int i = 0; i < N; ++i) {
        Node &n = c->nodes[(size_t)i];
        const sdrx_vfo_desc &d = n.d;
        n.leaf = n.children.empty();
        {
            char why[200];
            const int rc = sdrx_check_vfo(&d, why, sizeof why); // what a binding may already have asked at init() time
            if (rc != SDRX_OK)
                return fail(c, rc, "vfo %d: %s", i, why);
        }
        if (d.samples_per_buffer % kChunk != 0 && d.samples_per_buffer % kChunk < 256)
            return fail(c, SDRX_EUNSUPPORTED, "vfo %d: samples_per_buffer %d leaves a last chunk shorter than 256 samples", i,
                        d.samples_per_buffer);
        if ((long long)d.samples_per_buffer > (long long)d.fs)
            return fail(c, SDRX_EUNSUPPORTED, "vfo %d: a frame longer than one second of signal is not supported", i);
        n.n_f = d.samples_per_buffer >> d.decimate_count;
        int target = (int)(d.fs / std::pow(2, d.decimate_count)); // vfo.cpp:66
        n.n_out = n.n_f;
        const bool late = d.demod_usb && d.late_decimate > 0; // vfo.cpp:70
        if (late) {
            if (n.n_f % d.late_decimate)
                return fail(c, SDRX_EUNSUPPORTED, "vfo %d: %d samples per frame is not a multiple of late_decimate %d", i, n.n_f,
                            d.late_decimate);
            target /= d.late_decimate;
            n.n_out = n.n_f / d.late_decimate;
            if (!design_low_pass(2, (double)target * d.late_decimate, (double)(target / 2),
                                 (double)target / (d.late_decimate - 1), n.dec)) // vfo.cpp:82-87
                return fail(c, SDRX_EFILTER, "vfo %d: late-decimation low-pass rejected (firfilter.cpp:122-134)", i);
            if ((int)n.dec.size() > kMaxFir)
                return fail(c, SDRX_EUNSUPPORTED, "vfo %d: %zu-tap late-decimation filter exceeds %d", i, n.dec.size(), kMaxFir);
        }
        n.rate = (unsigned)target;
        if (d.demod_usb && d.filter_bw_hz > 0) { // vfo.cpp:106-124
            if (!design_low_pass(2, (double)target, (double)d.filter_bw_hz, (double)d.filter_bw_hz / 4, n.lpf))
                return fail(c, SDRX_EFILTER, "vfo %d: filter_bw %d Hz rejected at %d S/s (firfilter.cpp:122-134)", i, d.filter_bw_hz,
                            target);
            if ((int)n.lpf.size() > kMaxFirLong)
                return fail(c, SDRX_EUNSUPPORTED, "vfo %d: %zu-tap audio filter exceeds %d", i, n.lpf.size(), kMaxFirLong);
            n.long_lpf = (int)n.lpf.size() > kMaxFir;
        }
        if (d.demod_usb) {
            design_hilbert(kHilbert, n.n_out, n.hilbert); // vfo.cpp:137: "Fs" = samplesOut
            n.hnz.clear();
            for (int t = 0; t < kHilbert; ++t) {
                if (t & 1)
                    n.hnz.push_back(n.hilbert[(size_t)t]);
                else if (n.hilbert[(size_t)t] != 0.0f)
                    return fail(c, SDRX_EUNSUPPORTED, "vfo %d: even Hilbert tap %d is not zero", i, t);
            }
            n.hnz_e.assign(96, 0.0f);
            n.hnz_o.assign(96, 0.0f);
            std::copy(n.hnz.begin(), n.hnz.end(), n.hnz_e.begin() + 3);
            std::copy(n.hnz.begin(), n.hnz.end(), n.hnz_o.begin() + 2);
            if (!n.lpf.empty() && !n.long_lpf) {
                n.lpf_pad.assign(n.lpf.size() + 3 + 12, 0.0f);
                std::copy(n.lpf.begin(), n.lpf.end(), n.lpf_pad.begin() + 3);
            }
        }
        nco_rotation((double)d.fs, d.mixer_freq_hz, n.rot_re, n.rot_im);
        if (d.parent_id < 0) {
            n.level = 0;
            if (c->root_frame == 0)
                c->root_frame = d.samples_per_buffer;
            else if (c->root_frame != d.samples_per_buffer)
                return fail(c, SDRX_EINVAL, "vfo %d: all parent-less VFOs must share samples_per_buffer", i);
        } else {
            const Node &p = c->nodes[(size_t)d.parent_id];
            n.level = p.level + 1;
            if (d.samples_per_buffer != p.n_f)
                return fail(c, SDRX_EUNSUPPORTED, "vfo %d: samples_per_buffer %d != parent's output frame %d", i,
                            d.samples_per_buffer, p.n_f);
        }
        if (!n.leaf && d.demod_usb)
            return fail(c, SDRX_EINVAL, "vfo %d has children but demod_usb set", i);
        if (!n.leaf && n.detector)
            return fail(c, SDRX_EINVAL, "vfo %d has children but a detector set (sdrx_set_detector)", i);
        if (!n.post_taps.empty()) {
            if (!n.detector)
                return fail(c, SDRX_EINVAL, "vfo %d carries a post-detection filter (sdrx_set_postfilter) but no detector", i);
            if (n.n_f % n.post_decim)
                return fail(c, SDRX_EUNSUPPORTED, "vfo %d: %d samples per frame is not a multiple of the post-detection decimation %d", i, n.n_f,
                            n.post_decim);
            n.rate = (unsigned)target / (unsigned)n.post_decim;
        }
        max_level = std::max(max_level, n.level);
    }
    c->n_levels = max_level + 1;
    for (Node &n : c->nodes) {
        n.fused_late = fused_late_of(c, n);
        n.fused_demod = fused_demod_of(c, n);
    }
    return SDRX_OK;
}

// ---- where everything lives in the arena; the payload buffer; SURVEY.md 8d's byte count
void plan_buffers(sdrx_ctx *c, Built &B)
{
    const int N = (int)c->nodes.size();
    ArenaPlan &plan = B.plan;
    c->off_k1vfo = plan.take(sizeof(K1Vfo) * (size_t)N);
    c->alg_bytes = 0;
    c->vfo_samples = 0;
    size_t tap_len = 0; // longest decimate[0] a fused leaf would have to keep (sdrx_set_tap)
    for (int i = 0; i < N; ++i) {
        Node &n = c->nodes[(size_t)i];
        const sdrx_vfo_desc &d = n.d;
        const bool late = d.demod_usb && d.late_decimate > 0;
        n.off_cp = plan.take(sizeof(float2) * (size_t)(d.fs / kRun + 1));
        // half-band history -- or, for a fused late decimation, the previous frame's last mixed samples
        const size_t hist = n.fused_late == 5 ? (size_t)late_hist<5>() : n.fused_late == 6 ? (size_t)late_hist<6>() : (size_t)std::max(1, d.decimate_count * kHbHist);
        for (int p = 0; p < 2; ++p)
            n.off_hb[p] = plan.take(sizeof(float2) * hist);
        n.H = n.Hx = 0;
        if (n.leaf && d.demod_usb) {
            const int Hdemod = (int)align_up((size_t)((n.long_lpf ? 0 : n.lpf.size()) + 1 + kHilbert - 1), 4);
            if (late) {
                n.Hx = n.fused_late ? 0 : (int)align_up(n.dec.size(), 4);
                n.H = Hdemod;
            } else {
                n.Hx = Hdemod; // the stream itself feeds the demodulator
            }
        }
        n.has_stream = !(n.fused_late || n.fused_demod) || c->opt_keep_streams;
        if (n.fused_demod)
            for (int p = 0; p < 2; ++p)
                n.off_dstate[p] = plan.take(sizeof(float) * kDemodStateFloats);
        if (n.has_stream)
            for (int p = 0; p < 2; ++p) // a stream that feeds children is kept in whole 1024-sample tiles
                n.off_stream[p] = plan.take(sizeof(float2) * (n.leaf ? (size_t)(n.Hx + n.n_f) : align_up((size_t)n.n_f, kChunk) + kChunk)); // (+1 tile: a shifted walk's idle lanes read past the last one)
        else
            tap_len = std::max(tap_len, (size_t)n.n_f);
        if (late)
            for (int p = 0; p < 2; ++p)
                n.off_z[p] = plan.take(sizeof(float2) * (size_t)(n.H + n.n_out));
        if (!n.lpf_pad.empty())
            n.off_lpf = B.place_taps(n.lpf_pad);
        if (n.long_lpf) {
            n.off_lpf = B.place_taps(n.lpf);
            n.Hu = (int)align_up(n.lpf.size(), 4);
            for (int p = 0; p < 2; ++p)
                n.off_u[p] = plan.take(sizeof(float) * (size_t)(n.Hu + n.n_out));
        }
        if (!n.hnz.empty()) {
            n.off_hnz = B.place_taps(n.hnz);
            n.off_hnz_e = B.place_taps(n.hnz_e);
            n.off_hnz_o = B.place_taps(n.hnz_o);
        }
        if (!n.dec.empty())
            n.off_dec = B.place_taps(n.dec);
        if (!n.hilbert.empty())
            n.off_hilbert = B.place_taps(n.hilbert);
        if (n.leaf) {
            n.pay_off = B.pay;
            if (d.demod_usb)
                n.pay_len = (uint32_t)(n.n_out * 2);
            else if (n.detector)
                n.pay_len = (uint32_t)(2 * detect_out(n)); // n int16: exactly the bytes of the IQ leaf's int8 pairs (n / R with a post-detection filter)
            else
                n.pay_len = (uint32_t)(d.cstyle == 1 ? n.n_f : 2 * n.n_f); // vfo.cpp:143-150
            B.pay = align_up(B.pay + n.pay_len, 64);
            if (c->opt_prequant && d.demod_usb)
                n.off_preq = plan.take(sizeof(float) * (size_t)n.n_out);
            for (int p = 0; p < 2; ++p) { // a detector leaf's state: per frame parity the AM carrier's block partials, the FM z[-1]
                if (n.detector == kDetAm)
                    n.off_part[p] = plan.take(sizeof(unsigned long long) * (size_t)detect_blocks(n.n_f));
                if (n.detector == kDetFm)
                    n.off_zprev[p] = plan.take(sizeof(float2));
                if (!n.post_taps.empty()) // the post-detection filter's history: T - 1 floats (a slot of its own even for T = 1)
                    n.off_post_hist[p] = plan.take(sizeof(float) * std::max<size_t>(n.post_taps.size() - 1, 1));
            }
            if (!n.post_taps.empty())
                n.off_post_taps = B.place_taps(n.post_taps);
        }
        // SURVEY.md 8d algorithmic bytes: cf32 consumed + what this VFO hands on
        c->alg_bytes += 8ll * d.samples_per_buffer + (n.leaf ? (int64_t)n.pay_len : 8ll * n.n_f);
        c->vfo_samples += d.samples_per_buffer;
    }
    c->tap_len = tap_len;
    for (int p = 0; p < 2; ++p)
        c->off_tapbuf[p] = tap_len ? plan.take(sizeof(float2) * tap_len) : 0;
}

int cu_count(const sdrx_ctx *c)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0)
        return prop.multiProcessorCount;
    return 256;
}

// ---- work lists for the mix/decimate launches, one launch per tree level
// A work item is one wave walking a run of chunks of one VFO-frame (+ a warm-up when it starts mid-frame).  Measured on
// config 3 (profiles/README.md): the same NUMBER of segments for every VFO of a level, 32 work items per CU in total, in
// VFO creation order (the long d=5 items of the first parent first, the short d=2 items of the second parent back-filling
// the tail) beats one resident round of equal-length items (86 vs 91.5 us), equal-length short items (94-99 us),
// class-interleaved order (103 us) and segment-major order (96-102 us).
int build_mix_work(sdrx_ctx *c, Built &B)
{
    const int N = (int)c->nodes.size();
    B.works.assign((size_t)c->n_levels, {});
    B.level_count.assign((size_t)c->n_levels, 0);
    B.level_maxd.assign((size_t)c->n_levels, 0);
    for (const Node &n : c->nodes) {
        B.level_count[(size_t)n.level]++;
        B.level_maxd[(size_t)n.level] = std::max(B.level_maxd[(size_t)n.level], n.d.decimate_count);
    }
    const int ncu = cu_count(c);
    std::vector<int> level_nseg((size_t)c->n_levels, 1);
    constexpr int kItemsPerCu = 32;  // work items per CU a level is cut into (= the hardware's wave slots per CU)
    constexpr int kMinSegChunks = 4; // the fewest chunks of useful work a segment of a many-VFO level may have
    constexpr int kLateMinSeg = 4;   // the same for a fused late decimation (measured on config 4, interleaved: 2 / 3 / 4 / 6 / 8
                                     //   chunks per segment = 0.0481 / 0.0484 / 0.0471 / 0.0482 / 0.0509 ms per step)
    for (int lv = 0; lv < c->n_levels; ++lv)
        level_nseg[(size_t)lv] = std::max(1, (ncu * kItemsPerCu + B.level_count[(size_t)lv] - 1) / B.level_count[(size_t)lv]);
    c->mix_chunks = 0;
    for (int i = 0; i < N; ++i) {
        const Node &n = c->nodes[(size_t)i];
        const int n_in = n.d.samples_per_buffer;
        // the walk's chunk and what a segment that starts inside the frame must walk before its first exact output:
        // the half-band cascade's dependency cone, or the decimating low-pass's length (a multiple of 16 L: a segment of a
        // fused late decimation starts on an output AND on a 16-sample run)
        const int chunk = n.fused_late == 5 ? LateGeom<5>::kChunkLen : n.fused_late == 6 ? LateGeom<6>::kChunkLen : kChunk;
        // (a leaf that demodulates in its wave: behind the half-band warm-up another 124 stream samples until the Hilbert window
        // holds real samples and N more until the audio low-pass does -- usb'[m] reads usb[m - N .. m - 1] --, 4 input samples each)
        const int warm_demod = n.fused_demod ? (int)align_up((size_t)(warmup_samples(n.d.decimate_count) + ((kHilbert - 1 + (int)n.lpf.size()) << n.d.decimate_count)), 16) : 0;
        const int warm = n.fused_late == 5 ? LateGeom<5>::kWarm : n.fused_late == 6 ? LateGeom<6>::kWarm : n.fused_demod ? warm_demod : warmup_samples(n.d.decimate_count);
        const int nchunks = (n_in + chunk - 1) / chunk;
        const int wch = (warm + chunk - 1) / chunk; // chunks a segment spends before its first exact output
        // few VFOs in the level (the 2-3 mains): segments as short as the warm-up allows;
        // otherwise at least 4 chunks of useful work per segment
        const bool few = (long long)B.level_count[(size_t)n.level] * nchunks < (long long)ncu * 16;
        const int min_seg = few ? std::max(1, wch) : n.fused_late ? kLateMinSeg : std::max(kMinSegChunks, kMinSegChunks * wch);
        int nseg = c->opt_segments > 0 ? c->opt_segments : std::min(level_nseg[(size_t)n.level], std::max(1, nchunks / min_seg));
        nseg = std::max(1, std::min(nseg, nchunks / std::max(1, wch)));
        // Segment s > 0 starts `warm` samples before its first emitted output and ends on a chunk
        // boundary of ITS OWN walk (s_begin + a whole number of chunks), so the warm-up costs the
        // first `warm / 16` lanes of its first chunk instead of a whole extra chunk; the boundaries
        // between segments are therefore not multiples of 1024.
        // ... unless the whole-chunk warm-up costs little anyway (long VFO-frames cut into few segments:
        // < 4 % extra chunks): then segments stay tile aligned, which keeps the kernel's uniform
        // walk on the tiles (measured on the memory-bound flat workload: a walk that straddles two
        // tiles per chunk costs 5 %).
        const bool shifted = n.fused_late || (long long)(nseg - 1) * wch * 25 > nchunks;
        const int lead = shifted ? warm : wch * chunk; // samples a segment walks before its first emitted output
        const long long target = ((long long)n_in + nseg - 1) / nseg; // samples a segment should emit
        int first_out = 0;                                            // input position of the first output the next segment emits
        while (first_out < n_in) {
            K1Work w;
            w.vfo = i;
            w.s_first_out = first_out;
            w.s_begin = first_out == 0 ? 0 : first_out - lead;
            if (w.s_begin < 0)
                return fail(c, SDRX_EUNSUPPORTED, "vfo %d: %d segments do not leave room for the %d-sample warm-up", i, nseg, warm);
            long long k = ((long long)(first_out - w.s_begin) + target + chunk / 2) / chunk; // chunks of this segment's walk
            k = std::max<long long>(k, lead / chunk + 1);                                   // it must emit something
            long long end = w.s_begin + k * chunk;
            if (end + lead + chunk / 2 >= n_in) // what would be left is not worth a segment of its own
                end = n_in;
            w.s_end = (int)std::min<long long>(n_in, end);
            if (w.s_end == n_in && w.s_begin > 0 && !n.fused_late) {
                // The chunk that holds the frame's last sample saves the filter history for the next
                // frame from the registers of its last TWO lanes and from the tail of the LDS stages:
                // like a tile-aligned frame (checked above), a shifted walk must end in a chunk of
                // at least 256 samples.  Start earlier if it does not -- more warm-up is always exact.
                // (A fused late decimation saves its history from LDS rows that hold the previous chunk's tail
                // as well, and its first chunk is longer than that history: nothing to adjust.)
                const int r = (n_in - w.s_begin) & (kChunk - 1);
                if (r != 0 && r < 256) {
                    const int unit = std::max(16, 1 << n.d.decimate_count);
                    const int delta = (256 - r + unit - 1) / unit * unit;
                    w.s_begin = std::max(0, w.s_begin - delta); // (0 = walk from the frame's start with the real history)
                }
            }
            B.works[(size_t)n.level].push_back(w);
            c->mix_chunks += (w.s_end - w.s_begin + chunk - 1) / chunk;
            first_out = w.s_end;
        }
    }
    // The work items of a launch stay in VFO-major order, i.e. creation order (measured: spreading d=5 and d=2 items evenly
    // through the list is 12 % SLOWER than keeping each VFO's -- and each parent's -- items together).
    c->l1.clear();
    for (int lv = 0; lv < c->n_levels; ++lv) {
        Launch1 L;
        L.kind = lv == 0 ? KIND_MIX_ROOT : KIND_MIX_SUB;
        L.level = lv;
        L.n_work = (int)B.works[(size_t)lv].size();
        bool need_tr = false;
        int lds_late = 0;
        L.alg_bytes = 0;
        for (const Node &n : c->nodes) {
            if (n.level != lv)
                continue;
            need_tr |= n.d.decimate_count == 0 && n.leaf && !n.fused_late;
            lds_late = std::max(lds_late, n.fused_late == 5 ? late_lds_bytes<5>() : n.fused_late == 6 ? late_lds_bytes<6>() : 0);
            lds_late = std::max(lds_late, n.fused_demod ? demod_lds_bytes() : 0);
            // SURVEY.md 8d share of this launch: cf32 consumed (+ cf32 handed to children; + the int16 payload of a leaf that
            // demodulates in its wave)
            L.alg_bytes += 8ll * n.d.samples_per_buffer + (n.leaf ? (n.fused_demod ? (int64_t)n.pay_len : 0ll) : 8ll * n.n_f);
        }
        L.lds_bytes = std::max(k1_lds_bytes(B.level_maxd[(size_t)lv], need_tr), lds_late);
        L.off_work = B.plan.take(sizeof(K1Work) * B.works[(size_t)lv].size());
        c->l1.push_back(L);
    }
    return SDRX_OK;
}

// ---- block-per-tile launches of the leaf tail: one launch per kernel, driven by a (vfo, tile) work list
void build_tail_work(sdrx_ctx *c, Built &B)
{
    const int N = (int)c->nodes.size();
    int64_t b2 = 0, b3 = 0, b5am = 0, b5fm = 0, b5amp = 0, b5fmp = 0;
    int lds2a = 0;
    auto two_kernel_late = [](const Node &n) { return n.leaf && n.d.demod_usb && n.d.late_decimate > 0 && !n.fused_late; };
    // every late-decimating VFO left to a kernel of its own has L in {5,6} and <= 96 taps: one-wave tiles of k_late_decimate4,
    // 2 outputs per lane; anything else goes to the generic k_late_decimate
    bool late4 = true;
    int late_lmax = 5, late_ndec = 0;
    for (const Node &n : c->nodes)
        if (two_kernel_late(n)) {
            late4 = late4 && (n.d.late_decimate == 5 || n.d.late_decimate == 6) && (int)n.dec.size() <= kLateMaxTaps;
            late_lmax = std::max(late_lmax, n.d.late_decimate);
            late_ndec = std::max(late_ndec, (int)n.dec.size());
        }
    c->late4 = late4;
    const int late_tile = late4 ? 64 * kLate4R : 256;
    for (int i = 0; i < N; ++i) {
        Node &n = c->nodes[(size_t)i];
        if (!n.leaf)
            continue;
        if (n.d.demod_usb) {
            if (two_kernel_late(n)) {
                for (int b = 0; b < (n.n_out + late_tile - 1) / late_tile; ++b)
                    B.w2a.push_back({(int)B.d2a.size(), b});
                n.d2a_index = (int)B.d2a.size();
                B.n2a.push_back(i);
                B.d2a.push_back(K2aVfo{});
                lds2a = std::max(lds2a, (int)sizeof(float2) * (n.d.late_decimate * 255 + (int)n.dec.size()));
            }
            {
                // a block computes E = nlpf (rounded up to even) extra usb values as history for its low-pass:
                // its tile is shortened by E so that usb stays ONE pass of <= 1024 values (a second pass would
                // keep two of the four waves busy for a whole Hilbert loop on ~50 values)
                const int nl = n.long_lpf ? 0 : (int)n.lpf.size();
                n.demod_tile = nl > 0 ? ((kDemodTile - (nl + (nl & 1))) & ~3) : kDemodTile;
                // demod_window_rule: a block stages its window [hist | data] entries H + blk tile - E - 124 ... in 16-byte
                // units, sample PAIRS (demod_block).  That entry is even for every blk because the history H and the tile are
                // multiples of 4 and E is even; the stream's base must be a multiple of 16 bytes, and its 8 (H + n) bytes a
                // 32-bit offset.  allocate_and_upload checks all of it on the descriptor it writes.
            }
            // (a leaf that demodulates in its mix wave has a descriptor -- the wave reads it -- but no blocks in this launch)
            for (int b = 0; !n.fused_demod && b < (n.n_out + n.demod_tile - 1) / n.demod_tile; ++b)
                B.w2.push_back({(int)B.d2.size(), b});
            n.d2_index = (int)B.d2.size();
            B.n2.push_back(i);
            B.d2.push_back(K2Vfo{});
            if (!n.fused_demod)
                b2 += n.pay_len; // W_out of SURVEY.md 8d
            if (n.long_lpf) {
                for (int b = 0; b < (n.n_out + 255) / 256; ++b)
                    B.w4.push_back({(int)B.d4.size(), b});
                n.d4_index = (int)B.d4.size();
                B.n4.push_back(i);
                B.d4.push_back(K4Vfo{});
            }
        } else if (n.detector) {
            const bool post = !n.post_taps.empty();
            std::vector<BlockWork> &w = n.detector == kDetAm ? (post ? B.w5amp : B.w5am) : (post ? B.w5fmp : B.w5fm);
            for (int b = 0; b < detect_blocks(n.n_f); ++b)
                w.push_back({(int)B.d5.size(), b});
            n.d5_index = (int)B.d5.size();
            B.n5.push_back(i);
            B.d5.push_back(K5Vfo{});
            (n.detector == kDetAm ? (post ? b5amp : b5am) : (post ? b5fmp : b5fm)) += n.pay_len;
        } else {
            for (int b = 0; b < (n.n_f + 4095) / 4096; ++b)
                B.w3.push_back({(int)B.d3.size(), b});
            n.d3_index = (int)B.d3.size();
            B.n3.push_back(i);
            B.d3.push_back(K3Vfo{});
            b3 += n.pay_len;
        }
    }
    c->lb.clear();
    ArenaPlan &plan = B.plan;
    if (!B.d2a.empty()) {
        B.o2a = plan.take(sizeof(K2aVfo) * B.d2a.size());
        B.ow2a = plan.take(sizeof(BlockWork) * B.w2a.size());
        c->lb.push_back({KIND_LATE_DEC, (int)B.w2a.size(), B.o2a, B.ow2a, c->late4 ? late4_lds_bytes(late_lmax, late_ndec) : lds2a, 0});
    }
    if (!B.d2.empty()) {
        // Blocks are independent and the launch is a few resident rounds deep, so its tail is set by
        // what is dispatched last: longest blocks first (a block with the audio low-pass does about
        // twice the work; the last block of a VFO-frame may be nearly empty).
        auto cost = [&](const BlockWork &b) -> long long {
            const Node &n = c->nodes[(size_t)B.n2[(size_t)b.vfo]];
            const int outs = std::min(n.demod_tile, n.n_out - b.blk * n.demod_tile);
            return (long long)outs * (kHilbertNz + (long long)(n.long_lpf ? 0 : n.lpf.size()));
        };
        std::stable_sort(B.w2.begin(), B.w2.end(), [&](const BlockWork &a, const BlockWork &b) { return cost(a) > cost(b); });
    }
    if (!B.d2.empty()) {
        B.o2 = plan.take(sizeof(K2Vfo) * B.d2.size());
        c->off_k2 = B.o2;
        B.ow2 = plan.take(sizeof(BlockWork) * std::max<size_t>(1, B.w2.size()));
        if (!B.w2.empty()) // (every USB leaf may demodulate in its own mix wave: no k_usb_demod launch at all then)
            c->lb.push_back({KIND_DEMOD, (int)B.w2.size(), B.o2, B.ow2, 0, b2});
    }
    if (!B.d4.empty()) {
        int lds4 = 0;
        for (int i : B.n4)
            lds4 = std::max(lds4, (int)sizeof(float) * ((int)c->nodes[(size_t)i].lpf.size() + 256));
        B.o4 = plan.take(sizeof(K4Vfo) * B.d4.size());
        c->off_k4 = B.o4;
        B.ow4 = plan.take(sizeof(BlockWork) * B.w4.size());
        c->lb.push_back({KIND_LPF_LONG, (int)B.w4.size(), B.o4, B.ow4, lds4, 0});
    }
    if (!B.d3.empty()) {
        B.o3 = plan.take(sizeof(K3Vfo) * B.d3.size());
        B.ow3 = plan.take(sizeof(BlockWork) * B.w3.size());
        c->lb.push_back({KIND_COMPRESS, (int)B.w3.size(), B.o3, B.ow3, 0, b3});
    }
    if (!B.d5.empty()) { // the detector leaves, where k_compress's launch sits: the AM leaves' two passes, then the FM leaves
        B.o5 = plan.take(sizeof(K5Vfo) * B.d5.size());
        c->off_k5 = B.o5;
        if (!B.w5am.empty()) {
            B.ow5am = plan.take(sizeof(BlockWork) * B.w5am.size());
            c->lb.push_back({KIND_DETECT_AM, (int)B.w5am.size(), B.o5, B.ow5am, 0, b5am});
        }
        if (!B.w5fm.empty()) {
            B.ow5fm = plan.take(sizeof(BlockWork) * B.w5fm.size());
            c->lb.push_back({KIND_DETECT_FM, (int)B.w5fm.size(), B.o5, B.ow5fm, 0, b5fm});
        }
        c->off_k5post = 0;
        if (!B.w5amp.empty() || !B.w5fmp.empty()) { // the leaves with a post-detection filter: K5Post beside K5Vfo, lists of their own
            B.d5p.assign(B.d5.size(), K5Post{});
            B.o5p = plan.take(sizeof(K5Post) * B.d5p.size());
            c->off_k5post = B.o5p;
        }
        if (!B.w5amp.empty()) {
            B.ow5amp = plan.take(sizeof(BlockWork) * B.w5amp.size());
            c->lb.push_back({KIND_DETECT_AM_POST, (int)B.w5amp.size(), B.o5, B.ow5amp, 0, b5amp});
        }
        if (!B.w5fmp.empty()) {
            B.ow5fmp = plan.take(sizeof(BlockWork) * B.w5fmp.size());
            c->lb.push_back({KIND_DETECT_FM_POST, (int)B.w5fmp.size(), B.o5, B.ow5fmp, 0, b5fmp});
        }
    }
}

// ---- the one-launch levels (k_mix_levels): unified item array and list
void build_level_plan(sdrx_ctx *c, Built &B)
{
    LevelPlan &P = c->fp;
    P = LevelPlan();
    P.usable = c->n_levels >= 2 && c->n_levels <= kMaxLevels; // (one level: nothing to share a launch with)
    // Frame k passes level l in launch k + l and gets its leaf tail behind launch k + n_levels - 1; the streams are double
    // buffered by frame parity.  A leaf at level l is written in launch k + l and overwritten by frame k + 2 in launch
    // k + l + 2: its tail must have run by then, i.e. l >= n_levels - 2 -- true for every tree the reference builds (two
    // levels).  A deeper tree with a shallower leaf runs one launch per level instead (found by the 600-seed soak run of
    // test_frame_pipeline_on_random_trees: seed 213, a parent-less leaf beside a three-level tree).
    for (const Node &n : c->nodes)
        if (n.leaf && n.level < c->n_levels - 2)
            P.usable = false;
    // Option preroll: the gate of frame g, behind launch g + n_levels - 1, reads the payloads of g - 1 in the parity that g + 1
    // writes.  A leaf that demodulates in its mix wave on level n_levels - 2 writes g + 1's payload in that very launch: only
    // on the last level is its next write behind the gate (the argument above enqueue_frame_as).
    // Option agc needs the same launch order for another reason: the step of frame g, behind the gate of g, writes the gain that
    // g + 1 demodulates with, and such a leaf on level n_levels - 2 demodulates g + 1 in the launch in front of that step.
    for (const Node &n : c->nodes)
        if ((c->opt_preroll || c->opt_agc) && n.fused_demod && n.level != c->n_levels - 1)
            P.usable = false;
    // Option wake: the wake step of a frame, behind the watch of the leaf's source, must sit behind the leaf tail of the frame
    // before and in front of the leaf's own items.  In a step of the software pipeline that order exists only for leaves on the
    // last level (the argument above enqueue_frame): any other tree runs one launch per level.
    for (const Node &n : c->nodes)
        if (c->opt_wake && n.leaf && n.level != c->n_levels - 1)
            P.usable = false;
    if (!P.usable)
        return;
    // deepest level first: in the steady state of the reference's two-level trees the long sub-VFO
    // items are dispatched first and the short level-0 items fill the launch's tail
    P.part_begin.assign((size_t)c->n_levels, 0);
    P.part_end.assign((size_t)c->n_levels, 0);
    P.part_bytes.assign((size_t)c->n_levels, 0);
    for (int q = 0; q < c->n_levels; ++q) {
        const int lv = c->n_levels - 1 - q;
        while (B.llist.size() % 8)
            B.llist.push_back(-1);
        P.part_begin[(size_t)lv] = (int)B.llist.size();
        const int base = (int)B.all_items.size(), cnt = (int)B.works[(size_t)lv].size();
        B.all_items.insert(B.all_items.end(), B.works[(size_t)lv].begin(), B.works[(size_t)lv].end());
        B.all_item_level.insert(B.all_item_level.end(), (size_t)cnt, lv);
        for (int i = 0; i < cnt; ++i)
            B.llist.push_back(base + i);
        P.part_end[(size_t)lv] = (int)B.llist.size();
        P.part_bytes[(size_t)lv] = c->l1[(size_t)lv].alg_bytes;
        P.lds_bytes = std::max(P.lds_bytes, c->l1[(size_t)lv].lds_bytes);
    }
    P.off_items = B.plan.take(sizeof(K1Work) * B.all_items.size());
    P.off_item_level = B.plan.take(sizeof(int) * B.all_item_level.size());
    P.off_list = B.plan.take(sizeof(int) * B.llist.size());

    // Option tail_in_levels: the demodulation of frame k - n_levels inside the launch of frame k (k_levels_tail).  A leaf at
    // level l writes frame f in launch f + l and frame f + 2 -- the same parity buffer -- in launch f + l + 2; the demodulation
    // of f reads it in launch f + n_levels, so l + 2 > n_levels: every leaf that k_usb_demod serves must sit on the last
    // level (the reference's trees: the sub VFOs).  Its history prefix goes to the other parity's buffer, of which the same
    // launch writes only the data part (frame f + 1 on the last level).  A late decimation left to k_late_decimate writes
    // the demodulation's input behind the launch that finished the frame (next writer: frame f + 2, behind launch
    // f + n_levels + 1); compress reads its streams there too, as without the option.  Leaves that demodulate in their mix
    // wave (fuse_demod) have no blocks here.  One-level trees have no k_mix_levels launch to ride in (see above).
    const auto dm_launch = std::find_if(c->lb.begin(), c->lb.end(), [](const LaunchB &L) { return L.kind == KIND_DEMOD; });
    bool tail = c->opt_tail_in_levels && !c->opt_wake && dm_launch != c->lb.end(); // (wake: the demodulation must not ride in the next launch)
    for (const Node &n : c->nodes) {
        if (n.leaf && n.d.demod_usb && !n.fused_demod && n.level != c->n_levels - 1)
            tail = false;
        if (n.fused_demod && c->opt_meter && c->opt_exact == 1) // (k_levels_tail's exact form does not meter mix items: levels.hip)
            tail = false;
        if (n.fused_demod && (c->opt_preroll || c->opt_agc)) // (its payload of f+1 would be written in the launch in front of the gate
            tail = false;                                    //   of f -- and computed with the gain of f: the step of f runs behind it)
    }
    // LDS: four mix waves or one demodulation block per workgroup.  Where four waves' LDS would fit fewer mix waves on a CU
    // than k_mix_levels does (the fused /5 and /6 leaves: 9 KB a wave), the two-launch form stays.
    constexpr int kLdsPerCu = 160 * 1024;
    const int lds_wave = (int)align_up((size_t)P.lds_bytes, 16);
    const int tail_lds = std::max(4 * lds_wave, (int)sizeof(DemodLds));
    if (4 * (kLdsPerCu / tail_lds) < std::min(4 * kK1MinWaves, kLdsPerCu / std::max(1, lds_wave)))
        tail = false;
    // What the fusion buys is fixed per frame (the second launch's ramp and tail, ~6 us); what it costs grows with the
    // demodulation blocks (they run at the mix code's 96 registers, 5 waves per SIMD, instead of k_usb_demod's 7 -- or 9 in the
    // packed arithmetics, which lose more).  Measured: config 4 (13 blocks per CU) gains in every arithmetic,
    // config 3 (31 per CU) gains in the exact one and breaks even in the others, 10 240 subs (310 per CU) loses in all.
    const int dm_per_cu_max = c->opt_exact == 1 ? 64 : 16;
    if ((long long)B.w2.size() > (long long)dm_per_cu_max * cu_count(c))
        tail = false;
    if (!tail)
        return;
    P.tail = true;
    P.lds_wave = lds_wave;
    P.tail_lds = tail_lds;
    P.dm_bytes = dm_launch->alg_bytes;
    P.wg_begin.assign((size_t)c->n_levels, 0);
    P.wg_end.assign((size_t)c->n_levels, 0);
    const TailWg none = {{-1, -1, -1, -1}};
    for (int q = 0; q < c->n_levels; ++q) {
        const int lv = c->n_levels - 1 - q;
        while (B.tail_wgs.size() % 8)
            B.tail_wgs.push_back(none);
        P.wg_begin[(size_t)lv] = (int)B.tail_wgs.size();
        const int b0 = P.part_begin[(size_t)lv], cnt = P.part_end[(size_t)lv] - b0;
        // workgroup 8 b + x of the part takes the items 32 b + 8 w + x (w = its wave): item j on XCD j mod 8, as in k_mix_levels
        for (int blk = 0; 32 * blk < cnt; ++blk)
            for (int x = 0; x < 8; ++x) {
                TailWg g = none;
                for (int w = 0; w < 4; ++w) {
                    const int j = 32 * blk + 8 * w + x;
                    g.item[w] = j < cnt ? B.llist[(size_t)(b0 + j)] : -1;
                }
                B.tail_wgs.push_back(g);
            }
        while ((int)B.tail_wgs.size() > P.wg_begin[(size_t)lv] && B.tail_wgs.back().item[0] < 0) // (no empty workgroups at the end)
            B.tail_wgs.pop_back();
        P.wg_end[(size_t)lv] = (int)B.tail_wgs.size();
    }
    // the demodulation blocks behind the mix items, longest first (build_tail_work sorted them): they fill the mix tail
    while (B.tail_wgs.size() % 8)
        B.tail_wgs.push_back(none);
    P.dm_begin = (int)B.tail_wgs.size();
    for (size_t i = 0; i < B.w2.size(); ++i)
        B.tail_wgs.push_back(TailWg{{-2 - (int)i, -1, -1, -1}});
    P.dm_end = (int)B.tail_wgs.size();
    P.off_wgs = B.plan.take(sizeof(TailWg) * B.tail_wgs.size());
}

// ---- option meter: the record slots behind the payloads, leaf by leaf.  A leaf's records come from exactly one kind of work
// unit: its demodulation blocks (k_usb_demod / k_levels_tail; record = block), its k_lpf_long blocks (long low-pass; record =
// block, placed through a table: K4Vfo has no spare field), its fused-demodulation mix items (fuse_demod) or its k_compress
// blocks (record = block).  A mix item's record is s_first_out >> meter_shift, the shift chosen so that no two items of the
// leaf share one; records no item writes stay zero (d_pay is zeroed at finalize), which the fold ignores.
// byte offset from a leaf's payload to its first record
int meter_rel(const sdrx_ctx *c, const Node &n) { return (int)(c->meter_off + 16 * (size_t)n.meter_first - n.pay_off); }

void build_meter_plan(sdrx_ctx *c, Built &B)
{
    c->meter_off = 0;
    c->meter_slots = 0;
    if (!c->opt_meter)
        return;
    c->meter_off = align_up(B.pay, 16);
    const int N = (int)c->nodes.size();
    for (int i = 0; i < N; ++i) {
        Node &n = c->nodes[(size_t)i];
        n.meter_first = c->meter_slots;
        n.meter_n = 0;
        n.meter_shift = 0;
        if (!n.leaf)
            continue;
        if (n.fused_demod) {
            std::vector<int> fo;
            for (const K1Work &w : B.works[(size_t)n.level])
                if (w.vfo == i)
                    fo.push_back(w.s_first_out);
            std::sort(fo.begin(), fo.end());
            int gap = n.d.samples_per_buffer;
            for (size_t k = 1; k < fo.size(); ++k)
                gap = std::min(gap, fo[k] - fo[k - 1]);
            while (n.meter_shift < 15 && (2 << n.meter_shift) <= gap) // (15: what K2Vfo::meter_rel has room for)
                n.meter_shift++;
            n.meter_n = (fo.back() >> n.meter_shift) + 1;
        } else if (!n.d.demod_usb) { // (k_compress's blocks or a detector's: the same geometry)
            n.meter_n = (n.n_f + 4095) / 4096;
        } else if (n.long_lpf) {
            n.meter_n = (n.n_out + 255) / 256;
        } else {
            n.meter_n = (n.n_out + n.demod_tile - 1) / n.demod_tile;
        }
        c->meter_slots += n.meter_n;
    }
    for (const BlockWork &w : B.w4) {
        const Node &n = c->nodes[(size_t)B.n4[(size_t)w.vfo]];
        B.mrel4.push_back(meter_rel(c, n) + 16 * w.blk);
    }
    for (LaunchB &L : c->lb)
        if (L.kind == KIND_LPF_LONG)
            L.off_mrel = B.plan.take(sizeof(int) * B.mrel4.size());
}

// ---- allocate, zero (= the reference's zero-initialised filter state, dsp.cpp:40-49), fill the descriptors, build the NCO tables
// the tolerance arithmetic's NCO: 1 .. 4 steps of the recurrence as ONE rotation (the stabiliser holds |v|, so a step is the
// rotation by arg(rot) at unit modulus: oscillator.cpp:20-28), in double, stored as floats
void nco_powers(float rot_re, float rot_im, float2 rk[4])
{
    const double ang = std::atan2((double)rot_im, (double)rot_re);
    for (int t = 0; t < 4; ++t)
        rk[t] = make_float2((float)std::cos(ang * (t + 1)), (float)std::sin(ang * (t + 1)));
}

int allocate_and_upload(sdrx_ctx *c, Built &B)
{
    const int N = (int)c->nodes.size();
    B.off_nco_jobs = B.plan.take(sizeof(NcoInit) * (size_t)N);
    c->arena_bytes = align_up(B.plan.size, 256);
    HIPCHK(c, c->arena.alloc(c->arena_bytes));
    HIPCHK(c, hipMemsetAsync(c->arena, 0, c->arena_bytes, c->st.stream));
    // (the copy length stays a multiple of 64 bytes, as the packed payloads are)
    c->pay_bytes = std::max<size_t>(c->opt_meter ? align_up(c->meter_off + 16 * (size_t)c->meter_slots, 64) : B.pay, 64);
    c->agc.rec_off = 0;
    c->agc.n = 0;
    if (c->opt_agc) { // the step's records behind the meter records, one per USB leaf
        for (const Node &n : c->nodes)
            c->agc.n += n.leaf && n.d.demod_usb;
        c->agc.rec_off = align_up(c->meter_off + 16 * (size_t)c->meter_slots, 16);
        c->pay_bytes = align_up(c->agc.rec_off + sizeof(AgcRecord) * (size_t)c->agc.n, 64);
    }
    c->sq.dir_off = c->sq.pack_bytes = c->sq.hpack_off = c->sq.aux_off = 0; // (a finalize that was refused may have left another tree's values)
    if (c->opt_squelch) { // the directory behind the records: one fixed-size copy brings both
        size_t n_leaves = 0;
        for (const Node &n : c->nodes)
            n_leaves += n.leaf;
        c->sq.dir_off = c->pay_bytes;
        c->pay_bytes = align_up(c->sq.dir_off + sizeof(SqHeader) + (c->opt_preroll ? 12 : 8) * n_leaves, 64);
        if (c->opt_squelch_auto) { // thr_eff[n] | floor[n] behind it
            c->sq.aux_off = sq_aux_off(n_leaves, c->opt_preroll != 0);
            c->pay_bytes = align_up(c->sq.dir_off + c->sq.aux_off + 16 * n_leaves, 64);
        }
        c->sq.pack_bytes = std::max<size_t>(align_up(B.pay, 64), 64);
        if (c->opt_preroll) { // every leaf re-opens: two payloads each; on the host behind the fixed part, which they could overrun
            c->sq.pack_bytes *= 2;
            c->sq.hpack_off = c->pay_bytes;
        }
    }
    const size_t h_bytes = align_up(c->pay_bytes, 16) + (c->opt_preroll ? c->sq.pack_bytes : 0);
    for (int p = 0; p < 2; ++p) {
        HIPCHK(c, c->d_pay[p].alloc(align_up(c->pay_bytes, 16))); // (whole 16-byte units)
        HIPCHK(c, hipMemsetAsync(c->d_pay[p], 0, c->pay_bytes, c->st.stream));
        HIPCHK(c, c->h_pay[p].alloc(h_bytes, true));
    }
    {
        const size_t raw_tiles = align_up((size_t)c->root_frame, kChunk) + kChunk; // (+1 tile, as for the parents' streams)
        HIPCHK(c, c->d_raw_tiled.alloc(raw_tiles));
        HIPCHK(c, hipMemsetAsync(c->d_raw_tiled, 0, raw_tiles * sizeof(float2), c->st.stream));
        c->root_direct = B.level_count[0] <= 4; // the reference allows 3 mains (mainwindow.h:82)
    }
    auto P = [&](size_t off) { return c->arena + off; };
    std::vector<K1Vfo> k1((size_t)N);
    std::vector<NcoInit> jobs((size_t)N);
    for (int i = 0; i < N; ++i) {
        Node &n = c->nodes[(size_t)i];
        K1Vfo &k = k1[(size_t)i];
        memset(&k, 0, sizeof k);
        for (int p = 0; p < 2; ++p) {
            if (n.d.parent_id >= 0) {
                const Node &pn = c->nodes[(size_t)n.d.parent_id];
                k.in[p] = reinterpret_cast<const float2 *>(P(pn.off_stream[p])) + pn.Hx;
            } else {
                k.in[p] = c->d_raw_tiled;
            }
            if (n.fused_late) { // the wave writes the decimated stream itself; decimate[0] only where it is kept
                k.out[p] = reinterpret_cast<float2 *>(P(n.off_z[p])) + n.H;
                k.tap[p] = n.has_stream ? reinterpret_cast<float2 *>(P(n.off_stream[p])) : nullptr;
            } else if (n.fused_demod) { // the wave writes the int16 payload itself; decimate[d] only where it is kept
                k.out[p] = nullptr;
                k.tap[p] = n.has_stream ? reinterpret_cast<float2 *>(P(n.off_stream[p])) + n.Hx : nullptr;
            } else {
                k.out[p] = reinterpret_cast<float2 *>(P(n.off_stream[p])) + n.Hx;
            }
            k.hb[p] = reinterpret_cast<float2 *>(P(n.off_hb[p]));
        }
        k.cp = reinterpret_cast<const float2 *>(P(n.off_cp));
        k.rot_re = n.rot_re;
        k.rot_im = n.rot_im;
        nco_powers(n.rot_re, n.rot_im, k.rk);
        k.n_in = n.d.samples_per_buffer;
        k.d = n.d.decimate_count;
        k.L = n.d.fs;
        k.out_tiled = n.leaf ? 0 : 1;
        k.late_L = n.fused_late;
        k.late_taps = n.fused_late ? reinterpret_cast<const float *>(P(n.off_dec)) : nullptr;
        k.dm = n.fused_demod ? reinterpret_cast<const K2Vfo *>(P(B.o2)) + n.d2_index : nullptr;
        jobs[(size_t)i] = NcoInit{reinterpret_cast<float2 *>(P(n.off_cp)), n.rot_re, n.rot_im, n.d.fs, 0};
    }
    for (size_t q = 0; q < B.d2a.size(); ++q) {
        Node &n = c->nodes[(size_t)B.n2a[q]];
        K2aVfo &k = B.d2a[q];
        for (int p = 0; p < 2; ++p) {
            k.x[p] = reinterpret_cast<const float2 *>(P(n.off_stream[p]));
            k.x_next[p] = reinterpret_cast<float2 *>(P(n.off_stream[p ^ 1]));
            k.z[p] = reinterpret_cast<float2 *>(P(n.off_z[p])) + n.H;
        }
        k.taps = reinterpret_cast<const float *>(P(n.off_dec));
        k.Hx = n.Hx;
        k.n = n.n_f;
        k.ndec = (int)n.dec.size();
        k.L = n.d.late_decimate;
        k.n_out = n.n_out;
    }
    for (size_t q = 0; q < B.d2.size(); ++q) {
        Node &n = c->nodes[(size_t)B.n2[q]];
        K2Vfo &k = B.d2[q];
        const bool late = n.d.late_decimate > 0;
        for (int p = 0; p < 2; ++p) {
            k.s[p] = n.fused_demod ? nullptr : reinterpret_cast<const float2 *>(P(late ? n.off_z[p] : n.off_stream[p]));
            k.s_next[p] = n.fused_demod ? nullptr : reinterpret_cast<float2 *>(P(late ? n.off_z[p ^ 1] : n.off_stream[p ^ 1]));
        }
        k.hnz = reinterpret_cast<const float *>(P(n.off_hnz));
        k.hnz_e = reinterpret_cast<const float *>(P(n.off_hnz_e));
        k.hnz_o = reinterpret_cast<const float *>(P(n.off_hnz_o));
        k.lpf_pad = (n.lpf.empty() || n.long_lpf) ? nullptr : reinterpret_cast<const float *>(P(n.off_lpf));
        for (int p = 0; p < 2; ++p) {
            k.usb_out[p] = n.long_lpf ? reinterpret_cast<float *>(P(n.off_u[p])) + n.Hu : nullptr;
            k.state[p] = n.fused_demod ? reinterpret_cast<float *>(P(n.off_dstate[p])) : nullptr;
        }
        for (int p = 0; p < 2; ++p)
            k.pay[p] = reinterpret_cast<short *>(c->d_pay[p] + n.pay_off);
        k.prequant = (c->opt_prequant) ? reinterpret_cast<float *>(P(n.off_preq)) : nullptr;
        k.gain = n.d.gain;
        k.H = late ? n.H : n.Hx;
        k.n = n.n_out;
        k.nlpf = n.long_lpf ? 0 : (int)n.lpf.size();
        k.tile = n.demod_tile;
        if (!n.fused_demod) { // demod_window_rule (build_tail_work)
            if ((k.H | k.tile) & 1)
                return fail(c, SDRX_EUNSUPPORTED, "vfo %d: demodulation history %d or tile %d is odd", B.n2[q], k.H, k.tile);
            for (int p = 0; p < 2; ++p)
                if (reinterpret_cast<uintptr_t>(k.s[p]) % 16)
                    return fail(c, SDRX_EUNSUPPORTED, "vfo %d: demodulation stream %d is not 16-byte aligned", B.n2[q], p);
            if ((long long)k.H + k.n >= (1ll << 28))
                return fail(c, SDRX_EUNSUPPORTED, "vfo %d: demodulation stream of %d samples exceeds a 32-bit byte offset", B.n2[q], k.n);
        }
        k.meter_rel = c->opt_meter ? meter_rel(c, n) | n.meter_shift : 0;
    }
    for (size_t q = 0; q < B.d4.size(); ++q) {
        Node &n = c->nodes[(size_t)B.n4[q]];
        K4Vfo &k = B.d4[q];
        for (int p = 0; p < 2; ++p) {
            k.u[p] = reinterpret_cast<const float *>(P(n.off_u[p]));
            k.u_next[p] = reinterpret_cast<float *>(P(n.off_u[p ^ 1]));
            k.pay[p] = reinterpret_cast<short *>(c->d_pay[p] + n.pay_off);
        }
        k.taps = reinterpret_cast<const float *>(P(n.off_lpf));
        k.prequant = (c->opt_prequant) ? reinterpret_cast<float *>(P(n.off_preq)) : nullptr;
        k.gain = n.d.gain;
        k.Hu = n.Hu;
        k.n = n.n_out;
        k.nlpf = (int)n.lpf.size();
    }
    for (size_t q = 0; q < B.d3.size(); ++q) {
        Node &n = c->nodes[(size_t)B.n3[q]];
        K3Vfo &k = B.d3[q];
        for (int p = 0; p < 2; ++p) {
            k.s[p] = reinterpret_cast<const float2 *>(P(n.off_stream[p])) + n.Hx;
            k.pay[p] = reinterpret_cast<signed char *>(c->d_pay[p] + n.pay_off);
        }
        k.n = n.n_f;
        k.cstyle = n.d.cstyle;
        k.scalecomp = n.d.scalecomp;
        k.meter_rel = c->opt_meter ? meter_rel(c, n) : 0;
    }
    for (size_t q = 0; q < B.d5.size(); ++q) {
        Node &n = c->nodes[(size_t)B.n5[q]];
        K5Vfo &k = B.d5[q];
        memset(&k, 0, sizeof k);
        for (int p = 0; p < 2; ++p) {
            k.s[p] = reinterpret_cast<const float2 *>(P(n.off_stream[p])) + n.Hx;
            k.pay[p] = reinterpret_cast<short *>(c->d_pay[p] + n.pay_off);
            k.part[p] = n.detector == kDetAm ? reinterpret_cast<unsigned long long *>(P(n.off_part[p])) : nullptr;
            k.zprev[p] = n.detector == kDetFm ? reinterpret_cast<float2 *>(P(n.off_zprev[p])) : nullptr;
            if (reinterpret_cast<uintptr_t>(k.s[p]) % 16) // (k_detect loads sample pairs)
                return fail(c, SDRX_EUNSUPPORTED, "vfo %d: detector stream %d is not 16-byte aligned", B.n5[q], p);
        }
        k.gain = n.d.gain;
        k.n = n.n_f;
        k.kind = n.detector;
        k.meter_rel = c->opt_meter ? meter_rel(c, n) : 0;
        if (!n.post_taps.empty()) {
            K5Post &kp = B.d5p[q];
            kp.taps = reinterpret_cast<const float *>(P(n.off_post_taps));
            for (int p = 0; p < 2; ++p)
                kp.hist[p] = reinterpret_cast<float *>(P(n.off_post_hist[p]));
            kp.ntaps = (int)n.post_taps.size();
            kp.decim = n.post_decim;
        }
    }
    auto up = [&](size_t off, const void *src, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(P(off), src, bytes, hipMemcpyHostToDevice, c->st.stream) : hipSuccess;
    };
    HIPCHK(c, up(c->off_k1vfo, k1.data(), sizeof(K1Vfo) * k1.size()));
    HIPCHK(c, up(B.off_nco_jobs, jobs.data(), sizeof(NcoInit) * jobs.size()));
    for (int lv = 0; lv < c->n_levels; ++lv)
        HIPCHK(c, up(c->l1[(size_t)lv].off_work, B.works[(size_t)lv].data(), sizeof(K1Work) * B.works[(size_t)lv].size()));
    HIPCHK(c, up(B.o2a, B.d2a.data(), sizeof(K2aVfo) * B.d2a.size()));
    HIPCHK(c, up(B.ow2a, B.w2a.data(), sizeof(BlockWork) * B.w2a.size()));
    HIPCHK(c, up(B.o2, B.d2.data(), sizeof(K2Vfo) * B.d2.size()));
    HIPCHK(c, up(B.ow2, B.w2.data(), sizeof(BlockWork) * B.w2.size()));
    HIPCHK(c, up(B.o4, B.d4.data(), sizeof(K4Vfo) * B.d4.size()));
    HIPCHK(c, up(B.ow4, B.w4.data(), sizeof(BlockWork) * B.w4.size()));
    HIPCHK(c, up(B.o3, B.d3.data(), sizeof(K3Vfo) * B.d3.size()));
    HIPCHK(c, up(B.ow3, B.w3.data(), sizeof(BlockWork) * B.w3.size()));
    HIPCHK(c, up(B.o5, B.d5.data(), sizeof(K5Vfo) * B.d5.size()));
    HIPCHK(c, up(B.ow5am, B.w5am.data(), sizeof(BlockWork) * B.w5am.size()));
    HIPCHK(c, up(B.ow5fm, B.w5fm.data(), sizeof(BlockWork) * B.w5fm.size()));
    HIPCHK(c, up(B.o5p, B.d5p.data(), sizeof(K5Post) * B.d5p.size()));
    HIPCHK(c, up(B.ow5amp, B.w5amp.data(), sizeof(BlockWork) * B.w5amp.size()));
    HIPCHK(c, up(B.ow5fmp, B.w5fmp.data(), sizeof(BlockWork) * B.w5fmp.size()));
    if (c->fp.usable) {
        HIPCHK(c, up(c->fp.off_items, B.all_items.data(), sizeof(K1Work) * B.all_items.size()));
        HIPCHK(c, up(c->fp.off_item_level, B.all_item_level.data(), sizeof(int) * B.all_item_level.size()));
        HIPCHK(c, up(c->fp.off_list, B.llist.data(), sizeof(int) * B.llist.size()));
        if (c->fp.tail)
            HIPCHK(c, up(c->fp.off_wgs, B.tail_wgs.data(), sizeof(TailWg) * B.tail_wgs.size()));
    }
    for (auto &kv : B.tap_offsets)
        HIPCHK(c, up(kv.second, kv.first.data(), kv.first.size() * sizeof(float)));
    for (const LaunchB &L : c->lb)
        if (c->opt_meter && L.kind == KIND_LPF_LONG)
            HIPCHK(c, up(L.off_mrel, B.mrel4.data(), sizeof(int) * B.mrel4.size()));
    HIPCHK(c, hipStreamSynchronize(c->st.stream)); // the host vectors above go out of scope

    // NCO tables: Oscillator::Oscillator for every node, on the device
    hipLaunchKernelGGL(k_nco_init, dim3((N + 63) / 64), dim3(64), 0, c->st.stream, reinterpret_cast<const NcoInit *>(P(B.off_nco_jobs)), N);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->st.stream));
    return SDRX_OK;
}

// ---- publish order: main VFOs in list order, their subs in list order (vfo.cpp:257-263)
void build_publish_order(sdrx_ctx *c)
{
    c->publish_order.clear();
    std::vector<int> stack;
    for (int i = (int)c->nodes.size() - 1; i >= 0; --i)
        if (c->nodes[(size_t)i].d.parent_id < 0)
            stack.push_back(i);
    while (!stack.empty()) {
        const int i = stack.back();
        stack.pop_back();
        const Node &n = c->nodes[(size_t)i];
        if (n.leaf)
            c->publish_order.push_back(i);
        else
            for (auto it = n.children.rbegin(); it != n.children.rend(); ++it)
                stack.push_back(*it);
    }
}

// ---- option squelch: the per-leaf descriptors in publish order, thresholds 0 (always open), hang_left 0, the packed buffers
int squelch_setup(sdrx_ctx *c)
{
    if (!c->opt_squelch)
        return SDRX_OK;
    const size_t n = c->publish_order.size();
    if (n > (size_t)kSqMaxLeaves)
        return fail(c, SDRX_EUNSUPPORTED, "option squelch: %zu leaves, the gate handles %d", n, kSqMaxLeaves);
    c->sq.index.assign(c->nodes.size(), -1);
    std::vector<SqLeaf> leaves(n);
    size_t longest = 0;
    for (size_t k = 0; k < n; ++k) {
        const Node &nd = c->nodes[(size_t)c->publish_order[k]];
        c->sq.index[(size_t)c->publish_order[k]] = (int)k;
        SqLeaf &L = leaves[k];
        L.pay_off = (unsigned)nd.pay_off;
        L.pay_units = (unsigned)(align_up(nd.pay_len, 64) / 64);
        L.meter_off = (unsigned)(c->meter_off + 16 * (size_t)nd.meter_first);
        L.meter_n = (unsigned)nd.meter_n;
        longest = std::max(longest, align_up(nd.pay_len, 64));
    }
    c->sq.tiles = (int)std::max<size_t>((longest + kSqTile - 1) / kSqTile, 1);
    c->sq.cfg.assign(n, SqCfg{0, 0, 0});
    c->sq.offs.assign(n, 0);
    c->sq.hang.assign(n, 0);
    c->sq.pre.assign(n, 0);
    c->sq.units.resize(n);
    for (size_t k = 0; k < n; ++k)
        c->sq.units[k] = leaves[k].pay_units;
    const size_t n1 = std::max<size_t>(n, 1);
    HIPCHK(c, c->sq.d_leaves.alloc(n1));
    HIPCHK(c, c->sq.d_cfg.alloc(n1));
    HIPCHK(c, c->sq.d_hang.alloc(n1));
    if (c->opt_preroll) { // prev_open = 1: frame 0 has no predecessor
        HIPCHK(c, c->sq.d_prev.alloc(n1));
        HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->sq.d_prev.get()), 1, n1, c->st.stream));
    }
    std::vector<SqAuto> fresh; // (lives until the synchronisation below)
    if (c->opt_squelch_auto) { // no observation, ratio 0: the plain gate until sdrx_set_squelch_auto
        c->sq.acfg.assign(n, SqAutoJob{0, 0, 0, 0});
        c->sq.thr_eff.assign(n, 0);
        c->sq.floor.assign(n, kSqNone);
        fresh.assign(n1, SqAuto{kSqNone, kSqNone, 0, 0, 0, 0});
        HIPCHK(c, c->sq.d_auto.alloc(n1));
        HIPCHK(c, hipMemcpyAsync(c->sq.d_auto, fresh.data(), sizeof(SqAuto) * n1, hipMemcpyHostToDevice, c->st.stream));
    }
    HIPCHK(c, hipMemcpyAsync(c->sq.d_leaves, leaves.data(), sizeof(SqLeaf) * n, hipMemcpyHostToDevice, c->st.stream));
    HIPCHK(c, hipMemsetAsync(c->sq.d_cfg, 0, sizeof(SqCfg) * n1, c->st.stream));
    HIPCHK(c, hipMemsetAsync(c->sq.d_hang, 0, sizeof(unsigned) * n1, c->st.stream));
    for (int p = 0; p < 2; ++p) {
        HIPCHK(c, c->sq.d_pack[p].alloc(c->sq.pack_bytes));
        HIPCHK(c, hipMemsetAsync(c->sq.d_pack[p], 0, c->sq.pack_bytes, c->st.stream));
        if (!c->sq.ev_dir[p])
            HIPCHK(c, hipEventCreateWithFlags(&c->sq.ev_dir[p], hipEventDisableTiming));
    }
    HIPCHK(c, hipStreamSynchronize(c->st.stream)); // (`leaves` lives on this stack)
    return SDRX_OK;
}

// ---- option park: the flag words, all 1 (every leaf active, as the reference's VFOs are after vfo::init)
int park_setup(sdrx_ctx *c, const Built &B)
{
    c->park = sdrx_ctx::Park();
    if (!c->opt_park)
        return SDRX_OK;
    sdrx_ctx::Park &K = c->park;
    K.o_2a = c->nodes.size();
    K.o_2 = K.o_2a + B.d2a.size();
    K.o_3 = K.o_2 + B.d2.size();
    K.o_4 = K.o_3 + B.d3.size();
    K.o_5 = K.o_4 + B.d4.size();
    K.o_sq = K.o_5 + B.d5.size();
    K.words = K.o_sq + c->publish_order.size();
    K.leaf.assign(c->nodes.size(), sdrx_ctx::Park::Leaf());
    K.items.assign(c->nodes.size(), {});
    if (c->fp.usable)
        for (size_t it = 0; it < B.all_items.size(); ++it)
            K.items[(size_t)B.all_items[it].vfo].push_back((int)it);
    HIPCHK(c, K.d_act.alloc(K.words));
    HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(K.d_act.get()), 1, K.words, c->st.stream));
    HIPCHK(c, hipStreamSynchronize(c->st.stream));
    return SDRX_OK;
}

// ---- option agc: the per-leaf table in node order, settings all zero (off), quiet_run 0
int agc_setup(sdrx_ctx *c)
{
    const size_t rec_off = c->agc.rec_off;
    const int n_slots = c->agc.n;
    c->agc = sdrx_ctx::Agc();
    if (!c->opt_agc)
        return SDRX_OK;
    sdrx_ctx::Agc &A = c->agc;
    A.rec_off = rec_off;
    A.n = n_slots;
    A.slot.assign(c->nodes.size(), -1);
    sdrx_agc_cfg off;
    memset(&off, 0, sizeof off);
    A.cfg.assign(c->nodes.size(), off);
    std::vector<AgcLeaf> leaves;
    for (size_t i = 0; i < c->nodes.size(); ++i) {
        const Node &nd = c->nodes[i];
        if (!nd.leaf || !nd.d.demod_usb)
            continue;
        A.slot[i] = (int)leaves.size();
        AgcLeaf L;
        memset(&L, 0, sizeof L);
        L.gain = nd.d4_index >= 0 ? &(reinterpret_cast<K4Vfo *>(c->arena + c->off_k4) + nd.d4_index)->gain
                                  : &(reinterpret_cast<K2Vfo *>(c->arena + c->off_k2) + nd.d2_index)->gain;
        L.meter_off = (unsigned)(c->meter_off + 16 * (size_t)nd.meter_first);
        L.meter_n = (unsigned)nd.meter_n;
        L.n_values = (unsigned)nd.n_out;
        L.act_word = c->opt_park ? (unsigned)(c->park.o_2 + (size_t)nd.d2_index) : 0u;
        leaves.push_back(L);
    }
    const size_t n1 = std::max<size_t>(leaves.size(), 1);
    HIPCHK(c, A.d_leaves.alloc(n1));
    HIPCHK(c, A.d_cfg.alloc(n1));
    HIPCHK(c, A.d_quiet.alloc(n1));
    HIPCHK(c, hipMemcpyAsync(A.d_leaves, leaves.data(), sizeof(AgcLeaf) * leaves.size(), hipMemcpyHostToDevice, c->st.stream));
    HIPCHK(c, hipMemsetAsync(A.d_cfg, 0, sizeof(AgcCfg) * n1, c->st.stream));
    HIPCHK(c, hipMemsetAsync(A.d_quiet, 0, sizeof(unsigned) * n1, c->st.stream));
    HIPCHK(c, hipStreamSynchronize(c->st.stream)); // (`leaves` lives on this stack)
    return SDRX_OK;
}

// ---- option catchup: every leaf's own entries of the work lists, kept on the host (sdrx_set_active cuts its sub-lists from them)
void catchup_setup(sdrx_ctx *c, const Built &B)
{
    c->cu = sdrx_ctx::Catchup();
    if (!c->opt_catchup)
        return;
    c->cu.leaf.assign(c->nodes.size(), sdrx_ctx::Catchup::Leaf());
    for (const std::vector<K1Work> &level : B.works)
        for (const K1Work &w : level)
            if (c->nodes[(size_t)w.vfo].leaf)
                c->cu.leaf[(size_t)w.vfo].mix.push_back(w);
    for (const BlockWork &w : B.w2a)
        c->cu.leaf[(size_t)B.n2a[(size_t)w.vfo]].blk[0].push_back(w);
    for (const BlockWork &w : B.w2)
        c->cu.leaf[(size_t)B.n2[(size_t)w.vfo]].blk[1].push_back(w);
    for (size_t k = 0; k < B.w4.size(); ++k) {
        sdrx_ctx::Catchup::Leaf &L = c->cu.leaf[(size_t)B.n4[(size_t)B.w4[k].vfo]];
        L.blk[2].push_back(B.w4[k]);
        if (c->opt_meter)
            L.mrel.push_back(B.mrel4[k]);
    }
    for (const BlockWork &w : B.w3)
        c->cu.leaf[(size_t)B.n3[(size_t)w.vfo]].blk[3].push_back(w);
    for (const BlockWork &w : B.w5am)
        c->cu.leaf[(size_t)B.n5[(size_t)w.vfo]].blk[4].push_back(w);
    for (const BlockWork &w : B.w5fm)
        c->cu.leaf[(size_t)B.n5[(size_t)w.vfo]].blk[5].push_back(w);
    for (const BlockWork &w : B.w5amp)
        c->cu.leaf[(size_t)B.n5[(size_t)w.vfo]].blk[6].push_back(w);
    for (const BlockWork &w : B.w5fmp)
        c->cu.leaf[(size_t)B.n5[(size_t)w.vfo]].blk[7].push_back(w);
}

// Option adc_meter: what k_adc_meter needs for this context's frames -- one partial per workgroup of a frame, the launch's
// counter, and the record buffers of both frame parities with their pinned copies.  All of it or (the caller releases) none.
int adc_setup(sdrx_ctx *c)
{
    if (!c->opt_adc_meter)
        return SDRX_OK;
    const size_t nb = ((size_t)c->in_frame + kAdcWg - 1) / kAdcWg; // (the frame as it arrives: at the input rate with a resampler)
    if (c->adc.d_part.alloc(nb) != hipSuccess || c->adc.d_count.alloc(1, true) != hipSuccess || c->adc.rec.alloc(sizeof(AdcRecord)) != hipSuccess)
        return fail(c, SDRX_ENOMEM, "sdrx_finalize: no memory for the ADC meter (option \"adc_meter\")");
    return SDRX_OK;
}

// Resampler: the frame lengths of the ratio sdrx_set_resampler fixed, for the tree as it now stands (c->in_frame: what a frame
// call takes), or why this tree cannot have it.  Off: in_frame = root_frame.
int resample_plan_frames(sdrx_ctx *c)
{
    c->in_frame = c->root_frame;
    if (!c->rs.on)
        return SDRX_OK;
    if (!c->rs.refused.empty())
        return fail(c, SDRX_EUNSUPPORTED, "resampler %d -> %d S/s: %s", c->rs.plan.fs_in, c->rs.plan.fs_out, c->rs.refused.c_str());
    for (const Node &n : c->nodes)
        if (n.d.parent_id < 0 && n.d.fs != c->rs.plan.fs_out)
            return fail(c, SDRX_EUNSUPPORTED, "resampler: the parent-less VFOs must share one fs (%d and %d; sdrx_set_resampler took the first)",
                        c->rs.plan.fs_out, n.d.fs);
    if (const char *why = resample_frames(c->rs.plan, c->root_frame))
        return fail(c, SDRX_EUNSUPPORTED, "resampler %d -> %d S/s (L = %d, M = %d) with frames of %d: %s", c->rs.plan.fs_in, c->rs.plan.fs_out,
                    c->rs.plan.L, c->rs.plan.M, c->root_frame, why);
    c->in_frame = c->rs.plan.n_in;
    return SDRX_OK;
}

// ... and what k_resample needs on the device: the staging frame, the zeroed history, the taps phase-major g[ph][t] = h[ph + t L].
// All of it or (the caller releases) none.
int resample_setup(sdrx_ctx *c)
{
    if (!c->rs.on)
        return SDRX_OK;
    const ResamplePlan &P = c->rs.plan;
    const size_t stage = align_up((size_t)P.n_in, kChunk) + kChunk;
    if (c->rs.d_stage.alloc(stage) != hipSuccess || c->rs.d_hist.alloc(2 * (size_t)kRsHist) != hipSuccess ||
        c->rs.d_taps.alloc((size_t)P.L * P.T) != hipSuccess)
        return fail(c, SDRX_ENOMEM, "sdrx_finalize: no device memory for the resampler");
    HIPCHK(c, hipMemsetAsync(c->rs.d_stage, 0, stage * sizeof(float2), c->st.stream));
    HIPCHK(c, hipMemsetAsync(c->rs.d_hist, 0, 2 * (size_t)kRsHist * sizeof(float2), c->st.stream));
    std::vector<float> g((size_t)P.L * P.T);
    for (int ph = 0; ph < P.L; ++ph)
        for (int t = 0; t < P.T; ++t)
            g[(size_t)ph * P.T + t] = c->rs.taps[(size_t)ph + (size_t)t * P.L];
    HIPCHK(c, hipMemcpy(c->rs.d_taps, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice));
    c->rs.lds_bytes = resample_lds_bytes(resample_max_window(P));
    return SDRX_OK;
}

// Front stage: the frame lengths of the stages sdrx_set_front fixed in front of what the tree (or the resampler) takes -- c->in_frame
// grows by 2^stages --, or why this tree cannot have it.  Off: nothing.
int front_plan_frames(sdrx_ctx *c)
{
    if (!c->fr.on)
        return SDRX_OK;
    const Node *first = nullptr;
    for (const Node &n : c->nodes) {
        if (n.d.parent_id >= 0)
            continue;
        if (!first)
            first = &n;
        else if (n.d.fs != first->d.fs || n.d.samples_per_buffer != first->d.samples_per_buffer)
            return fail(c, SDRX_EUNSUPPORTED, "front stage: the parent-less VFOs must share one fs and one frame (%d S/s with %d samples, and %d S/s with %d)",
                        first->d.fs, first->d.samples_per_buffer, n.d.fs, n.d.samples_per_buffer);
    }
    if (const char *why = front_frames(c->fr.plan, c->in_frame))
        return fail(c, SDRX_EUNSUPPORTED, "front stage of %d half-band(s) in front of frames of %d: %s", c->fr.plan.stages, c->in_frame, why);
    c->in_frame = c->fr.plan.in_frame;
    return SDRX_OK;
}

// ... and what k_front_halfband needs on the device: the cf32 input frame of every complex stage (whole tiles plus one), the
// zeroed histories, the non-zero taps as the kernel reads them: h[0], h[2], .. h[4K+2], then h[C].  All of it or (the caller
// releases) none.
int front_setup(sdrx_ctx *c)
{
    if (!c->fr.on)
        return SDRX_OK;
    const FrontPlan &P = c->fr.plan;
    for (int s = P.real ? 2 : 1; s <= P.stages; ++s) {
        const size_t n = align_up((size_t)front_stage_in(P, s), kChunk) + kChunk;
        if (c->fr.d_in[s - 1].alloc(n) != hipSuccess)
            return fail(c, SDRX_ENOMEM, "sdrx_finalize: no device memory for the front stage");
        HIPCHK(c, hipMemsetAsync(c->fr.d_in[s - 1], 0, n * sizeof(float2), c->st.stream));
    }
    const size_t hist = 2 * (size_t)kFrHist * P.stages;
    if (c->fr.d_hist.alloc(hist) != hipSuccess || c->fr.d_taps.alloc(2 * (size_t)P.K + 3) != hipSuccess)
        return fail(c, SDRX_ENOMEM, "sdrx_finalize: no device memory for the front stage");
    HIPCHK(c, hipMemsetAsync(c->fr.d_hist, 0, hist * sizeof(float2), c->st.stream));
    std::vector<float> g(2 * (size_t)P.K + 3);
    for (int i = 0; i <= 2 * P.K + 1; ++i)
        g[(size_t)i] = c->fr.taps[2 * (size_t)i];
    g[2 * (size_t)P.K + 2] = c->fr.taps[(size_t)front_centre(P.K)];
    HIPCHK(c, hipMemcpy(c->fr.d_taps, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice));
    return SDRX_OK;
}

// Impulse blanker: why this context cannot have it, or nothing ...
int blank_plan(sdrx_ctx *c)
{
    if (c->bl.on && c->fr.on && c->fr.plan.real)
        return fail(c, SDRX_EUNSUPPORTED, "blanker: a real first front stage (sdrx_set_front with real_input = 1) reads the caller's words itself -- there is "
                                          "no complex frame in front of it to blank");
    return SDRX_OK;
}

// ... and what k_blank needs on the device: the staging frame the ingest kernels write (whole tiles plus one, zeroed), the state
// (no reference yet, no carry, an empty histogram) and the record buffers of both frame parities.  All of it or (the caller
// releases) none.
int blank_setup(sdrx_ctx *c)
{
    c->bl.reset_used();
    if (!c->bl.on)
        return SDRX_OK;
    const size_t stage = align_up((size_t)c->in_frame, kChunk) + kChunk;
    if (c->bl.d_stage.alloc(stage) != hipSuccess || c->bl.d_state.alloc(1) != hipSuccess || c->bl.rec.alloc(sizeof(BlankRecord)) != hipSuccess)
        return fail(c, SDRX_ENOMEM, "sdrx_finalize: no device memory for the blanker");
    HIPCHK(c, hipMemsetAsync(c->bl.d_stage, 0, stage * sizeof(float2), c->st.stream));
    std::vector<BlankState> st(1);
    memset(st.data(), 0, sizeof(BlankState));
    st[0].ref_bin = -1, st[0].tail_gap = kBlankNoHit, st[0].last_hit = -1;
    HIPCHK(c, hipMemcpy(c->bl.d_state, st.data(), sizeof(BlankState), hipMemcpyHostToDevice));
    return SDRX_OK;
}

// IQ balance correction: why this context cannot have it, or nothing ...
int iqbal_plan(sdrx_ctx *c)
{
    if (c->iq.on && c->fr.on && c->fr.plan.real)
        return fail(c, SDRX_EUNSUPPORTED, "IQ balance: a real first front stage (sdrx_set_front with real_input = 1) reads the caller's words itself -- there "
                                          "is no complex frame in front of it, and I/Q made digitally has no imbalance");
    return SDRX_OK;
}

// ... and what k_iqbal needs on the device: the state (the pair c0, d0 and empty accumulators) and the record buffers of both
// frame parities.  All of it or (the caller releases) none.
int iqbal_setup(sdrx_ctx *c)
{
    c->iq.reset_used();
    if (!c->iq.on)
        return SDRX_OK;
    if (c->iq.d_state.alloc(1) != hipSuccess || c->iq.rec.alloc(sizeof(IqRecord)) != hipSuccess)
        return fail(c, SDRX_ENOMEM, "sdrx_finalize: no device memory for the IQ balance correction");
    IqState st;
    memset(&st, 0, sizeof st);
    st.c = c->iq.cfg.c0, st.d = c->iq.cfg.d0;
    HIPCHK(c, hipMemcpy(c->iq.d_state, &st, sizeof st, hipMemcpyHostToDevice));
    return SDRX_OK;
}

// The shift's three tables A | B | C into a buffer of 3 * kShTab entries its owner allocated: the shift's, or the spur canceller's
// where the shift is off (sdrx_ctx::shift_tables_dev hands out the one there is).
hipError_t fill_shift_tables(DevBuf<float2> &d_tab)
{
    std::vector<float> tab(3 * kShTab * 2);
    shift_tables(tab.data());
    return hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
}

// Frequency shift: what k_shift needs on the device -- the state (phase0, inc), the three tables and the record buffers of both
// frame parities.  All of it or (the caller releases) none.  It is offered behind every ingest chain, a real first front stage
// included: it works on the tree's raw frame.
int shift_setup(sdrx_ctx *c)
{
    c->sh.reset_used();
    if (!c->sh.on)
        return SDRX_OK;
    if (c->sh.d_state.alloc(1) != hipSuccess || c->sh.d_tab.alloc(3 * kShTab) != hipSuccess || c->sh.rec.alloc(sizeof(ShiftRecord)) != hipSuccess)
        return fail(c, SDRX_ENOMEM, "sdrx_finalize: no device memory for the frequency shift");
    ShiftState st;
    memset(&st, 0, sizeof st);
    st.phase = c->sh.cfg.phase0, st.inc = c->sh.cfg.inc;
    HIPCHK(c, hipMemcpy(c->sh.d_state, &st, sizeof st, hipMemcpyHostToDevice));
    HIPCHK(c, fill_shift_tables(c->sh.d_tab));
    return SDRX_OK;
}

// Spur canceller: the eight tone slots at (0, inc0, 0), c[b][k] and used[b][k] of one frame's blocks, the record buffers of both
// frame parities, and the three tables unless the shift's copy serves.  All of it or (the caller releases) none.
int notch_setup(sdrx_ctx *c)
{
    c->nt.reset_used();
    if (!c->nt.on)
        return SDRX_OK;
    const size_t per_frame = (size_t)notch_blocks(c->root_frame) * kNtMax;
    if (c->nt.d_state.alloc(kNtMax) != hipSuccess || c->nt.d_c.alloc(per_frame, true) != hipSuccess || c->nt.d_used.alloc(per_frame, true) != hipSuccess ||
        c->nt.rec.alloc(sizeof(NotchRecord)) != hipSuccess || (!c->sh.on && c->nt.d_tab.alloc(3 * kShTab) != hipSuccess))
        return fail(c, SDRX_ENOMEM, "sdrx_finalize: no device memory for the spur canceller");
    NotchTone st[kNtMax];
    memset(st, 0, sizeof st);
    for (int k = 0; k < (int)c->nt.cfg.n_tones; ++k)
        st[k].inc = st[k].inc0 = st[k].inc_used = c->nt.cfg.inc0[k];
    HIPCHK(c, hipMemcpy(c->nt.d_state, st, sizeof st, hipMemcpyHostToDevice));
    if (!c->sh.on)
        HIPCHK(c, fill_shift_tables(c->nt.d_tab));
    return SDRX_OK;
}

// The route of a frame through the ingest chain, planned once: every buffer exists by now and stays until free_device_state.
//   - the format conversion (or the DC form's last kernel) writes ingest_out: the blanker's staging frame if it is on, else what
//     the blanker would have written;
//   - k_iqbal works in place on ingest_out (so in front of the blanker, on what the blanker reads);
//   - k_blank reads its staging frame and writes blank_out: the first front stage's input frame, else what the front stage
//     would have written;
//   - front stage s reads fr.d_in[s - 1] and writes fr.d_in[s]; the last one writes front_out: the resampler's staging frame,
//     else the tree's raw frame.  (A real first stage reads the caller's words; nothing is staged in front of it, fr.d_in[0] is
//     empty and ingest_out is never written: blank_plan and iqbal_plan refused the two stages that would.)
//   - k_resample reads its staging frame and writes the tree's raw frame, d_raw_tiled;
//   - the spur canceller, then the shift, work in place on d_raw_tiled.
// Whatever is on, the last destination is the tree's raw frame.  The order is ingest_chain_launch's (sdrx_frame.hip).
void plan_ingest_route(sdrx_ctx *c)
{
    sdrx_ctx::IngestRoute &R = c->route;
    R.front_out = c->rs.on ? c->rs.d_stage.get() : c->d_raw_tiled.get();
    R.blank_out = c->fr.on ? c->fr.d_in[0].get() : R.front_out;
    R.ingest_out = c->bl.on ? c->bl.d_stage.get() : R.blank_out;
}

int finalize_impl(sdrx_ctx *c)
{
    if (int rc = derive_nodes(c))
        return rc;
    // the ingest stages' plans: the frame lengths from the tree outwards (each stage in front multiplies what is behind it), then
    // the two stages a real first front stage rules out (the blanker first: its message is what a context with both gets)
    if (int rc = resample_plan_frames(c))
        return rc;
    if (int rc = front_plan_frames(c))
        return rc;
    if (int rc = blank_plan(c))
        return rc;
    if (int rc = iqbal_plan(c))
        return rc;
    Built B;
    plan_buffers(c, B);
    if (int rc = build_mix_work(c, B))
        return rc;
    build_tail_work(c, B);
    build_level_plan(c, B);
    build_meter_plan(c, B);
    if (int rc = allocate_and_upload(c, B))
        return rc;
    build_publish_order(c);
    if (int rc = squelch_setup(c))
        return rc;
    if (int rc = park_setup(c, B))
        return rc;
    if (int rc = agc_setup(c))
        return rc;
    if (int rc = adc_setup(c))
        return rc;
    // the ingest stages' device state, in chain order, and the route between their buffers
    if (int rc = iqbal_setup(c))
        return rc;
    if (int rc = blank_setup(c))
        return rc;
    if (int rc = front_setup(c))
        return rc;
    if (int rc = resample_setup(c))
        return rc;
    if (int rc = notch_setup(c))
        return rc;
    if (int rc = shift_setup(c))
        return rc;
    plan_ingest_route(c);
    catchup_setup(c, B);
    c->sq.preroll_fused = false;
    for (const Node &n : c->nodes)
        c->sq.preroll_fused |= n.fused_demod;
    c->taps.clear();
    c->finalized = true;
    return SDRX_OK;
}

} // namespace
