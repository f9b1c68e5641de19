// sdrx_watch.hip -- host side of option "watch" (include/sdrx.h "Channel watch", watch.hip) and of the analyses on
// a watched source's spectrum (drift estimate, 4n; band scan, 4o): a leaf's band, the launch lists of the measured sources, what
// an analysis per source keeps (sdrx_ctx::SourceAnalysis), and the ABI calls.  The launches themselves sit in the frame sequence
// (watch_launch / watch_raw_step, sdrx_frame.hip), the records' way to the host in sdrx_delivery.hip (queue_watch).
// A fragment of sdrx.hip's translation unit.

namespace {

int wake_rebuild(sdrx_ctx *c); // (sdrx_wake.hip: option wake's launch list follows the watch's)

// The band of a leaf in bins of its source's 8192-point spectrum: include/sdrx.h, in IEEE double.
void watch_band(const sdrx_vfo_desc &d, int *first_bin, int *n_bins)
{
    const double f = d.mixer_freq_hz, fs = (double)d.fs;
    const double R = fs / (double)(1 << d.decimate_count);
    double lo, hi;
    if (d.demod_usb) {
        const double R_out = d.late_decimate == 5 || d.late_decimate == 6 ? R / (double)d.late_decimate : R;
        double B = d.filter_bw_hz > 0 ? (double)d.filter_bw_hz : R_out / 2;
        if (B > R_out / 2)
            B = R_out / 2;
        lo = -f;
        hi = -f + B;
    } else {
        lo = -f - R / 2;
        hi = -f + R / 2;
    }
    const long long k_lo = (long long)std::ceil(lo * 8192.0 / fs), k_hi = (long long)std::floor(hi * 8192.0 / fs);
    const long long nb = std::min<long long>(std::max<long long>(k_hi - k_lo + 1, 1), kSpecN);
    *n_bins = (int)nb;
    *first_bin = (int)(((k_lo % kSpecN) + kSpecN) % kSpecN);
}

// host bookkeeping of every leaf and the slot of every possible source (no device memory): by the first watch call of a
// finalized context
void watch_host_init(sdrx_ctx *c)
{
    sdrx_ctx::Watch &W = c->watch;
    if (!W.leaf.empty())
        return;
    W.leaf.assign(c->nodes.size(), sdrx_ctx::Watch::Leaf());
    W.src_slot.assign(c->nodes.size() + 1, -1);
    W.n_slots = 0;
    W.n_src_slots = 0;
    W.src_slot[0] = W.n_src_slots++;
    for (size_t id = 0; id < c->nodes.size(); ++id) {
        if (!c->nodes[id].leaf) {
            W.src_slot[1 + id] = W.n_src_slots++;
            continue;
        }
        W.leaf[id].slot = W.n_slots++;
        watch_band(c->nodes[id].d, &W.leaf[id].first_bin, &W.leaf[id].n_bins);
    }
    W.seg_begin.assign((size_t)c->n_levels + 2, 0);
    W.leaf_begin.assign((size_t)c->n_levels + 2, 0);
}

int watch_segments(int n) { return std::min(std::max(n / kSpecN, 1), kWatchMaxSeg); }

// A source is launched with its group: 0 the raw frame (id -1), 1 + l the streams of tree level l.  The frame a kernel finds
// in a stream is its level's (only the frame pipeline, at most kMaxLevels deep, has frames per level); -1: the raw frame's.
size_t source_of(const sdrx_ctx *c, int leaf_id) { return (size_t)(1 + c->nodes[(size_t)leaf_id].d.parent_id); }
int source_group(const sdrx_ctx *c, int id) { return id < 0 ? 0 : c->nodes[(size_t)id].level + 1; }
int source_level(int g) { return g == 0 ? -1 : std::min(g - 1, kMaxLevels - 1); }

// The setting S becomes `to` before frame `now`; false: it is `to` already.  (A second change before the same frame: the frames
// before it ran in the state they ran in.)
bool switch_to(sdrx_ctx::Switched &S, int to, unsigned long long now)
{
    if (S.v == to)
        return false;
    if (S.since != now)
        S.was = S.v;
    S.v = to;
    S.since = now;
    return true;
}

// ---- what the drift estimate and the band scan share: an analysis per source
// the analysis's bookkeeping of the source of `leaf_id` (host memory: sized by the first call, whatever it sets)
sdrx_ctx::SourceAnalysis::Src &analysis_source(sdrx_ctx *c, sdrx_ctx::SourceAnalysis &A, int leaf_id)
{
    if (A.src.empty())
        A.src.resize(c->nodes.size() + 1);
    return A.src[source_of(c, leaf_id)];
}
// first use on the device: the launch list (`desc_bytes` per possible source) and the records (`rec_bytes` per possible source),
// both or neither
int analysis_alloc(sdrx_ctx *c, sdrx_ctx::SourceAnalysis &A, size_t desc_bytes, size_t rec_bytes)
{
    if (A.d_desc)
        return SDRX_OK;
    HIPCHK(c, A.d_desc.alloc(desc_bytes * (size_t)c->watch.n_src_slots));
    const hipError_t e = A.rec.alloc(rec_bytes * (size_t)c->watch.n_src_slots);
    if (e == hipSuccess)
        return SDRX_OK;
    A.d_desc.reset();
    return fail(c, SDRX_EHIP, "no memory for the analysis's records: %s", hipGetErrorString(e));
}
// a source's state, cleared, by the first call that switches the analysis on for it
int analysis_state(sdrx_ctx *c, sdrx_ctx::SourceAnalysis::Src &S, size_t state_bytes)
{
    if (!S.d_state)
        HIPCHK(c, S.d_state.alloc(state_bytes, true));
    return SDRX_OK;
}
bool analysis_on(const sdrx_ctx::SourceAnalysis &A, size_t src) { return !A.src.empty() && A.src[src].on.v != 0; }

// was the source of `leaf_id` measured by the analysis in frame `frame`: switched on then, and a leaf of it watched
bool analysis_measured_at(const sdrx_ctx *c, const sdrx_ctx::SourceAnalysis &A, int leaf_id, unsigned long long frame)
{
    if (A.src.empty() || A.src[source_of(c, leaf_id)].on.at(frame) == 0)
        return false;
    const int parent = c->nodes[(size_t)leaf_id].d.parent_id;
    for (size_t id = 0; id < c->nodes.size(); ++id)
        if (c->nodes[id].leaf && c->nodes[id].d.parent_id == parent && c->watch.watched_at((int)id, frame))
            return true;
    return false;
}

// The record of the source of `leaf_id` for the delivered frame (sdrx_get_drift, sdrx_get_scan): zeros but for the frame where
// the source was not measured.  Out is the ABI's name for the device's record (the static_asserts of sdrx.hip).
template <class Out>
int analysis_record(sdrx_ctx *c, const char *what, const sdrx_ctx::SourceAnalysis *which, int leaf_id, Out *out)
{
    if (int rc = leaf_call(c, what, &sdrx_ctx::opt_watch, "watch", &leaf_id, out != nullptr, 1, kDelivered))
        return rc;
    const sdrx_ctx::SourceAnalysis &A = *which; // (of `c`: null with a null handle, which leaf_call has refused)
    Out r;
    memset(&r, 0, sizeof r);
    r.frame = (int64_t)c->host_frame;
    if (A.rec.h[c->host_slot] && analysis_measured_at(c, A, leaf_id, c->host_frame))
        memcpy(&r, A.rec.host<Out>(c->host_slot) + c->watch.src_slot[source_of(c, leaf_id)], sizeof r);
    *out = r;
    return SDRX_OK;
}

// The one walk over the measured sources `ids` (watch_rebuild's launch order: by source group) whose PSDs lie at `off_psd` in
// the watch's data: add(source index, level, psd) says how many launch entries the source adds to an analysis's list.  Returns
// the first entry of every source group.
std::vector<int> walk_sources(const sdrx_ctx *c, const std::vector<int> &ids, const std::vector<size_t> &off_psd,
                              const std::function<int(size_t, int, const double *)> &add)
{
    std::vector<int> begin((size_t)c->n_levels + 2, 0);
    int n = 0;
    size_t k = 0;
    for (int g = 0; g <= c->n_levels; ++g) {
        begin[(size_t)g] = n;
        for (; k < ids.size() && source_group(c, ids[k]) == g; ++k)
            n += add((size_t)(1 + ids[k]), source_level(g), reinterpret_cast<const double *>(c->watch.d_data + off_psd[k]));
    }
    begin[(size_t)c->n_levels + 1] = n;
    return begin;
}

// The drift launch list: the sources among the measured ones with max_shift > 0, one entry per block of shifts.  Synchronous,
// as watch_rebuild is.  Nothing before the first sdrx_set_drift that switched a source on.
int drift_rebuild(sdrx_ctx *c, const std::vector<int> &ids, const std::vector<size_t> &off_psd)
{
    sdrx_ctx::Drift &D = c->drift;
    if (!D.d_desc)
        return SDRX_OK;
    std::vector<DriftSrc> srcs;
    std::vector<DriftBlk> blks;
    const std::vector<int> begin = walk_sources(c, ids, off_psd, [&](size_t i, int level, const double *psd) {
        const int K = D.src[i].on.v;
        if (K == 0)
            return 0;
        const int n_blocks = (2 * K + 1 + kDriftBlock - 1) / kDriftBlock;
        for (int b = 0; b < n_blocks; ++b)
            blks.push_back(DriftBlk{(int)srcs.size(), b});
        srcs.push_back(DriftSrc{psd, reinterpret_cast<DriftState *>(D.src[i].d_state.get()), K, n_blocks, level, c->watch.src_slot[i]});
        return n_blocks;
    });
    if (!srcs.empty()) {
        HIPCHK(c, hipMemcpy(D.d_src(), srcs.data(), sizeof(DriftSrc) * srcs.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(D.d_blk(c->watch.n_src_slots), blks.data(), sizeof(DriftBlk) * blks.size(), hipMemcpyHostToDevice));
    }
    D.begin = begin;
    return SDRX_OK;
}

// The scan launch list: the sources among the measured ones with cell_bins > 0, one workgroup each.  Nothing before the first
// sdrx_set_scan that switched a source on.
int scan_rebuild(sdrx_ctx *c, const std::vector<int> &ids, const std::vector<size_t> &off_psd)
{
    sdrx_ctx::Scan &S = c->scan;
    if (!S.d_desc)
        return SDRX_OK;
    std::vector<ScanSrc> srcs;
    const std::vector<int> begin = walk_sources(c, ids, off_psd, [&](size_t i, int level, const double *psd) {
        if (S.src[i].on.v == 0)
            return 0;
        srcs.push_back(ScanSrc{psd, reinterpret_cast<ScanState *>(S.src[i].d_state.get()), S.cfg[i], level, c->watch.src_slot[i]});
        return 1;
    });
    if (!srcs.empty())
        HIPCHK(c, hipMemcpy(S.d_src(), srcs.data(), sizeof(ScanSrc) * srcs.size(), hipMemcpyHostToDevice));
    S.begin = begin;
    return SDRX_OK;
}

// what is wrong with a setting that switches a scan on (include/sdrx.h "Band scan", the table)
const char *bad_scan(const sdrx_scan_cfg &s)
{
    const int w = s.cell_bins;
    if (w < 1 || w > kScanMaxCellBins || (w & (w - 1)) != 0)
        return "cell_bins must be 0 or a power of two 1 .. 256";
    if (s.frames < 1 || s.frames > 65536)
        return "frames must lie in 1 .. 65536";
    if (s.floor_permille < 0 || s.floor_permille > 1000)
        return "floor_permille must lie in 0 .. 1000";
    if (s.ratio_q8 == 0)
        return "ratio_q8 must be at least 1";
    if (s.min_cells < 1 || s.min_cells > kSpecN / w)
        return "min_cells must lie in 1 .. 8192 / cell_bins";
    return nullptr;
}

// first use on the device: the launch lists, the tables and the records
int watch_first_use(sdrx_ctx *c)
{
    sdrx_ctx::Watch &W = c->watch;
    const std::vector<float2> tab = spectrum_tables();
    HIPCHK(c, W.d_desc.alloc((sizeof(WatchSrc) + sizeof(WatchSeg) * kWatchMaxSeg) * (size_t)W.n_src_slots + sizeof(WatchLeaf) * (size_t)W.n_slots));
    HIPCHK(c, W.d_tw.alloc(tab.size()));
    HIPCHK(c, hipMemcpy(W.d_tw, tab.data(), sizeof(float2) * tab.size(), hipMemcpyHostToDevice));
    HIPCHK(c, W.rec.alloc(sizeof(WatchRecord) * (size_t)W.n_slots));
    return SDRX_OK;
}

// The launch lists for the present selection, uploaded whenever it or a watched leaf's band changes.  Synchronous: never inside
// a frame call, and the context is drained.  The sources in launch order: the raw frame, then the parents by tree level.
int watch_rebuild(sdrx_ctx *c)
{
    sdrx_ctx::Watch &W = c->watch;
    const int N = (int)c->nodes.size();
    std::vector<char> measured((size_t)N + 1, 0); // [0]: the raw frame, [1 + id]: the stream of node id
    bool any = false;
    for (int id = 0; id < N; ++id)
        if (W.leaf[(size_t)id].on.v) {
            measured[source_of(c, id)] = 1;
            any = true;
        }
    if (!any && !W.d_desc) // nothing was ever switched on: nothing is allocated
        return SDRX_OK;
    if (!W.d_desc)
        if (int rc = watch_first_use(c)) { // all of it or none: the next call starts here again
            static_cast<sdrx_ctx::WatchDevice &>(W) = sdrx_ctx::WatchDevice();
            return rc;
        }
    // the measured sources, by group, and where each one's buffers lie
    std::vector<int> ids;
    std::vector<WatchSrc> srcs;
    std::vector<WatchSeg> segs;
    std::vector<size_t> off_P, off_psd, off_done;
    std::vector<int> src_index((size_t)N + 1, -1);
    size_t need = 0;
    auto take = [&](size_t bytes) {
        const size_t o = align_up(need, 256);
        need = o + bytes;
        return o;
    };
    for (int g = 0; g <= c->n_levels; ++g) {
        W.seg_begin[(size_t)g] = (int)segs.size();
        for (int id = -1; id < N; ++id) {
            if (!measured[(size_t)(1 + id)] || source_group(c, id) != g)
                continue;
            WatchSrc e;
            memset(&e, 0, sizeof e);
            e.n = id < 0 ? c->root_frame : c->nodes[(size_t)id].n_f;
            e.S = watch_segments(e.n);
            e.level = source_level(g);
            if (id >= 0)
                for (int p = 0; p < 2; ++p)
                    e.src[p] = reinterpret_cast<const float2 *>(c->arena + c->nodes[(size_t)id].off_stream[p]);
            src_index[(size_t)(1 + id)] = (int)srcs.size();
            for (int s = 0; s < e.S; ++s)
                segs.push_back(WatchSeg{(int)srcs.size(), s});
            off_P.push_back(take(sizeof(float) * (size_t)e.S * kSpecN));
            off_psd.push_back(take(sizeof(double) * ((size_t)kSpecN + 1)));
            off_done.push_back(take(sizeof(unsigned)));
            ids.push_back(id);
            srcs.push_back(e);
        }
    }
    W.seg_begin[(size_t)c->n_levels + 1] = (int)segs.size();
    if (ids != W.src_ids || need > W.d_data.bytes()) { // the buffers move: what they held is gone
        HIPCHK(c, W.d_data.reserve(need));
        if (W.d_data)
            HIPCHK(c, hipMemset(W.d_data, 0, W.d_data.bytes()));
        W.psd_since = c->frame_no;
    }
    W.src_psd = off_psd;
    for (size_t k = 0; k < srcs.size(); ++k) {
        srcs[k].P = reinterpret_cast<float *>(W.d_data + off_P[k]);
        srcs[k].psd = reinterpret_cast<double *>(W.d_data + off_psd[k]);
        srcs[k].done = reinterpret_cast<unsigned *>(W.d_data + off_done[k]);
    }
    // the watched leaves in the order of their sources
    std::vector<WatchLeaf> leaves;
    for (int g = 0; g <= c->n_levels; ++g) {
        W.leaf_begin[(size_t)g] = (int)leaves.size();
        for (int id = 0; id < N; ++id) {
            const sdrx_ctx::Watch::Leaf &L = W.leaf[(size_t)id];
            const int parent = c->nodes[(size_t)id].d.parent_id;
            if (!L.on.v || source_group(c, parent) != g)
                continue;
            leaves.push_back(WatchLeaf{src_index[(size_t)(1 + parent)], L.first_bin, L.n_bins, L.slot});
        }
    }
    W.leaf_begin[(size_t)c->n_levels + 1] = (int)leaves.size();
    if (!srcs.empty()) {
        HIPCHK(c, hipMemcpy(W.d_src(), srcs.data(), sizeof(WatchSrc) * srcs.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(W.d_seg(), segs.data(), sizeof(WatchSeg) * segs.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(W.d_leaf(), leaves.data(), sizeof(WatchLeaf) * leaves.size(), hipMemcpyHostToDevice));
    }
    if (int rc = drift_rebuild(c, ids, off_psd)) // (the templates stay where they are; their sources' PSDs may have moved)
        return rc;
    if (int rc = scan_rebuild(c, ids, off_psd)) // (so do the scans' states)
        return rc;
    const std::vector<WatchLeaf> leaves_before = W.launch_leaves;
    W.launch_leaves = leaves;
    if (int rc = wake_rebuild(c)) { // (the controlled leaves' sources and bands)
        W.launch_leaves = leaves_before;
        return rc;
    }
    W.src_ids = ids; // (last: the frame sequence launches from these lists only when everything above succeeded)
    return SDRX_OK;
}

// sdrx_set_mixer_freqs has changed the descriptors of `ids` (the context is drained): the bands follow
int watch_retuned(sdrx_ctx *c, const int *ids, int n)
{
    sdrx_ctx::Watch &W = c->watch;
    if (!c->opt_watch || W.leaf.empty())
        return SDRX_OK;
    bool any = false;
    for (int k = 0; k < n; ++k) {
        sdrx_ctx::Watch::Leaf &L = W.leaf[(size_t)ids[k]];
        if (L.slot < 0)
            continue;
        watch_band(c->nodes[(size_t)ids[k]].d, &L.first_bin, &L.n_bins);
        any |= L.on.v != 0;
    }
    return any ? watch_rebuild(c) : SDRX_OK;
}

// A call `what` about the source of ONE watched leaf between frames -- it changes what the next frame measures, or reads the
// device: leaf_call's checks with "the leaf is watched" in front of the caller's own `bad`, then the context's device, drained
// (frames inside the software pipeline finish with the old setting).
int watched_leaf_call(sdrx_ctx *c, const char *what, int leaf_id, bool arrays, const std::function<const char *()> &bad = nullptr)
{
    auto all = [&](int) -> const char * {
        if (c->watch.leaf.empty() || !c->watch.leaf[(size_t)leaf_id].on.v)
            return "is not watched (sdrx_set_watch)";
        return bad ? bad() : nullptr;
    };
    if (int rc = leaf_call(c, what, &sdrx_ctx::opt_watch, "watch", &leaf_id, arrays, 1, kBetweenFrames, all))
        return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return drain(c);
}

// what sdrx_get_scan_hits and sdrx_get_scan_cells share: the checks, and the record of the last completed evaluation
int scan_evaluation(sdrx_ctx *c, const char *what, int leaf_id, bool arrays, const ScanState **state, ScanRecord *head)
{
    auto bad = [&] { return analysis_on(c->scan, source_of(c, leaf_id)) ? nullptr : "its source has no band scan (sdrx_set_scan)"; };
    if (int rc = watched_leaf_call(c, what, leaf_id, arrays, bad))
        return rc;
    const ScanState *st = reinterpret_cast<const ScanState *>(c->scan.src[source_of(c, leaf_id)].d_state.get());
    struct {
        ScanRecord head;
        unsigned count, valid;
    } tail;
    static_assert(offsetof(ScanState, count) == offsetof(ScanState, head) + sizeof(ScanRecord), "head, count and valid are read together");
    HIPCHK(c, hipMemcpy(&tail, reinterpret_cast<const unsigned char *>(st) + offsetof(ScanState, head), sizeof tail, hipMemcpyDeviceToHost));
    if (!tail.valid)
        return fail(c, SDRX_ESTATE, "%s: no evaluation has completed for the source of vfo %d under the present setting yet", what, leaf_id);
    *state = st;
    *head = tail.head;
    return SDRX_OK;
}

} // namespace

extern "C" {

int sdrx_set_watch(sdrx_ctx *c, const int *ids, const int32_t *on, int n)
{
    if (int rc = leaf_call(c, "sdrx_set_watch", &sdrx_ctx::opt_watch, "watch", ids, on != nullptr, n, kBetweenFrames, [&](int k) {
            return !on[k] && c->wake.controlled(ids[k]) ? "is under the device's wake control (sdrx_set_wake)" : bad_switch(on[k]);
        }))
        return rc;
    if (n == 0)
        return SDRX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c)) // frames inside the software pipeline finish with the old selection
        return rc;
    watch_host_init(c);
    sdrx_ctx::Watch &W = c->watch;
    const std::vector<sdrx_ctx::Watch::Leaf> before = W.leaf;
    bool changed = false;
    for (int k = 0; k < n; ++k)
        changed |= switch_to(W.leaf[(size_t)ids[k]].on, on[k], c->frame_no);
    if (!changed)
        return SDRX_OK;
    const int rc = watch_rebuild(c);
    if (rc) { // the lists on the device are the old ones (W.src_ids is set last): so is the selection
        W.leaf = before;
        return rc;
    }
    return SDRX_OK;
}

int sdrx_get_watch(sdrx_ctx *c, const int *ids, int n, sdrx_watch_level *out)
{
    if (int rc = leaf_call(c, "sdrx_get_watch", &sdrx_ctx::opt_watch, "watch", ids, out != nullptr, n, kDelivered))
        return rc;
    if (n == 0)
        return SDRX_OK;
    watch_host_init(c);
    const sdrx_ctx::Watch &W = c->watch;
    for (int k = 0; k < n; ++k) {
        const sdrx_ctx::Watch::Leaf &L = W.leaf[(size_t)ids[k]];
        sdrx_watch_level r;
        memset(&r, 0, sizeof r);
        if (W.rec.h[c->host_slot] && W.watched_at(ids[k], c->host_frame)) {
            memcpy(&r, W.rec.host<WatchRecord>(c->host_slot) + L.slot, sizeof r);
        } else {
            r.first_bin = L.first_bin;
            r.n_bins = L.n_bins;
        }
        r.frame = (int64_t)c->host_frame;
        out[k] = r;
    }
    return SDRX_OK;
}

int sdrx_get_watch_psd(sdrx_ctx *c, int leaf_id, double *psd, int64_t *frame)
{
    if (int rc = watched_leaf_call(c, "sdrx_get_watch_psd", leaf_id, true))
        return rc;
    const sdrx_ctx::Watch &W = c->watch;
    if (c->frame_no <= std::max(W.psd_since, W.leaf[(size_t)leaf_id].on.since))
        return fail(c, SDRX_ESTATE, "sdrx_get_watch_psd: no frame has been measured for vfo %d yet", leaf_id);
    const int parent = c->nodes[(size_t)leaf_id].d.parent_id;
    size_t k = 0;
    while (k < W.src_ids.size() && W.src_ids[k] != parent)
        ++k;
    if (k == W.src_ids.size())
        return fail(c, SDRX_EHIP, "sdrx_get_watch_psd: the source of vfo %d is not in the launch list", leaf_id);
    if (psd)
        HIPCHK(c, hipMemcpy(psd, W.d_data + W.src_psd[k], sizeof(double) * kSpecN, hipMemcpyDeviceToHost));
    if (frame)
        *frame = (int64_t)c->frame_no - 1;
    return SDRX_OK;
}

int sdrx_set_drift(sdrx_ctx *c, int leaf_id, const double *templ, int max_shift)
{
    auto bad = [&]() -> const char * {
        if (max_shift < 0 || max_shift > SDRX_DRIFT_MAX_SHIFT)
            return "max_shift must lie in 0 .. SDRX_DRIFT_MAX_SHIFT";
        for (int i = 0; templ && max_shift > 0 && i < kSpecN; ++i)
            if (!(templ[i] >= 0.0) || !std::isfinite(templ[i]))
                return "a template entry is negative or not finite";
        return nullptr;
    };
    if (int rc = watched_leaf_call(c, "sdrx_set_drift", leaf_id, true, bad))
        return rc;
    sdrx_ctx::Drift &D = c->drift;
    sdrx_ctx::SourceAnalysis::Src &S = analysis_source(c, D, leaf_id);
    if (max_shift == 0 && S.on.v == 0)
        return SDRX_OK;
    if (int rc = analysis_alloc(c, D, sizeof(DriftSrc) + sizeof(DriftBlk) * kDriftMaxBlocks, sizeof(DriftRecord)))
        return rc;
    D.set_at.resize(D.src.size(), 0);
    if (max_shift > 0) {
        if (int rc = analysis_state(c, S, sizeof(DriftState)))
            return rc;
        unsigned char *base = S.d_state;
        if (templ)
            HIPCHK(c, hipMemcpy(base + offsetof(DriftState, templ), templ, sizeof(double) * kSpecN, hipMemcpyHostToDevice));
        const unsigned capture = templ ? 0u : 1u; // (an upload also calls off a capture still waiting for its frame)
        HIPCHK(c, hipMemcpy(base + offsetof(DriftState, capture), &capture, sizeof capture, hipMemcpyHostToDevice));
    }
    unsigned long long &set_at = D.set_at[source_of(c, leaf_id)];
    const sdrx_ctx::Switched before = S.on;
    const unsigned long long set_before = set_at;
    switch_to(S.on, max_shift, c->frame_no);
    set_at = c->frame_no;
    if (int rc = drift_rebuild(c, c->watch.src_ids, c->watch.src_psd)) {
        S.on = before;
        set_at = set_before;
        return rc;
    }
    return SDRX_OK;
}

int sdrx_get_drift(sdrx_ctx *c, int leaf_id, sdrx_drift_level *out) { return analysis_record(c, "sdrx_get_drift", c ? &c->drift : nullptr, leaf_id, out); }

int sdrx_get_drift_profile(sdrx_ctx *c, int leaf_id, double *profile, int64_t *frame)
{
    auto bad = [&] { return analysis_on(c->drift, source_of(c, leaf_id)) ? nullptr : "its source has no drift estimate (sdrx_set_drift)"; };
    if (int rc = watched_leaf_call(c, "sdrx_get_drift_profile", leaf_id, true, bad))
        return rc;
    const sdrx_ctx::SourceAnalysis::Src &S = c->drift.src[source_of(c, leaf_id)];
    if (c->frame_no <= std::max(std::max(c->drift.set_at[source_of(c, leaf_id)], S.on.since), c->watch.leaf[(size_t)leaf_id].on.since))
        return fail(c, SDRX_ESTATE, "sdrx_get_drift_profile: no frame has been measured for the source of vfo %d yet", leaf_id);
    if (profile)
        HIPCHK(c, hipMemcpy(profile, S.d_state + offsetof(DriftState, profile), sizeof(double) * (size_t)(2 * S.on.v + 1),
                            hipMemcpyDeviceToHost));
    if (frame)
        *frame = (int64_t)c->frame_no - 1;
    return SDRX_OK;
}

int sdrx_set_scan(sdrx_ctx *c, int leaf_id, const sdrx_scan_cfg *cfg)
{
    const bool on = cfg && cfg->cell_bins != 0;
    auto bad = [&]() -> const char * {
        if (cfg && (cfg->reserved[0] || cfg->reserved[1] || cfg->reserved[2]))
            return "a reserved field is not 0";
        return on ? bad_scan(*cfg) : nullptr;
    };
    if (int rc = watched_leaf_call(c, "sdrx_set_scan", leaf_id, true, bad))
        return rc;
    sdrx_ctx::Scan &S = c->scan;
    sdrx_ctx::SourceAnalysis::Src &R = analysis_source(c, S, leaf_id);
    if (!on && R.on.v == 0)
        return SDRX_OK;
    if (int rc = analysis_alloc(c, S, sizeof(ScanSrc), sizeof(ScanRecord)))
        return rc;
    S.cfg.resize(S.src.size(), ScanCfg{});
    if (on) {
        if (int rc = analysis_state(c, R, sizeof(ScanState)))
            return rc;
        // every accepted setting restarts the integration, and the last evaluation is no longer this setting's
        static_assert(offsetof(ScanState, valid) == offsetof(ScanState, count) + sizeof(unsigned), "count and valid are cleared together");
        HIPCHK(c, hipMemset(R.d_state + offsetof(ScanState, count), 0, 2 * sizeof(unsigned)));
    }
    ScanCfg &kept = S.cfg[source_of(c, leaf_id)];
    const sdrx_ctx::Switched before = R.on;
    const ScanCfg cfg_before = kept;
    switch_to(R.on, on ? cfg->cell_bins : 0, c->frame_no);
    if (on)
        memcpy(&kept, cfg, sizeof kept);
    if (int rc = scan_rebuild(c, c->watch.src_ids, c->watch.src_psd)) {
        R.on = before;
        kept = cfg_before;
        return rc;
    }
    return SDRX_OK;
}

int sdrx_get_scan(sdrx_ctx *c, int leaf_id, sdrx_scan_level *out) { return analysis_record(c, "sdrx_get_scan", c ? &c->scan : nullptr, leaf_id, out); }

int sdrx_get_scan_hits(sdrx_ctx *c, int leaf_id, sdrx_scan_hit *hits, int max_hits, int *n, int64_t *frame)
{
    const ScanState *st = nullptr;
    ScanRecord head;
    if (int rc = scan_evaluation(c, "sdrx_get_scan_hits", leaf_id, max_hits >= 0 && (hits || max_hits == 0), &st, &head))
        return rc;
    const int take = std::min(head.n_stored, max_hits);
    if (take > 0)
        HIPCHK(c, hipMemcpy(hits, reinterpret_cast<const unsigned char *>(st) + offsetof(ScanState, hits), sizeof(ScanHit) * (size_t)take, hipMemcpyDeviceToHost));
    if (n)
        *n = take;
    if (frame)
        *frame = (int64_t)head.frame;
    return SDRX_OK;
}

int sdrx_get_scan_cells(sdrx_ctx *c, int leaf_id, double *cells, int64_t *frame)
{
    const ScanState *st = nullptr;
    ScanRecord head;
    if (int rc = scan_evaluation(c, "sdrx_get_scan_cells", leaf_id, true, &st, &head))
        return rc;
    if (cells)
        HIPCHK(c, hipMemcpy(cells, reinterpret_cast<const unsigned char *>(st) + offsetof(ScanState, cells), sizeof(double) * (size_t)(kSpecN / head.cell_bins),
                            hipMemcpyDeviceToHost));
    if (frame)
        *frame = (int64_t)head.frame;
    return SDRX_OK;
}

} // extern "C"
