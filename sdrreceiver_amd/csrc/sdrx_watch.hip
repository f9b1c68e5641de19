// sdrx_watch.hip -- host side of option "watch" (include/sdrx.h "Channel watch", watch.hip): a leaf's band, the
// launch lists of the measured sources, and the ABI calls.  The launches themselves sit in the frame sequence
// (watch_launch / watch_raw_step, sdrx_frame.hip), the records' way to the host in sdrx_delivery.hip (queue_watch).
// A fragment of sdrx.hip's translation unit.

namespace {

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

// host bookkeeping of every leaf (no device memory): by the first watch call of a finalized context
void watch_host_init(sdrx_ctx *c)
{
    sdrx_ctx::Watch &W = c->watch;
    if (!W.leaf.empty())
        return;
    W.leaf.assign(c->nodes.size(), sdrx_ctx::Watch::Leaf());
    W.n_slots = 0;
    for (size_t id = 0; id < c->nodes.size(); ++id) {
        if (!c->nodes[id].leaf)
            continue;
        W.leaf[id].slot = W.n_slots++;
        watch_band(c->nodes[id].d, &W.leaf[id].first_bin, &W.leaf[id].n_bins);
    }
    W.seg_begin.assign((size_t)c->n_levels + 2, 0);
    W.leaf_begin.assign((size_t)c->n_levels + 2, 0);
}

int watch_segments(int n) { return std::min(std::max(n / kSpecN, 1), kWatchMaxSeg); }

// ---- drift estimate: host bookkeeping of every possible source (no device memory), by the first drift call
void drift_host_init(sdrx_ctx *c)
{
    sdrx_ctx::Drift &D = c->drift;
    if (!D.src.empty())
        return;
    D.src.assign(c->nodes.size() + 1, sdrx_ctx::Drift::Src());
    D.n_slots = 0;
    D.src[0].slot = D.n_slots++;
    for (size_t id = 0; id < c->nodes.size(); ++id)
        if (!c->nodes[id].leaf)
            D.src[1 + id].slot = D.n_slots++;
}

// The drift launch list for the measured sources `ids` (watch_rebuild's launch order: by source group) whose PSDs lie at
// `off_psd` in the watch's data: the sources among them with max_shift > 0, one entry per block of shifts.  Synchronous, as
// watch_rebuild is.  Nothing before the first sdrx_set_drift that switched a source on.
int drift_rebuild(sdrx_ctx *c, const std::vector<int> &ids, const std::vector<size_t> &off_psd)
{
    sdrx_ctx::Drift &D = c->drift;
    if (!D.d_desc)
        return SDRX_OK;
    std::vector<DriftSrc> srcs;
    std::vector<DriftBlk> blks;
    std::vector<int> begin((size_t)c->n_levels + 2, 0);
    size_t k = 0;
    for (int g = 0; g <= c->n_levels; ++g) {
        begin[(size_t)g] = (int)blks.size();
        for (; k < ids.size() && (ids[k] < 0 ? 0 : c->nodes[(size_t)ids[k]].level + 1) == g; ++k) {
            const sdrx_ctx::Drift::Src &S = D.src[(size_t)(1 + ids[k])];
            if (S.K == 0)
                continue;
            DriftSrc e;
            e.psd = reinterpret_cast<const double *>(c->watch.d_data + off_psd[k]);
            e.state = S.d_state;
            e.K = S.K;
            e.n_blocks = (2 * S.K + 1 + kDriftBlock - 1) / kDriftBlock;
            e.level = ids[k] < 0 ? -1 : std::min(g - 1, kMaxLevels - 1);
            e.slot = S.slot;
            for (int b = 0; b < e.n_blocks; ++b)
                blks.push_back(DriftBlk{(int)srcs.size(), b});
            srcs.push_back(e);
        }
    }
    begin[(size_t)c->n_levels + 1] = (int)blks.size();
    if (!srcs.empty()) {
        HIPCHK(c, hipMemcpy(D.d_src(), srcs.data(), sizeof(DriftSrc) * srcs.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(D.d_blk(), blks.data(), sizeof(DriftBlk) * blks.size(), hipMemcpyHostToDevice));
    }
    D.blk_begin = begin;
    return SDRX_OK;
}

// was the source of `leaf_id` measured for its drift in frame `frame`: max_shift > 0 then, and a leaf of it watched
bool drift_measured_at(const sdrx_ctx *c, int leaf_id, unsigned long long frame)
{
    const sdrx_ctx::Drift &D = c->drift;
    if (D.src.empty())
        return false;
    const int parent = c->nodes[(size_t)leaf_id].d.parent_id;
    const sdrx_ctx::Drift::Src &S = D.src[(size_t)(1 + parent)];
    if ((frame >= S.since ? S.K : S.was_K) == 0)
        return false;
    for (size_t id = 0; id < c->nodes.size(); ++id)
        if (c->nodes[id].leaf && c->nodes[id].d.parent_id == parent && c->watch.watched_at((int)id, frame))
            return true;
    return false;
}

// ---- band scan: host bookkeeping of every possible source (no device memory), by the first scan call; the slots are the drift's
void scan_host_init(sdrx_ctx *c)
{
    sdrx_ctx::Scan &S = c->scan;
    if (!S.src.empty())
        return;
    S.src.assign(c->nodes.size() + 1, sdrx_ctx::Scan::Src());
    S.n_slots = 0;
    S.src[0].slot = S.n_slots++;
    for (size_t id = 0; id < c->nodes.size(); ++id)
        if (!c->nodes[id].leaf)
            S.src[1 + id].slot = S.n_slots++;
}

// The scan launch list for the measured sources `ids` whose PSDs lie at `off_psd` (as drift_rebuild): the sources among them
// with cell_bins > 0, one workgroup each.  Nothing before the first sdrx_set_scan that switched a source on.
int scan_rebuild(sdrx_ctx *c, const std::vector<int> &ids, const std::vector<size_t> &off_psd)
{
    sdrx_ctx::Scan &S = c->scan;
    if (!S.d_src)
        return SDRX_OK;
    std::vector<ScanSrc> srcs;
    std::vector<int> begin((size_t)c->n_levels + 2, 0);
    size_t k = 0;
    for (int g = 0; g <= c->n_levels; ++g) {
        begin[(size_t)g] = (int)srcs.size();
        for (; k < ids.size() && (ids[k] < 0 ? 0 : c->nodes[(size_t)ids[k]].level + 1) == g; ++k) {
            const sdrx_ctx::Scan::Src &R = S.src[(size_t)(1 + ids[k])];
            if (R.cfg.cell_bins == 0)
                continue;
            ScanSrc e;
            e.psd = reinterpret_cast<const double *>(c->watch.d_data + off_psd[k]);
            e.state = R.d_state;
            e.cfg = R.cfg;
            e.level = ids[k] < 0 ? -1 : std::min(g - 1, kMaxLevels - 1);
            e.slot = R.slot;
            srcs.push_back(e);
        }
    }
    begin[(size_t)c->n_levels + 1] = (int)srcs.size();
    if (!srcs.empty())
        HIPCHK(c, hipMemcpy(S.d_src, srcs.data(), sizeof(ScanSrc) * srcs.size(), hipMemcpyHostToDevice));
    S.src_begin = begin;
    return SDRX_OK;
}

// was the source of `leaf_id` scanned in frame `frame`: cell_bins > 0 then, and a leaf of it watched
bool scan_measured_at(const sdrx_ctx *c, int leaf_id, unsigned long long frame)
{
    const sdrx_ctx::Scan &S = c->scan;
    if (S.src.empty())
        return false;
    const int parent = c->nodes[(size_t)leaf_id].d.parent_id;
    const sdrx_ctx::Scan::Src &R = S.src[(size_t)(1 + parent)];
    if ((frame >= R.since ? R.cfg.cell_bins : R.was_w) == 0)
        return false;
    for (size_t id = 0; id < c->nodes.size(); ++id)
        if (c->nodes[id].leaf && c->nodes[id].d.parent_id == parent && c->watch.watched_at((int)id, frame))
            return true;
    return false;
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

// The launch lists for the present selection, uploaded whenever it or a watched leaf's band changes.  Synchronous: never inside
// a frame call, and the context is drained.  The sources in launch order: the raw frame, then the parents by tree level.
int watch_rebuild(sdrx_ctx *c)
{
    sdrx_ctx::Watch &W = c->watch;
    const int N = (int)c->nodes.size();
    std::vector<char> measured((size_t)N + 1, 0); // [0]: the raw frame, [1 + id]: the stream of node id
    bool any = false;
    for (int id = 0; id < N; ++id)
        if (W.leaf[(size_t)id].on) {
            measured[(size_t)(1 + c->nodes[(size_t)id].d.parent_id)] = 1;
            any = true;
        }
    if (!any && !W.d_desc) // nothing was ever switched on: nothing is allocated
        return SDRX_OK;
    if (!W.d_desc) {
        int parents = 0;
        for (const Node &n : c->nodes)
            parents += !n.leaf;
        W.src_cap = parents + 1;
        const size_t desc_bytes = (sizeof(WatchSrc) + sizeof(WatchSeg) * kWatchMaxSeg) * (size_t)W.src_cap + sizeof(WatchLeaf) * (size_t)W.n_slots;
        const size_t rec_bytes = sizeof(WatchRecord) * (size_t)W.n_slots;
        const std::vector<float2> tab = spectrum_tables();
        HIPCHK(c, hipMalloc(&W.d_desc, desc_bytes));
        HIPCHK(c, hipMalloc(&W.d_tw, sizeof(float2) * tab.size()));
        HIPCHK(c, hipMemcpy(W.d_tw, tab.data(), sizeof(float2) * tab.size(), hipMemcpyHostToDevice));
        for (int p = 0; p < 2; ++p) {
            HIPCHK(c, hipMalloc(&W.d_rec[p], rec_bytes));
            HIPCHK(c, hipMemset(W.d_rec[p], 0, rec_bytes));
            HIPCHK(c, hipHostMalloc(&W.h_rec[p], rec_bytes, hipHostMallocDefault));
            memset(W.h_rec[p], 0, rec_bytes);
        }
        W.bytes = desc_bytes + sizeof(float2) * tab.size() + 2 * rec_bytes;
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
            if (!measured[(size_t)(1 + id)] || (id < 0 ? g != 0 : c->nodes[(size_t)id].level != g - 1))
                continue;
            WatchSrc e;
            memset(&e, 0, sizeof e);
            e.n = id < 0 ? c->root_frame : c->nodes[(size_t)id].n_f;
            e.S = watch_segments(e.n);
            e.level = id < 0 ? -1 : std::min(g - 1, kMaxLevels - 1); // (only the frame pipeline, at most kMaxLevels deep, has frames per level)
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
    if (ids != W.src_ids || need > W.data_cap) { // the buffers move: what they held is gone
        if (need > W.data_cap) {
            if (W.d_data)
                (void)hipFree(W.d_data);
            W.d_data = nullptr;
            W.bytes -= W.data_cap;
            W.data_cap = 0;
            HIPCHK(c, hipMalloc(&W.d_data, need));
            W.data_cap = need;
            W.bytes += need;
        }
        if (W.d_data)
            HIPCHK(c, hipMemset(W.d_data, 0, W.data_cap));
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
            if (!L.on || (parent < 0 ? g != 0 : c->nodes[(size_t)parent].level != g - 1))
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
        any |= L.on != 0;
    }
    return any ? watch_rebuild(c) : SDRX_OK;
}

// what sdrx_get_scan_hits and sdrx_get_scan_cells share: the checks, and the record of the last completed evaluation
int scan_evaluation(sdrx_ctx *c, const char *what, int leaf_id, bool arrays, const ScanState **state, ScanRecord *head)
{
    auto bad = [&](int) -> const char * {
        if (c->watch.leaf.empty() || !c->watch.leaf[(size_t)leaf_id].on)
            return "is not watched (sdrx_set_watch)";
        if (c->scan.src.empty() || c->scan.src[(size_t)(1 + c->nodes[(size_t)leaf_id].d.parent_id)].cfg.cell_bins == 0)
            return "its source has no band scan (sdrx_set_scan)";
        return nullptr;
    };
    if (int rc = leaf_call(c, what, &sdrx_ctx::opt_watch, "watch", &leaf_id, arrays, 1, kBetweenFrames, bad))
        return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    const ScanState *st = c->scan.src[(size_t)(1 + c->nodes[(size_t)leaf_id].d.parent_id)].d_state;
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
    if (int rc = leaf_call(c, "sdrx_set_watch", &sdrx_ctx::opt_watch, "watch", ids, on != nullptr, n, kBetweenFrames, [&](int k) { return bad_switch(on[k]); }))
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
    for (int k = 0; k < n; ++k) {
        sdrx_ctx::Watch::Leaf &L = W.leaf[(size_t)ids[k]];
        if (L.on == on[k])
            continue;
        if (L.since != c->frame_no) // (a second change before the same frame: the frames before it ran in the state they ran in)
            L.was_on = L.on;
        L.on = on[k];
        L.since = c->frame_no;
        changed = true;
    }
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
        if (W.h_rec[c->host_slot] && W.watched_at(ids[k], c->host_frame)) {
            memcpy(&r, W.h_rec[c->host_slot] + L.slot, sizeof r);
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
    auto unwatched = [&](int) { return c->watch.leaf.empty() || !c->watch.leaf[(size_t)leaf_id].on ? "is not watched (sdrx_set_watch)" : nullptr; };
    if (int rc = leaf_call(c, "sdrx_get_watch_psd", &sdrx_ctx::opt_watch, "watch", &leaf_id, true, 1, kBetweenFrames, unwatched))
        return rc;
    const sdrx_ctx::Watch &W = c->watch;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    if (c->frame_no <= std::max(W.psd_since, W.leaf[(size_t)leaf_id].since))
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
    auto bad = [&](int) -> const char * {
        if (c->watch.leaf.empty() || !c->watch.leaf[(size_t)leaf_id].on)
            return "is not watched (sdrx_set_watch)";
        if (max_shift < 0 || max_shift > SDRX_DRIFT_MAX_SHIFT)
            return "max_shift must lie in 0 .. SDRX_DRIFT_MAX_SHIFT";
        for (int i = 0; templ && max_shift > 0 && i < kSpecN; ++i)
            if (!(templ[i] >= 0.0) || !std::isfinite(templ[i]))
                return "a template entry is negative or not finite";
        return nullptr;
    };
    if (int rc = leaf_call(c, "sdrx_set_drift", &sdrx_ctx::opt_watch, "watch", &leaf_id, true, 1, kBetweenFrames, bad))
        return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c)) // frames inside the software pipeline finish with the old setting
        return rc;
    drift_host_init(c);
    sdrx_ctx::Drift &D = c->drift;
    sdrx_ctx::Drift::Src &S = D.src[(size_t)(1 + c->nodes[(size_t)leaf_id].d.parent_id)];
    if (max_shift == 0 && S.K == 0)
        return SDRX_OK;
    if (!D.d_desc) {
        const size_t desc_bytes = (sizeof(DriftSrc) + sizeof(DriftBlk) * kDriftMaxBlocks) * (size_t)D.n_slots;
        const size_t rec_bytes = sizeof(DriftRecord) * (size_t)D.n_slots;
        HIPCHK(c, hipMalloc(&D.d_desc, desc_bytes));
        for (int p = 0; p < 2; ++p) {
            HIPCHK(c, hipMalloc(&D.d_rec[p], rec_bytes));
            HIPCHK(c, hipMemset(D.d_rec[p], 0, rec_bytes));
            HIPCHK(c, hipHostMalloc(&D.h_rec[p], rec_bytes, hipHostMallocDefault));
            memset(D.h_rec[p], 0, rec_bytes);
        }
        D.bytes += desc_bytes + 2 * rec_bytes;
    }
    if (max_shift > 0) {
        if (!S.d_state) {
            HIPCHK(c, hipMalloc(&S.d_state, sizeof(DriftState)));
            HIPCHK(c, hipMemset(S.d_state, 0, sizeof(DriftState)));
            D.bytes += sizeof(DriftState);
        }
        unsigned char *base = reinterpret_cast<unsigned char *>(S.d_state);
        if (templ)
            HIPCHK(c, hipMemcpy(base + offsetof(DriftState, templ), templ, sizeof(double) * kSpecN, hipMemcpyHostToDevice));
        const unsigned capture = templ ? 0u : 1u; // (an upload also calls off a capture still waiting for its frame)
        HIPCHK(c, hipMemcpy(base + offsetof(DriftState, capture), &capture, sizeof capture, hipMemcpyHostToDevice));
    }
    const sdrx_ctx::Drift::Src before = S;
    if (S.K != max_shift) {
        if (S.since != c->frame_no) // (as sdrx_set_watch: the frames before ran in the state they ran in)
            S.was_K = S.K;
        S.K = max_shift;
        S.since = c->frame_no;
    }
    S.set_at = c->frame_no;
    if (int rc = drift_rebuild(c, c->watch.src_ids, c->watch.src_psd)) {
        S = before;
        return rc;
    }
    return SDRX_OK;
}

int sdrx_get_drift(sdrx_ctx *c, int leaf_id, sdrx_drift_level *out)
{
    if (int rc = leaf_call(c, "sdrx_get_drift", &sdrx_ctx::opt_watch, "watch", &leaf_id, out != nullptr, 1, kDelivered))
        return rc;
    sdrx_drift_level r;
    memset(&r, 0, sizeof r);
    r.frame = (int64_t)c->host_frame;
    const sdrx_ctx::Drift &D = c->drift;
    if (D.h_rec[c->host_slot] && drift_measured_at(c, leaf_id, c->host_frame))
        memcpy(&r, D.h_rec[c->host_slot] + D.src[(size_t)(1 + c->nodes[(size_t)leaf_id].d.parent_id)].slot, sizeof r);
    *out = r;
    return SDRX_OK;
}

int sdrx_get_drift_profile(sdrx_ctx *c, int leaf_id, double *profile, int64_t *frame)
{
    auto bad = [&](int) -> const char * {
        if (c->watch.leaf.empty() || !c->watch.leaf[(size_t)leaf_id].on)
            return "is not watched (sdrx_set_watch)";
        if (c->drift.src.empty() || c->drift.src[(size_t)(1 + c->nodes[(size_t)leaf_id].d.parent_id)].K == 0)
            return "its source has no drift estimate (sdrx_set_drift)";
        return nullptr;
    };
    if (int rc = leaf_call(c, "sdrx_get_drift_profile", &sdrx_ctx::opt_watch, "watch", &leaf_id, true, 1, kBetweenFrames, bad))
        return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    const sdrx_ctx::Drift::Src &S = c->drift.src[(size_t)(1 + c->nodes[(size_t)leaf_id].d.parent_id)];
    if (c->frame_no <= std::max(std::max(S.set_at, S.since), c->watch.leaf[(size_t)leaf_id].since))
        return fail(c, SDRX_ESTATE, "sdrx_get_drift_profile: no frame has been measured for the source of vfo %d yet", leaf_id);
    if (profile)
        HIPCHK(c, hipMemcpy(profile, reinterpret_cast<const unsigned char *>(S.d_state) + offsetof(DriftState, profile), sizeof(double) * (size_t)(2 * S.K + 1),
                            hipMemcpyDeviceToHost));
    if (frame)
        *frame = (int64_t)c->frame_no - 1;
    return SDRX_OK;
}

int sdrx_set_scan(sdrx_ctx *c, int leaf_id, const sdrx_scan_cfg *cfg)
{
    const bool on = cfg && cfg->cell_bins != 0;
    auto bad = [&](int) -> const char * {
        if (c->watch.leaf.empty() || !c->watch.leaf[(size_t)leaf_id].on)
            return "is not watched (sdrx_set_watch)";
        if (cfg && (cfg->reserved[0] || cfg->reserved[1] || cfg->reserved[2]))
            return "a reserved field is not 0";
        return on ? bad_scan(*cfg) : nullptr;
    };
    if (int rc = leaf_call(c, "sdrx_set_scan", &sdrx_ctx::opt_watch, "watch", &leaf_id, true, 1, kBetweenFrames, bad))
        return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c)) // frames inside the software pipeline finish with the old setting
        return rc;
    scan_host_init(c);
    sdrx_ctx::Scan &S = c->scan;
    sdrx_ctx::Scan::Src &R = S.src[(size_t)(1 + c->nodes[(size_t)leaf_id].d.parent_id)];
    if (!on && R.cfg.cell_bins == 0)
        return SDRX_OK;
    if (!S.d_src) {
        const size_t src_bytes = sizeof(ScanSrc) * (size_t)S.n_slots, rec_bytes = sizeof(ScanRecord) * (size_t)S.n_slots;
        HIPCHK(c, hipMalloc(&S.d_src, src_bytes));
        for (int p = 0; p < 2; ++p) {
            HIPCHK(c, hipMalloc(&S.d_rec[p], rec_bytes));
            HIPCHK(c, hipMemset(S.d_rec[p], 0, rec_bytes));
            HIPCHK(c, hipHostMalloc(&S.h_rec[p], rec_bytes, hipHostMallocDefault));
            memset(S.h_rec[p], 0, rec_bytes);
        }
        S.bytes += src_bytes + 2 * rec_bytes;
    }
    if (on) {
        if (!R.d_state) {
            HIPCHK(c, hipMalloc(&R.d_state, sizeof(ScanState)));
            HIPCHK(c, hipMemset(R.d_state, 0, sizeof(ScanState)));
            S.bytes += sizeof(ScanState);
        }
        // every accepted setting restarts the integration, and the last evaluation is no longer this setting's
        static_assert(offsetof(ScanState, valid) == offsetof(ScanState, count) + sizeof(unsigned), "count and valid are cleared together");
        HIPCHK(c, hipMemset(reinterpret_cast<unsigned char *>(R.d_state) + offsetof(ScanState, count), 0, 2 * sizeof(unsigned)));
    }
    const sdrx_ctx::Scan::Src before = R;
    const int w = on ? cfg->cell_bins : 0;
    if (R.cfg.cell_bins != w) {
        if (R.since != c->frame_no) // (as sdrx_set_watch: the frames before ran in the state they ran in)
            R.was_w = R.cfg.cell_bins;
        R.since = c->frame_no;
    }
    if (on)
        memcpy(&R.cfg, cfg, sizeof R.cfg);
    else
        R.cfg.cell_bins = 0;
    if (int rc = scan_rebuild(c, c->watch.src_ids, c->watch.src_psd)) {
        R = before;
        return rc;
    }
    return SDRX_OK;
}

int sdrx_get_scan(sdrx_ctx *c, int leaf_id, sdrx_scan_level *out)
{
    if (int rc = leaf_call(c, "sdrx_get_scan", &sdrx_ctx::opt_watch, "watch", &leaf_id, out != nullptr, 1, kDelivered))
        return rc;
    sdrx_scan_level r;
    memset(&r, 0, sizeof r);
    r.frame = (int64_t)c->host_frame;
    const sdrx_ctx::Scan &S = c->scan;
    if (S.h_rec[c->host_slot] && scan_measured_at(c, leaf_id, c->host_frame))
        memcpy(&r, S.h_rec[c->host_slot] + S.src[(size_t)(1 + c->nodes[(size_t)leaf_id].d.parent_id)].slot, sizeof r);
    *out = r;
    return SDRX_OK;
}

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
