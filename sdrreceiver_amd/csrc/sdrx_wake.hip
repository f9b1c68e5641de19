// sdrx_wake.hip -- host side of option "wake" (include/sdrx.h "Device-side wake", wake.hip): the one list of a
// leaf's flag words and state regions (leaf_regions: what sdrx_set_active fills between two frames and what k_watch_wake fills
// inside one), the device tables of the controlled leaves, and the ABI calls.  The launch sits in watch_launch_groups
// (sdrx_frame.hip), the records' way to the host in queue_watch, and what the host answers from them in leaf_parked_at
// (sdrx_delivery.hip).  A fragment of sdrx.hip's translation unit.

namespace {

// Every word that says whether leaf `id` runs, and every word that makes it a new vfo when it starts to:
//   emit(ptr, words, v_on, v_off, wake_only) -- `words` 32-bit words from `ptr` on become v_on when the leaf is unparked and,
//   unless wake_only, v_off when it is parked.
// The flag words in Park::d_act (K1, 2a, 2, 3, 4, 5, the gate) and the item_level[] words with kParkBit; then, wake_only, zeros over
// every filter-state region of both frame parities (whichever the next frame reads: the reference's zero-initialised filter
// state, dsp.cpp:40-49), the gate state of sdrx_finalize -- prev_open = `prev_open`: 1, or 0 for a leaf that is caught up -- and
// the AGC's quiet_run.  The oscillator's origin is not a fill: the caller writes K1Vfo::origin.
void leaf_regions(sdrx_ctx *c, int id, unsigned prev_open, const std::function<void(void *, size_t, unsigned, unsigned, bool)> &emit)
{
    sdrx_ctx::Park &K = c->park;
    const Node &nd = c->nodes[(size_t)id];
    auto put = [&](void *ptr, size_t words, unsigned v_on, unsigned v_off, bool wake_only) {
        if (words)
            emit(ptr, words, v_on, v_off, wake_only);
    };
    put(K.d_act + id, 1, 1, 0, false);
    for (int it : K.items[(size_t)id]) // (k_mix_levels / k_levels_tail: the flag rides in the item's level word)
        put(reinterpret_cast<int *>(c->arena + c->fp.off_item_level) + it, 1, (unsigned)nd.level, (unsigned)nd.level | (unsigned)kParkBit, false);
    if (nd.d2a_index >= 0)
        put(K.d_act + K.o_2a + nd.d2a_index, 1, 1, 0, false);
    if (nd.d2_index >= 0)
        put(K.d_act + K.o_2 + nd.d2_index, 1, 1, 0, false);
    if (nd.d3_index >= 0)
        put(K.d_act + K.o_3 + nd.d3_index, 1, 1, 0, false);
    if (nd.d4_index >= 0)
        put(K.d_act + K.o_4 + nd.d4_index, 1, 1, 0, false);
    if (nd.d5_index >= 0)
        put(K.d_act + K.o_5 + nd.d5_index, 1, 1, 0, false);
    const int sq = c->opt_squelch ? c->sq.index[(size_t)id] : -1; // (without the gate nothing reads its words)
    if (sq >= 0)
        put(K.d_act + K.o_sq + sq, 1, 1, 0, false);
    // the leaf starts as vfo::init leaves a new vfo: every history zero, in both parities
    const bool late = nd.d.demod_usb && nd.d.late_decimate > 0;
    const size_t hist = nd.fused_late == 5 ? (size_t)late_hist<5>() : nd.fused_late == 6 ? (size_t)late_hist<6>() : (size_t)std::max(1, nd.d.decimate_count * kHbHist);
    for (int p = 0; p < 2; ++p) {
        put(c->arena + nd.off_hb[p], 2 * hist, 0, 0, true);
        if (nd.fused_demod)
            put(c->arena + nd.off_dstate[p], 256, 0, 0, true);
        if (nd.has_stream)
            put(c->arena + nd.off_stream[p], 2 * (size_t)nd.Hx, 0, 0, true);
        if (late)
            put(c->arena + nd.off_z[p], 2 * (size_t)nd.H, 0, 0, true);
        if (nd.long_lpf)
            put(c->arena + nd.off_u[p], (size_t)nd.Hu, 0, 0, true);
        if (nd.detector == kDetFm) // z[-1] = 0 + 0j: the one place a detector leaf's start as a new vfo is defined (AM carries nothing)
            put(c->arena + nd.off_zprev[p], 2, 0, 0, true);
        if (nd.post_taps.size() > 1) // the post-detection filter's history = +0.0f: a new vfo's, defined here alone
            put(c->arena + nd.off_post_hist[p], nd.post_taps.size() - 1, 0, 0, true);
    }
    if (sq >= 0) { // the gate state of sdrx_finalize; thresholds, hang time, ratio and window stay
        put(c->sq.d_hang + sq, 1, 0, 0, true);
        if (c->opt_preroll)
            put(c->sq.d_prev + sq, 1, prev_open, 0, true);
        if (c->opt_squelch_auto) {
            put(c->sq.d_auto + sq, 4, 0xffffffffu, 0, true); // cur_min = prev_min = NONE
            put(reinterpret_cast<unsigned *>(c->sq.d_auto + sq) + 4, 1, 0, 0, true); // age
        }
    }
    if (c->opt_agc && c->agc.slot[(size_t)id] >= 0) // the gain stays what the device holds; the cold run starts again
        put(c->agc.d_quiet + c->agc.slot[(size_t)id], 1, 0, 0, true);
}

// The device tables for the present selection: the controlled leaves in the order of the watch's launch list, their sources in
// it, their settings and their fill lists.  Uploaded by sdrx_set_wake and whenever the watch's lists move (watch_rebuild: a
// retuned band, another selection).  Synchronous: never inside a frame call, and the context is drained.  Nothing before the
// first sdrx_set_wake that switched a leaf on.
int wake_rebuild(sdrx_ctx *c)
{
    sdrx_ctx::Wake &K = c->wake;
    if (!K.d_leaf)
        return SDRX_OK;
    const sdrx_ctx::Watch &W = c->watch;
    std::vector<int> id_of((size_t)W.n_slots, -1);
    for (size_t id = 0; id < c->nodes.size(); ++id)
        if (W.leaf[id].slot >= 0)
            id_of[(size_t)W.leaf[id].slot] = (int)id;
    std::vector<int> list;
    std::vector<WakeFill> fills;
    std::vector<int> begin((size_t)c->n_levels + 2, 0);
    K1Vfo *k1 = reinterpret_cast<K1Vfo *>(c->arena + c->off_k1vfo);
    for (int g = 0; g <= c->n_levels; ++g) {
        begin[(size_t)g] = (int)list.size();
        for (int k = W.leaf_begin[(size_t)g]; k < W.leaf_begin[(size_t)g + 1]; ++k) {
            const WatchLeaf &E = W.launch_leaves[(size_t)k];
            const int id = id_of[(size_t)E.slot];
            if (!K.controlled(id))
                continue;
            WakeLeaf &L = K.h_leaf[(size_t)E.slot];
            memset(&L, 0, sizeof L);
            memcpy(&L.cfg, &K.cfg[(size_t)id], sizeof L.cfg);
            L.vfo = k1 + id;
            L.src = E.src;
            L.fill_begin = (int)fills.size();
            leaf_regions(c, id, 1u, [&](void *ptr, size_t words, unsigned v_on, unsigned v_off, bool wake_only) {
                fills.push_back(WakeFill{static_cast<unsigned *>(ptr), (unsigned)words, v_on, v_off, wake_only ? 1u : 0u});
            });
            L.fill_n = (int)fills.size() - L.fill_begin;
            list.push_back(E.slot);
        }
    }
    begin[(size_t)c->n_levels + 1] = (int)list.size();
    HIPCHK(c, K.d_fill.reserve(fills.size()));
    if (!list.empty()) {
        HIPCHK(c, hipMemcpy(K.d_leaf, K.h_leaf.data(), sizeof(WakeLeaf) * K.h_leaf.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(K.d_fill, fills.data(), sizeof(WakeFill) * fills.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(K.d_list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice));
    }
    K.begin = begin;
    K.n_ctl = (int)list.size(); // (last: the frame sequence launches from these lists only when everything above succeeded)
    return SDRX_OK;
}

// first use on the device: the static table, the state and the records per watch slot, and the launch list
int wake_first_use(sdrx_ctx *c)
{
    sdrx_ctx::Wake &K = c->wake;
    const size_t slots = (size_t)c->watch.n_slots;
    HIPCHK(c, K.d_state.alloc(slots, true));
    HIPCHK(c, K.d_list.alloc(slots));
    HIPCHK(c, K.rec.alloc(sizeof(WakeRecord) * slots));
    HIPCHK(c, K.d_leaf.alloc(slots, true));
    return SDRX_OK;
}

// what is wrong with a setting for leaf `id` of context `m` (the table of include/sdrx.h, in its order)
const char *bad_wake(const sdrx_ctx *m, int id, const sdrx_wake_cfg &w)
{
    if (m->watch.leaf.empty() || !m->watch.leaf[(size_t)id].on.v)
        return "is not watched (sdrx_set_watch)";
    if (!m->spec.slots.empty() && m->spec.slots[(size_t)id].on)
        return "has an enabled spectrum (sdrx_set_spectrum)";
    if (w.on > 1)
        return "on must be 0 or 1";
    if (!std::isfinite(w.min_band_pwr) || !(w.min_band_pwr >= 0.0))
        return "min_band_pwr must be finite and not negative";
    if (w.reserved[0] || w.reserved[1] || w.reserved[2])
        return "a reserved field is not 0";
    return nullptr;
}
// ... with a call that a controlled leaf refuses
const char *bad_if_controlled(const sdrx_ctx *c, int id) { return c->wake.controlled(id) ? "is under the device's wake control (sdrx_set_wake)" : nullptr; }

} // namespace

extern "C" {

int sdrx_set_wake(sdrx_ctx *c, const int *ids, const sdrx_wake_cfg *cfgs, int n)
{
    if (int rc = leaf_call(c, "sdrx_set_wake", &sdrx_ctx::opt_wake, "wake", ids, cfgs != nullptr, n, kBetweenFrames, [&](int k) { return bad_wake(c, ids[k], cfgs[k]); }))
        return rc;
    if (n == 0)
        return SDRX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c)) // frames inside the software pipeline finish under the old settings
        return rc;
    sdrx_ctx::Wake &K = c->wake;
    const sdrx_ctx::Watch &W = c->watch;
    if (K.ctl.empty()) {
        K.ctl.assign(c->nodes.size(), sdrx_ctx::Switched());
        K.cfg.assign(c->nodes.size(), sdrx_wake_cfg{});
    }
    bool any_on = false;
    for (int k = 0; k < n; ++k)
        any_on |= cfgs[k].on != 0;
    if (!K.d_leaf && !any_on) { // nothing was ever switched on: nothing is allocated
        for (int k = 0; k < n; ++k)
            K.cfg[(size_t)ids[k]] = cfgs[k];
        return SDRX_OK;
    }
    if (!K.d_leaf) {
        if (int rc = wake_first_use(c)) { // all of it or none: the next call starts here again
            static_cast<sdrx_ctx::WakeDevice &>(K) = sdrx_ctx::WakeDevice();
            return rc;
        }
        K.h_leaf.assign((size_t)W.n_slots, WakeLeaf{});
    }
    // what the device holds for the leaves that are controlled already; then the named ones
    std::vector<WakeState> state((size_t)W.n_slots);
    HIPCHK(c, hipMemcpy(state.data(), K.d_state, sizeof(WakeState) * state.size(), hipMemcpyDeviceToHost));
    const std::vector<sdrx_ctx::Switched> ctl_before = K.ctl;
    const std::vector<sdrx_wake_cfg> cfg_before = K.cfg;
    const std::vector<sdrx_ctx::Park::Leaf> park_before = c->park.leaf;
    for (int k = 0; k < n; ++k) {
        const int id = ids[k];
        WakeState &S = state[(size_t)W.leaf[(size_t)id].slot];
        sdrx_ctx::Park::Leaf &P = c->park.leaf[(size_t)id];
        const bool was = K.ctl[(size_t)id].v != 0, now = cfgs[k].on != 0;
        if (was && !now) { // released: it stays in the state its last frame ran in
            if (S.active != P.active || (unsigned long long)S.since != P.since) {
                P.active = P.was_active = S.active; // (the frames before the release answer from their wake records)
                P.since = (unsigned long long)S.since;
            }
        } else if (now && !was) {
            S.active = P.active;
            S.since = (long long)P.since;
        }
        S.hold_left = 0;
        switch_to(K.ctl[(size_t)id], now ? 1 : 0, c->frame_no);
        K.cfg[(size_t)id] = cfgs[k];
    }
    int rc = hipMemcpy(K.d_state, state.data(), sizeof(WakeState) * state.size(), hipMemcpyHostToDevice) == hipSuccess
                 ? SDRX_OK
                 : fail(c, SDRX_EHIP, "sdrx_set_wake: the upload of the leaves' state failed");
    if (rc == SDRX_OK)
        rc = wake_rebuild(c);
    if (rc) { // (the launch list on the device is the old one -- n_ctl is set last --: so is the selection)
        K.ctl = ctl_before;
        K.cfg = cfg_before;
        c->park.leaf = park_before;
    }
    return rc;
}

int sdrx_get_wake(sdrx_ctx *c, const int *ids, int n, sdrx_wake_state *out)
{
    if (int rc = leaf_call(c, "sdrx_get_wake", &sdrx_ctx::opt_wake, "wake", ids, out != nullptr, n, kDelivered))
        return rc;
    for (int k = 0; k < n; ++k) {
        sdrx_wake_state s;
        memset(&s, 0, sizeof s);
        WakeRecord r;
        if (wake_record(c, ids[k], c->host_frame, &r)) {
            memcpy(&s, &r, sizeof s);
        } else {
            s.frame = (int64_t)c->host_frame;
            const sdrx_ctx::Park::Leaf &P = c->park.leaf[(size_t)ids[k]];
            s.active = !c->park.parked_at(ids[k], c->host_frame);
            s.since_frame = c->host_frame >= P.since ? (int64_t)P.since : 0;
        }
        out[k] = s;
    }
    return SDRX_OK;
}

} // extern "C"
