// wake.hip -- device-side wake (option "wake", include/sdrx.h "Device-side wake"): behind k_watch_bands, one
// workgroup per leaf under the device's control decides from the leaf's watch record of frame f whether the leaf runs in frame
// f, and on a change of state writes what sdrx_set_active writes between two frames -- the flag words, and for a leaf that
// wakes zeros over its state regions, the gate state of sdrx_finalize and the oscillator's origin -- with plain vector stores.
// No atomics, no protocol between workgroups: a leaf's words belong to its workgroup, and every launch that reads them is
// behind this one in stream order (the argument above enqueue_frame, sdrx_frame.hip).  Included from sdrx.hip behind watch.hip.
#pragma once

namespace sdrx {

constexpr int kWakeThreads = 256;

struct WakeCfg { // = sdrx_wake_cfg (include/sdrx.h)
    double min_band_pwr;
    unsigned contrast_q8, hold_frames, on;
    unsigned reserved[3];
};
struct WakeRecord { // = sdrx_wake_state
    long long frame, since_frame;
    int active, hot;
    unsigned hold_left;
    int controlled;
};
// What a leaf carries from frame to frame: written by its workgroup alone (and by sdrx_set_wake, between frames).
struct WakeState {
    long long since; // first frame of the present state
    int active;
    unsigned hold_left;
};
// One entry of a leaf's fill list: `words` 32-bit words from `ptr` on become v_on when the leaf wakes, and -- the flag words
// only (wake_only 0) -- v_off when it parks.
struct WakeFill {
    unsigned *ptr;
    unsigned words, v_on, v_off, wake_only;
};
static_assert(sizeof(WakeFill) == 24, "WakeFill array stride");
struct WakeLeaf { // per watch slot; what sdrx_set_wake and the watch's launch lists say about a controlled leaf
    WakeCfg cfg;
    K1Vfo *vfo;   // its oscillator's origin becomes the frame it wakes in
    int src;      // its source in the watch's launch list (WatchSrc)
    int fill_begin, fill_n;
    int pad_;
};

// The rule of include/sdrx.h on one watch record.  -ffp-contract=off: every operation below rounds once.
__device__ __forceinline__ bool wake_hot(const WakeCfg &C, double b, double t, int n)
{
    bool c_ok = C.contrast_q8 == 0;
    if (!c_ok && n < kSpecN) {
        const double lhs = b * (double)(256 * (kSpecN - n));
        const double rhs = (t - b) * (double)((unsigned long long)C.contrast_q8 * (unsigned long long)n);
        c_ok = lhs >= rhs;
    }
    return b >= C.min_band_pwr && c_ok;
}

// One workgroup per controlled leaf of the source groups k_watch_bands has just measured (`list`: their watch slots).
__global__ __launch_bounds__(kWakeThreads) void k_watch_wake(const WatchSrc *__restrict__ srcs, const WakeLeaf *__restrict__ leaves, WakeState *__restrict__ state,
                                                             const int *__restrict__ list, const WakeFill *__restrict__ fills, WatchArgs A,
                                                             const WatchRecord *__restrict__ wrec0, const WatchRecord *__restrict__ wrec1,
                                                             WakeRecord *__restrict__ rec0, WakeRecord *__restrict__ rec1)
{
    __shared__ int transition; // 0: none; 1: the leaf wakes; 2: it parks
    const int slot = list[blockIdx.x];
    const WakeLeaf &L = leaves[slot];
    const WatchSrc &D = srcs[L.src];
    const unsigned long long frame = D.level < 0 ? A.frame_raw : spec_level_frame(A.frame_level, D.level);
    if (threadIdx.x == 0) {
        const WatchRecord &w = (frame & 1ull ? wrec1 : wrec0)[slot];
        WakeState S = state[slot];
        const bool hot = wake_hot(L.cfg, w.band_pwr, w.total_pwr, w.n_bins);
        int active = 1;
        if (hot)
            S.hold_left = L.cfg.hold_frames;
        else if (S.hold_left > 0)
            S.hold_left -= 1;
        else
            active = 0;
        const int tr = active == S.active ? 0 : active ? 1 : 2;
        if (tr)
            S.since = (long long)frame;
        S.active = active;
        state[slot] = S;
        WakeRecord r;
        r.frame = (long long)frame;
        r.since_frame = S.since;
        r.active = active;
        r.hot = hot ? 1 : 0;
        r.hold_left = S.hold_left;
        r.controlled = 1;
        (frame & 1ull ? rec1 : rec0)[slot] = r;
        if (tr == 1)
            L.vfo->origin = frame; // a fresh Oscillator from sample 0 of this frame (the checkpoints stand: same frequency)
        transition = tr;
    }
    __syncthreads();
    const int tr = transition;
    if (tr == 0)
        return;
    for (int k = 0; k < L.fill_n; ++k) {
        const WakeFill F = fills[L.fill_begin + k];
        if (tr == 2 && F.wake_only)
            continue;
        const unsigned v = tr == 1 ? F.v_on : F.v_off;
        for (unsigned i = threadIdx.x; i < F.words; i += kWakeThreads)
            F.ptr[i] = v;
    }
}

} // namespace sdrx
