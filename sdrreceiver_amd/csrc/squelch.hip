// squelch.hip -- option "squelch": the per-leaf gate behind a frame's last payload-producing launch (included from sdrx.hip,
// launched by its frame sequence).  Two launches on one stream:
//
//   k_squelch_scan   ONE workgroup.  Per leaf, in publish order: fold sum_sq of its meter records (what sdrx_get_meters folds
//                    on the host), apply the rule
//                        s >= thr: open, hang_left = hang_frames | hang_left > 0: open, hang_left -= 1 | else closed
//                    on the per-leaf device state, and take the exclusive prefix sum of `open ? pay_len / 64 : 0` (payloads
//                    are padded to 64 bytes).  Integers only: exact and independent of any order.  Writes the directory
//                    {frame, n_open, packed_bytes | offset per leaf in 64-byte units, all ones = closed | hang_left per leaf}.
//   k_squelch_gather reads the directory (a launch later on the same stream: no inter-workgroup protocol) and copies the open
//                    leaves' payloads to their packed place, 16 bytes per lane and step.  The grid is sized for the worst
//                    case (every leaf open): workgroups of closed leaves, and of tiles behind a leaf's end, return at once.
//
// No atomics, no grid-wide barrier; plain vector loads and stores.
//
// Option "preroll"  launches the second form of both kernels (template parameter PRE, and what it needs
// besides in a trailing argument that is empty for the first form: the option off runs the kernels above as they were).
// One more bit of per-leaf state, prev_open (1 after finalize, then the previous gate's `open`):
//     pre = open && !prev_open;  prev_open = open
// A pre-rolled leaf takes 2 * pay_units in the prefix sum -- its payload of frame f-1 (still in the other parity of d_pay) at
// its offset, that of frame f directly behind -- and the directory gains pre[n] behind hang[n], the header the count of
// pre-rolled leaves.  The gather's grid gets a third dimension: z = 0 copies from d_pay[p] as before, z = 1 from d_pay[p ^ 1]
// and returns after one 4-byte load unless the leaf is pre-rolled.
//
// Option "squelch_auto"  launches k_squelch_scan with the template parameter AUTO (the gather is
// unchanged): the threshold follows the leaf's own noise floor, tracked by minimum statistics over a sliding window of frames.
// One 32-byte record per leaf (SqAuto: state and settings, two 16-byte loads issued with the pass's other loads, in front of
// the meter records -- no dependent step more).  With s the frame's sum_sq and NONE = 2^64 - 1 "no observation":
//     floor   = min(cur_min, prev_min)                                       (the frames BEFORE this one)
//     auto    = ratio_q8 == 0 || floor == NONE ? 0 : min(NONE, (floor * ratio_q8) >> 8)      (the product in 128 bits)
//     thr_eff = max(thr, auto);  the rule above with thr_eff in place of thr
//     cur_min = min(cur_min, s);  age += 1;  if (age == window_frames) { prev_min = cur_min; cur_min = NONE; age = 0; }
// and the directory gains thr_eff[n] and floor[n] (u64, 8-byte aligned) behind what it holds without: this frame's values.
//
// Option "park"  launches k_squelch_scan with the template parameter PARK and one word per leaf (ParkArg,
// sdrx_dev.h).  A parked leaf is closed whatever its threshold is (0 = "always open" holds for active leaves only), never
// pre-rolled, and the frame is no observation: hang_left, prev_open and the floor state stay as they are.  Its meter records
// are stale (nothing wrote them) and are not read into the decision.
#pragma once

namespace sdrx {

constexpr int kSqThreads = 1024;    // k_squelch_scan: 16 waves, passes of 1 024 consecutive leaves, one per lane
constexpr int kSqMaxLeaves = 65536; //   ... at most 64 passes
constexpr int kSqTile = 16384;      // k_squelch_gather: bytes per workgroup (256 lanes x 4 x 16 bytes)
constexpr unsigned kSqClosed = 0xffffffffu;

struct SqLeaf { // static, per leaf in publish order (byte offsets into d_pay[p]; every one a multiple of 16)
    unsigned pay_off, pay_units; // payload: offset, length in 64-byte units (padding included)
    unsigned meter_off, meter_n; // its MeterAcc records
};
struct SqCfg { // sdrx_set_squelch
    unsigned long long thr;
    unsigned hang_frames, pad;
};
struct SqHeader { // 64 bytes in front of the directory's per-leaf arrays
    long long frame;
    unsigned n_open, n_leaves;
    unsigned long long packed_bytes;
    unsigned long long pad[5]; // option preroll: pad[0] = pre-rolled leaves of this frame; zero otherwise
};
struct SqJob { // sdrx_set_squelch: leaf `index` (publish order) gets thr / hang_frames, its hang_left restarts at 0
    unsigned long long thr;
    unsigned hang_frames, index;
};

constexpr unsigned long long kSqNone = ~0ull; // option squelch_auto: no observation
struct SqAuto { // option squelch_auto: a leaf's floor state and settings, 32 bytes = two 16-byte loads
    unsigned long long cur_min, prev_min; // minimum of sum_sq in the running bucket / in the one before
    unsigned age;                         // frames in the running bucket
    unsigned ratio_q8, window_frames;     // sdrx_set_squelch_auto (ratio_q8 = 0: off for this leaf)
    unsigned pad;
};
struct SqAutoJob { // sdrx_set_squelch_auto: leaf `index` gets ratio_q8 / window_frames, its floor state restarts
    unsigned ratio_q8, window_frames, index, pad;
};
static_assert(sizeof(SqAuto) == 32 && sizeof(SqAutoJob) == sizeof(SqJob), "squelch_auto: record sizes");

template <bool PRE>
struct SqPre { // what the second form of the gate's kernels is given besides (option preroll); empty for the first
};
template <>
struct SqPre<true> {
    unsigned *prev_open;           // k_squelch_scan: per leaf, 1 = the previous gate left it open
    const unsigned char *pay_prev; // k_squelch_gather: d_pay[p ^ 1], the payloads of the frame before
};

template <bool AUTO>
struct SqAut { // what k_squelch_scan<.., AUTO> is given besides (option squelch_auto); empty without
};
template <>
struct SqAut<true> {
    SqAuto *state; // per leaf
};

__global__ __launch_bounds__(64) void k_squelch_set(const SqJob *__restrict__ jobs, int n, SqCfg *__restrict__ cfg, unsigned *__restrict__ hang_left)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= n)
        return;
    const SqJob J = jobs[j];
    SqCfg c;
    c.thr = J.thr;
    c.hang_frames = J.hang_frames;
    c.pad = 0;
    cfg[J.index] = c;
    hang_left[J.index] = 0;
}

__global__ __launch_bounds__(64) void k_squelch_set_auto(const SqAutoJob *__restrict__ jobs, int n, SqAuto *__restrict__ state)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= n)
        return;
    const SqAutoJob J = jobs[j];
    SqAuto a;
    a.cur_min = a.prev_min = kSqNone;
    a.age = 0;
    a.ratio_q8 = J.ratio_q8;
    a.window_frames = J.window_frames;
    a.pad = 0;
    state[J.index] = a;
}

// where thr_eff[n] | floor[n] begin in the directory (AUTO): behind hang[n] / pre[n], on 8 bytes
__host__ __device__ inline size_t sq_aux_off(size_t n, bool pre) { return (sizeof(SqHeader) + (pre ? 12 : 8) * n + 7) / 8 * 8; }

// dir: SqHeader | unsigned offs[n] | unsigned hang[n] | PRE: unsigned pre[n] | AUTO: u64 thr_eff[n] | u64 floor[n]
template <bool PRE = false, bool AUTO = false, bool PARK = false>
__global__ __launch_bounds__(kSqThreads) void k_squelch_scan(const SqLeaf *__restrict__ leaves, const SqCfg *__restrict__ cfg,
                                                             unsigned *__restrict__ hang_left, const unsigned char *__restrict__ pay,
                                                             unsigned char *__restrict__ dir, int n, long long frame, SqPre<PRE> X,
                                                             SqAut<AUTO> A, ParkArg<PARK> K)
{
    __shared__ unsigned s_units[kSqThreads / 64], s_open[kSqThreads / 64];
    __shared__ unsigned s_pre[PRE ? kSqThreads / 64 : 1]; // (PRE = false never touches it and the compiler drops it: 128 bytes
                                                          //   of LDS as before; a declaration cannot sit under `if constexpr`)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned *offs = reinterpret_cast<unsigned *>(dir + sizeof(SqHeader));
    unsigned *hang = offs + n;
    unsigned run_u = 0, run_o = 0; // units and open leaves of the passes so far (the same in every lane)
    unsigned run_p = 0;            // PRE: pre-rolled leaves
    for (int i0 = 0; i0 < n; i0 += kSqThreads) { // pass: leaves i0 .. i0 + 1023, leaf i0 + t in lane t (coalesced loads)
        const int i = i0 + t;
        unsigned units = 0, is_open = 0, pre = 0;
        if (i < n) {
            const SqLeaf L = leaves[i];
            const SqCfg C = cfg[i];
            bool parked = false;
            if constexpr (PARK)
                parked = K.act[i] == 0;
            uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0; // AUTO: the leaf's record, asked for HERE, with the loads above
            if constexpr (AUTO) {
                const uint4 *ap = reinterpret_cast<const uint4 *>(A.state + i);
                a0 = ap[0];
                a1 = ap[1];
            }
            unsigned long long s = 0;
            const uint4 *rec = reinterpret_cast<const uint4 *>(pay + L.meter_off);
            for (unsigned j = 0; j < L.meter_n; ++j) { // {sum_sq u64, clipped u32, peak u32}
                const uint4 r = rec[j];
                s += ((unsigned long long)r.y << 32) | r.x;
            }
            unsigned h = hang_left[i];
            unsigned long long thr = C.thr;
            if constexpr (AUTO) {
                unsigned long long cur = ((unsigned long long)a0.y << 32) | a0.x, prev = ((unsigned long long)a0.w << 32) | a0.z;
                unsigned age = a1.x;
                const unsigned long long ratio = a1.y, floor = min(cur, prev);
                if (ratio != 0 && floor != kSqNone) { // (floor * ratio) >> 8 in 128 bits, saturating
                    const unsigned long long lo = floor * ratio, hi = __umul64hi(floor, ratio);
                    thr = max(thr, (hi >> 8) ? kSqNone : ((hi << 56) | (lo >> 8)));
                }
                unsigned long long *aux = reinterpret_cast<unsigned long long *>(dir + sq_aux_off((size_t)n, PRE));
                aux[i] = thr;
                aux[n + i] = floor;
                cur = min(cur, s);
                age += 1;
                if (age == a1.z) {
                    prev = cur;
                    cur = kSqNone;
                    age = 0;
                }
                if (!parked) { // (a parked frame is not an observation of the floor)
                    uint4 *ap = reinterpret_cast<uint4 *>(A.state + i);
                    ap[0] = make_uint4((unsigned)cur, (unsigned)(cur >> 32), (unsigned)prev, (unsigned)(prev >> 32));
                    reinterpret_cast<unsigned *>(ap + 1)[0] = age;
                }
            }
            const unsigned h_was = h;
            is_open = 1;
            if (s >= thr)
                h = C.hang_frames;
            else if (h > 0)
                h -= 1;
            else
                is_open = 0;
            if (parked) { // closed, and the hang time does not run
                is_open = 0;
                h = h_was;
            }
            hang_left[i] = h;
            hang[i] = h;
            units = is_open ? L.pay_units : 0u;
            if constexpr (PRE) {
                if (!parked) {
                    pre = is_open & (X.prev_open[i] == 0u);
                    X.prev_open[i] = is_open;
                }
                hang[n + i] = pre; // (pre[] lies behind hang[])
                units += pre ? L.pay_units : 0u; // frame f-1's payload in front of frame f's
            }
        }
        // inclusive scan over the wave, the waves' totals through LDS
        unsigned su = units, so = is_open;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned u = __shfl_up(su, d, 64), o = __shfl_up(so, d, 64);
            if (lane >= d) {
                su += u;
                so += o;
            }
        }
        if (lane == 63) {
            s_units[wave] = su;
            s_open[wave] = so;
        }
        if constexpr (PRE) { // (only the total is wanted)
            const unsigned long long m = __ballot(pre != 0);
            if (lane == 0)
                s_pre[wave] = (unsigned)__popcll(m);
        }
        __syncthreads();
        unsigned base = run_u + su - units;
#pragma unroll
        for (int w = 0; w < kSqThreads / 64; ++w) {
            if (w < wave)
                base += s_units[w];
            run_u += s_units[w];
            run_o += s_open[w];
        }
        if constexpr (PRE) {
#pragma unroll
            for (int w = 0; w < kSqThreads / 64; ++w)
                run_p += s_pre[w];
        }
        if (i < n)
            offs[i] = is_open ? base : kSqClosed;
        __syncthreads(); // (the next pass overwrites the totals)
    }
    if (t == 0) {
        SqHeader H;
        H.frame = frame;
        H.n_open = run_o;
        H.n_leaves = (unsigned)n;
        H.packed_bytes = 64ull * run_u;
        for (int k = 0; k < 5; ++k)
            H.pad[k] = 0;
        if constexpr (PRE)
            H.pad[0] = run_p;
        *reinterpret_cast<SqHeader *>(dir) = H;
    }
}

// grid (n leaves, tiles of the longest payload[, PRE: source 0 = this frame's parity | 1 = the other one]), 256 lanes
template <bool PRE = false>
__global__ __launch_bounds__(256) void k_squelch_gather(const SqLeaf *__restrict__ leaves, const unsigned char *__restrict__ pay,
                                                        const unsigned char *__restrict__ dir, unsigned char *__restrict__ pack, SqPre<PRE> X)
{
    const int i = blockIdx.x;
    const unsigned *offs = reinterpret_cast<const unsigned *>(dir + sizeof(SqHeader));
    unsigned pre = 0;
    if constexpr (PRE) {
        pre = offs[2 * gridDim.x + i]; // (pre[] behind offs[] and hang[]: one entry per leaf = per blockIdx.x)
        if (blockIdx.z == 1 && pre == 0)
            return;
    }
    unsigned off = offs[i];
    if (off == kSqClosed)
        return;
    const SqLeaf L = leaves[i];
    const unsigned n16 = L.pay_units * 4u; // 16-byte units of this payload
    const unsigned tile = blockIdx.y * (unsigned)(kSqTile / 16);
    if (tile >= n16)
        return;
    if constexpr (PRE) {
        if (blockIdx.z == 1)
            pay = X.pay_prev; // the pre-rolled payload at the leaf's offset ...
        else if (pre)
            off += L.pay_units; // ... this frame's behind it
    }
    const uint4 *src = reinterpret_cast<const uint4 *>(pay + L.pay_off) + tile;
    uint4 *dst = reinterpret_cast<uint4 *>(pack + 64ull * off) + tile;
    const unsigned m = min(n16 - tile, (unsigned)(kSqTile / 16));
    for (unsigned k = threadIdx.x; k < m; k += 256)
        dst[k] = src[k];
}
} // namespace sdrx
