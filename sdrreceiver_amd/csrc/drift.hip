// drift.hip -- drift estimate (include/sdrx.h "Drift estimate"): the circular cross-correlation of a per-source
// template with the PSD the channel watch has just computed for that source (watch.hip), over the shifts -K .. K, and its first
// maximum -- the sensor of the loop sdrx_set_mixer_freqs closes for a dongle's frequency offset (included from sdrx.hip behind
// watch.hip, launched behind k_watch_bands).
//
//   profile[s] = sum over i of T[i] * PSD[(i + s) mod N]      s = -K .. K, N = 8192, IEEE double, FMA, parallel order
//   shift      = the first maximum of profile in the order 0, -1, +1, -2, +2, ...
#pragma once

namespace sdrx {

constexpr int kDriftMaxShift = 1024;                   // SDRX_DRIFT_MAX_SHIFT
constexpr int kDriftBlock = 16;                        // shifts per workgroup (a workgroup walks its shifts one after the other: the launch is as long as one block)
constexpr int kDriftPerThread = kSpecN / kSpecThreads; // template entries a thread keeps in registers
constexpr int kDriftMaxBlocks = (2 * kDriftMaxShift + 1 + kDriftBlock - 1) / kDriftBlock;

struct DriftRecord { // = sdrx_drift_level (include/sdrx.h)
    long long frame;
    double peak, left, right, zero;
    int shift, max_shift, measured, captured;
    int reserved[2];
};

struct DriftState { // what a source keeps on the device from its first sdrx_set_drift on: one allocation that never moves
    double templ[kSpecN];
    double profile[2 * kDriftMaxShift + 1]; // of the last measured frame: [s + K]
    unsigned done;                          // shift blocks of this launch that have written their part (back to 0 behind the last)
    unsigned capture;                       // 1: the next measured frame's PSD becomes the template (back to 0 behind it)
};
struct DriftSrc {
    const double *psd; // the watch's PSD of the source (WatchSrc::psd)
    DriftState *state;
    int K, n_blocks; // max_shift; ceil((2K + 1) / kDriftBlock)
    int level, slot; // tree level of the stream's VFO, -1: the raw frame; its record
};
struct DriftBlk { // one workgroup of k_watch_drift
    int src, blk;
};

// the better of two candidates of the argmax: the larger value, the earlier rank among equal ones
__device__ __forceinline__ void drift_better(double &v, int &r, double v2, int r2)
{
    if (v2 > v || (v2 == v && r2 < r)) {
        v = v2;
        r = r2;
    }
}
// rank in the order 0, -1, +1, -2, +2, ... -> shift
__device__ __forceinline__ int drift_rank_shift(int r) { return r & 1 ? -((r + 1) >> 1) : r >> 1; }

// One workgroup per (source with a template, block of kDriftBlock = 16 shifts).  The PSD lies in LDS as doubles (64 KiB, what
// k_watch_psd's F takes); thread t keeps T[t + 512 k], k < 16, in registers and reads PSD[(t + 512 k + s) mod N] for every shift
// of its block: consecutive lanes, consecutive doubles.  Per shift a wave reduction; the eight wave sums meet in LDS behind the
// loop.  The workgroup that completes a source's last block -- the counter and fences of k_watch_psd -- takes the argmax and
// writes the record to the fixed part of the frame the source stream holds (as k_watch_bands does).
// Capture: every workgroup takes the PSD itself for T (no workgroup of this launch reads state->templ then), block 0 stores it.
__global__ __launch_bounds__(kSpecThreads) void k_watch_drift(const DriftSrc *__restrict__ srcs, const DriftBlk *__restrict__ blks, WatchArgs A,
                                                              DriftRecord *__restrict__ rec0, DriftRecord *__restrict__ rec1)
{
    __shared__ double X[kSpecN];
    __shared__ double part[kSpecThreads / 64][kDriftBlock];
    __shared__ int part_rank[kSpecThreads / 64];
    __shared__ int last;
    const DriftBlk G = blks[blockIdx.x];
    const DriftSrc &D = srcs[G.src];
    DriftState *st = D.state;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = D.K, n_shifts = 2 * K + 1;
    const bool capture = st->capture != 0u;
    const double *psd = D.psd;
    double t[kDriftPerThread];
#pragma unroll
    for (int k = 0; k < kDriftPerThread; ++k) {
        const int i = tid + k * kSpecThreads;
        const double x = psd[i];
        X[i] = x;
        t[k] = capture ? x : st->templ[i];
    }
    if (capture && G.blk == 0) {
#pragma unroll
        for (int k = 0; k < kDriftPerThread; ++k)
            st->templ[tid + k * kSpecThreads] = t[k];
    }
    __syncthreads();
    const int first = G.blk * kDriftBlock; // index into profile: shift = index - K
    const int n_here = n_shifts - first < kDriftBlock ? n_shifts - first : kDriftBlock;
    for (int j = 0; j < n_here; ++j) {
        const int base = tid + first + j - K + kSpecN; // > 0: K <= 1024
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < kDriftPerThread; ++k)
            acc = fma(t[k], X[(base + k * kSpecThreads) & (kSpecN - 1)], acc);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            acc += __shfl_xor(acc, off);
        if (lane == 0)
            part[wave][j] = acc;
    }
    __syncthreads();
    if (tid < n_here) {
        double sum = part[0][tid];
#pragma unroll
        for (int w = 1; w < kSpecThreads / 64; ++w)
            sum += part[w][tid];
        st->profile[first + tid] = sum;
    }
    __threadfence();
    __syncthreads();
    if (tid == 0)
        last = atomicAdd(&st->done, 1u) == (unsigned)(D.n_blocks - 1);
    __syncthreads();
    if (!last)
        return;
    __threadfence();
    // the whole profile is there: into LDS (nobody reads X any more), then the first maximum in the defined order
    for (int i = tid; i < n_shifts; i += kSpecThreads)
        X[i] = st->profile[i];
    __syncthreads();
    double best = X[K];
    int rank = 0;
    for (int r = tid; r < n_shifts; r += kSpecThreads) // (ascending ranks: > keeps the first)
        drift_better(best, rank, X[K + drift_rank_shift(r)], r);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double v2 = __shfl_xor(best, off);
        const int r2 = __shfl_xor(rank, off);
        drift_better(best, rank, v2, r2);
    }
    if (lane == 0) {
        part[wave][0] = best;
        part_rank[wave] = rank;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kSpecThreads / 64; ++w)
            drift_better(best, rank, part[w][0], part_rank[w]);
        const int s = drift_rank_shift(rank);
        const unsigned long long frame = D.level < 0 ? A.frame_raw : spec_level_frame(A.frame_level, D.level);
        DriftRecord r;
        r.frame = (long long)frame;
        r.peak = X[K + s];
        r.left = s - 1 >= -K ? X[K + s - 1] : 0.0;
        r.right = s + 1 <= K ? X[K + s + 1] : 0.0;
        r.zero = X[K];
        r.shift = s;
        r.max_shift = K;
        r.measured = 1;
        r.captured = capture ? 1 : 0;
        r.reserved[0] = r.reserved[1] = 0;
        (frame & 1ull ? rec1 : rec0)[D.slot] = r;
        st->capture = 0u; // (every workgroup of this launch has read it: all of them have counted)
        st->done = 0u;    // (the next launch on this source is behind this one in stream order)
    }
}

} // namespace sdrx
