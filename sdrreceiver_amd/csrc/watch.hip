// watch.hip -- channel watch (option "watch", include/sdrx.h): the power inside a leaf's passband, measured on
// the stream the leaf is FED -- its parent's decimate[d], or the raw frame -- so that a parked leaf can be watched at the
// price of one power spectrum per source stream, shared by all its children (included from sdrx.hip, launched by its frame
// sequence where the spectrum display is).
//
// Per measured source and frame (n samples, N = 8192): S = min(max(n / N, 1), 16) segments, segment s from sample s * (n / S),
// min(N, n) samples each, zero-padded;  Hann window and kiss_fft exactly as k_spectrum (spec_fft);
//   P_s[i] = fl(fl(im*im) + fl(re*re))     fp32, the expression under k_spectrum's sqrtf (the library is built without contraction)
//   PSD[i] = sum over s, ascending, of (double)P_s[i]
// Per watched leaf: band_pwr = sum of PSD over its n_bins bins from first_bin (mod N), total_pwr = sum of PSD.
#pragma once

namespace sdrx {

constexpr int kWatchMaxSeg = 16;     // SDRX_WATCH_MAX_SEGMENTS
constexpr int kWatchLeafThreads = 256; // k_watch_bands: one wave per leaf, four leaves per workgroup

struct WatchRecord { // = sdrx_watch_level (include/sdrx.h)
    long long frame;
    double band_pwr, total_pwr;
    int first_bin, n_bins, segments, watched;
    int reserved[2];
};

struct WatchSrc {
    const float2 *src[2]; // the stream per frame parity (a parent's decimate[d], tile layout); the raw frame: WatchArgs::raw
    float *P;             // S x kSpecN: P_s of this frame
    double *psd;          // kSpecN doubles, then total_pwr
    unsigned *done;       // segments of this frame that have written their P_s (the last one sums; back to 0 behind it)
    int n, S, level, pad; // samples per frame; segments; tree level of the stream's VFO, -1: the raw frame
};
struct WatchSeg { // one workgroup of k_watch_psd
    int src, seg;
};
struct WatchLeaf { // one wave of k_watch_bands
    int src, first_bin, n_bins, slot;
};
struct WatchArgs {
    unsigned long long frame_level[kMaxLevels]; // the frame each tree level's streams hold in this launch
    unsigned long long frame_raw;               // ... and the frame `raw` is
    const void *raw;
    int raw_mode; // kRawF32 | kRawTiled | kRawU8
};

// One workgroup per (measured source, segment).  The workgroup that completes a source's last segment adds the segments up in
// ascending order -- every other one has published its P_s by then: a release fence in front of its count, an acquire fence
// behind the last count.
__global__ __launch_bounds__(kSpecThreads) void k_watch_psd(const WatchSrc *__restrict__ srcs, const WatchSeg *__restrict__ segs, WatchArgs A,
                                                            const float2 *__restrict__ tw, const float *__restrict__ hann)
{
    __shared__ float2 F[kSpecN];
    __shared__ double red_sum[kSpecThreads / 64];
    __shared__ int last;
    const WatchSeg G = segs[blockIdx.x];
    const WatchSrc &D = srcs[G.src];
    const int tid = threadIdx.x;
    SpecSource S;
    if (D.level < 0) {
        S = spec_raw_source(A.raw, A.raw_mode);
    } else {
        S.src = D.src[spec_level_frame(A.frame_level, D.level) & 1ull];
        S.tiled = true;
    }
    const int n_in = D.n < kSpecN ? D.n : kSpecN, n_seg = D.S;
    const int start = G.seg * (D.n / n_seg); // start + n_in <= n: n / S >= N whenever n >= N
    spec_fft(
        F,
        [&](int a) -> float2 {
            if (a >= n_in)
                return make_float2(0.f, 0.f);
            const float2 x = spec_sample(S, start + a);
            const float h = hann[a];
            return make_float2(x.x * h, x.y * h);
        },
        tw, tid);
    float *P = D.P + (size_t)G.seg * kSpecN;
    for (int i = tid; i < kSpecN; i += kSpecThreads) {
        const float2 o = F[i];
        P[i] = o.y * o.y + o.x * o.x;
    }
    __threadfence();
    __syncthreads();
    if (tid == 0)
        last = atomicAdd(D.done, 1u) == (unsigned)(n_seg - 1);
    __syncthreads();
    if (!last)
        return;
    __threadfence();
    const float *P0 = D.P;
    double *psd = D.psd;
    double sum = 0.0;
    for (int i = tid; i < kSpecN; i += kSpecThreads) {
        double acc = (double)P0[i];
        for (int s = 1; s < n_seg; ++s)
            acc += (double)P0[(size_t)s * kSpecN + i];
        psd[i] = acc;
        sum += acc;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        sum += __shfl_xor(sum, off);
    if ((tid & 63) == 0)
        red_sum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        sum = red_sum[0];
        for (int w = 1; w < kSpecThreads / 64; ++w)
            sum += red_sum[w];
        psd[kSpecN] = sum;
        *D.done = 0u; // (the next launch on this source is behind this one in stream order)
    }
}

// One wave per watched leaf: lanes stride over the band; the record goes to the fixed part of the frame its source stream holds.
__global__ __launch_bounds__(kWatchLeafThreads) void k_watch_bands(const WatchSrc *__restrict__ srcs, const WatchLeaf *__restrict__ leaves, int n_leaves,
                                                                   WatchArgs A, WatchRecord *__restrict__ rec0, WatchRecord *__restrict__ rec1)
{
    const int w = blockIdx.x * (kWatchLeafThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= n_leaves)
        return;
    const WatchLeaf L = leaves[w];
    const WatchSrc &D = srcs[L.src];
    const unsigned long long frame = D.level < 0 ? A.frame_raw : spec_level_frame(A.frame_level, D.level);
    const double *psd = D.psd;
    double acc = 0.0;
    for (int j = lane; j < L.n_bins; j += 64)
        acc += psd[(L.first_bin + j) & (kSpecN - 1)];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        acc += __shfl_xor(acc, off);
    if (lane == 0) {
        WatchRecord r;
        r.frame = (long long)frame;
        r.band_pwr = acc;
        r.total_pwr = psd[kSpecN];
        r.first_bin = L.first_bin;
        r.n_bins = L.n_bins;
        r.segments = D.S;
        r.watched = 1;
        r.reserved[0] = r.reserved[1] = 0;
        (frame & 1ull ? rec1 : rec0)[L.slot] = r;
    }
}

} // namespace sdrx
