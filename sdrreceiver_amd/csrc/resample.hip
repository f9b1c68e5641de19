// resample.hip -- k_resample: the polyphase rational resampler L/M between the ingest kernels and level 0 (include/sdrx.h
// "Resampler").  The ingest family leaves the frame at the INPUT rate in a staging buffer in tile layout; this
// kernel writes the tree's raw frame, d_raw_tiled, from it:
//   y[m] = sum over t = 0 .. T-1, ascending, of fl(h[ph + t L] * x[i - t]),  p = m M, i = p div L, ph = p mod L
// -- acc = fl(acc + fl(h x)) from +0.0f, two roundings per tap (-ffp-contract=off: v_mul_f32, v_add_f32), the same in every
// arithmetic.  x[j] for j < 0 is the previous frame's x[n_in + j]: a T-1 sample history in a two-slot parity buffer.
//
// One workgroup of 256 threads per chunk of 1024 outputs = one tile.  The chunk's input window (resample_window,
// sdrx_resample.h: at most 4 * 1023 + T samples) is staged into LDS in natural order -- read through tile_index, and from the
// history for negative indices --; thread t owns outputs t, t + 256, t + 512, t + 768 of the chunk, so the lanes of a wave
// read consecutive windows (M / L <= 4 samples apart).  The taps are read as float4s from the phase-major table g[ph][t] =
// h[ph + t L] (at most 128 KiB: L1 / L2).  The results go through an LDS tile (16 bytes of padding per 16 samples: a lane's
// float4 of the tile layout is 144 bytes from its neighbour's, 16 distinct slots per 16 lanes), so that every wave store is
// a full 1 KiB row of the tile layout.
// Relies on tile_index / tile_unit (sdrx_dev.h) and sdrx_resample.h.

struct ResampleArgs {
    const float2 *stage;     // the frame at the input rate, tile layout
    const float2 *hist_prev; // x[-(T-1)] .. x[-1] of this frame: what the previous frame left (zeros at finalize)
    float2 *hist_next;       // the same for the next frame: the last chunk's workgroup writes it
    const float4 *taps;      // g[ph][t], T / 4 float4s per phase
    float4 *out;             // the tree's raw frame, tile layout
    int n_in, n_out;
    int L, M, T;
};

constexpr int kRsTileF2 = kRsChunk + 2 * (kRsChunk / 16); // the output tile in LDS: 2 cf32 of padding per 16 samples
__host__ __device__ constexpr int rs_tile_pos(int j) { return j + 2 * (j >> 4); }
inline int resample_lds_bytes(int max_window) { return (int)(sizeof(float2) * (size_t)(kRsTileF2 + ((max_window + 1) & ~1))); }

__global__ __launch_bounds__(256) void k_resample(const ResampleArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *tile = reinterpret_cast<float2 *>(smem);
    float2 *win = tile + kRsTileF2;
    const int c = blockIdx.x, t = threadIdx.x;
    const int count = min(kRsChunk, A.n_out - c * kRsChunk); // a multiple of 16
    // positions in 64 bits for the chunk's first output only: p = p0 + j M with j < 1024 and r0 + j M < 2^23 from there
    const long long p0 = (long long)c * kRsChunk * A.M;
    const long long i0 = p0 / A.L;
    const unsigned r0 = (unsigned)(p0 - i0 * A.L);
    const int lo = (int)i0 - (A.T - 1);                                            // resample_window
    const int W = (int)((r0 + (unsigned)(count - 1) * (unsigned)A.M) / (unsigned)A.L) + A.T; // hi - lo + 1; hi < n_in
    for (int w = t; w < W; w += 256) {
        const int idx = lo + w;
        win[w] = idx < 0 ? A.hist_prev[A.T - 1 + idx] : A.stage[tile_index<size_t>(idx)];
    }
    if (c == (int)gridDim.x - 1 && t < A.T - 1) // (n_in >= T: all of it lies in this frame)
        A.hist_next[t] = A.stage[tile_index<size_t>(A.n_in - (A.T - 1) + t)];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = t + 256 * k;
        if (j >= count)
            break;
        const unsigned q = r0 + (unsigned)j * (unsigned)A.M;
        const unsigned irel = q / (unsigned)A.L, ph = q - irel * (unsigned)A.L;
        const float4 *g = A.taps + (size_t)ph * (size_t)(A.T >> 2);
        const float2 *x = win + irel + (A.T - 1); // x[i]: x[i - t] = x[-t]
        float re = 0.0f, im = 0.0f;
        for (int tt = 0; tt < A.T; tt += 4) {
            const float4 h = g[tt >> 2];
            const float2 x0 = x[-tt], x1 = x[-tt - 1], x2 = x[-tt - 2], x3 = x[-tt - 3];
            re = re + h.x * x0.x, im = im + h.x * x0.y;
            re = re + h.y * x1.x, im = im + h.y * x1.y;
            re = re + h.z * x2.x, im = im + h.z * x2.y;
            re = re + h.w * x3.x, im = im + h.w * x3.y;
        }
        tile[rs_tile_pos(j)] = make_float2(re, im);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int u = t + 256 * k, i2 = u >> 6, ln = u & 63; // unit (i2, ln) of the tile: samples 16 ln + 2 i2 and + 1
        if (ln * 16 < count)
            A.out[tile_unit(c, i2, ln)] = *reinterpret_cast<const float4 *>(tile + rs_tile_pos(ln * 16 + 2 * i2));
    }
}
