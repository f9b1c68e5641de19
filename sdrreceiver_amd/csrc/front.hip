// front.hip -- k_front_halfband<MODE>: the half-band front stage between the ingest kernels and the resampler, or level 0 where
// none is set (include/sdrx.h "Front stage").  One launch per stage; every stage halves the rate with the one
// prototype h[0 .. N-1], N = 4 K + 3, centre C = 2 K + 1, whose odd taps other than C are zero:
//   y[m] = sum over the non-zero k, ascending (0, 2, .. 2K, 2K+1, 2K+2, .. 4K+2), of fl(h[k] * z[2m - k])
// -- acc = fl(acc + fl(h z)) from +0.0f, two roundings per tap (-ffp-contract=off: v_mul_f32, v_add_f32), the same in every
// arithmetic.  z[n] for n < 0 is the previous frame's z[n_in + n]: an N-1 sample history per stage in a two-slot parity buffer.
//   MODE kFrontComplex: z is a cf32 frame in tile layout -- what the ingest kernels or the stage in front wrote.
//   MODE kFrontRS16 / kFrontRU12 (stage 1 of a real front end): z[n] = r[n] (-j)^n with r the converted real sample, read
//   straight from the 16-bit words; the products with a structurally zero component are not formed -- I sums the even k only,
//   Q is the single product fl(h[C] * Im z[2m - C]).  The history holds r.
//
// One workgroup of 256 threads per tile of 1024 outputs.  The tile's window (front_window, sdrx_front.h: 2 * 1024 + N - 1 inputs
// at most) is staged into LDS as its even and its odd positions -- N - 1 is even, so the even taps of output j read
// E[j + 2K+1 - i], the lanes of a wave consecutive slots (a 256-byte bank row per 32 lanes of cf32), and the centre tap O[j + K].
// Thread t owns outputs t, t + 256, t + 512, t + 768 of the tile.  The taps are wave-uniform: at most 65 floats, read through a
// pointer into the constant address space with a uniform index (scalar loads).  The results leave through the padded LDS tile of
// resample.hip as full 1 KiB rows of the tile layout; a short last tile (a multiple of 16) masks whole lanes.
// Relies on tile_index / tile_unit (sdrx_dev.h), rs_tile_pos / kRsTileF2 (resample.hip) and sdrx_front.h.

constexpr int kFrontComplex = 0, kFrontRS16 = 1, kFrontRU12 = 2;

struct FrontArgs {
    const void *in;                 // complex: float2, tile layout; real: the frame's 16-bit words in natural order
    const void *hist_prev;          // z[-(N-1)] .. z[-1] of this frame (float2) or r[..] (float): what the previous frame left
    void *hist_next;                // the same for the next frame: the last tile's workgroup writes it
    const float *taps;              // h[0], h[2], .. h[4K+2] (2K+2 floats), then h[C]
    float4 *out;                    // the stage's output frame, tile layout
    int n_in, n_out;                // n_in = 2 n_out
    int K;
};

template <int MODE>
__device__ __forceinline__ auto front_load(const void *in, int idx)
{
    if constexpr (MODE == kFrontComplex) {
        return static_cast<const float2 *>(in)[tile_index<size_t>(idx)];
    } else {
        const unsigned v = static_cast<const unsigned short *>(in)[idx];
        if constexpr (MODE == kFrontRS16)
            return (float)(short)v * 0.00390625f;
        else
            return (float)((int)(v & 4095u) - 2048) * 0.0625f;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_front_halfband(const FrontArgs A)
{
    using T = std::conditional_t<MODE == kFrontComplex, float2, float>;
    __shared__ __attribute__((aligned(16))) float2 tile[kRsTileF2];
    __shared__ __attribute__((aligned(16))) T win_e[kFrWinHalf];
    __shared__ __attribute__((aligned(16))) T win_o[kFrWinHalf];
    const int c = blockIdx.x, t = threadIdx.x;
    const int K = A.K, n1 = 4 * K + 2;                        // N - 1
    const int count = min(kFrTile, A.n_out - c * kFrTile);    // a multiple of 16
    const int lo = 2 * kFrTile * c - n1;                      // front_window
    const int W = 2 * count + n1 - 1;                         // hi - lo + 1 <= kFrMaxWindow; hi < n_in
    const T *hp = static_cast<const T *>(A.hist_prev);
    for (int w = t; w < W; w += 256) {
        const int idx = lo + w;
        const T v = idx < 0 ? hp[n1 + idx] : front_load<MODE>(A.in, idx);
        if (w & 1)
            win_o[w >> 1] = v;
        else
            win_e[w >> 1] = v;
    }
    if (c == (int)gridDim.x - 1 && t < n1) // (n_in >= N - 1: all of it lies in this frame)
        static_cast<T *>(A.hist_next)[t] = front_load<MODE>(A.in, A.n_in - n1 + t);
    __syncthreads();
    // (the constant address space: with the loop counter as the index the compiler selects scalar loads, one per wave and tap)
    const __attribute__((address_space(4))) float *taps = (const __attribute__((address_space(4))) float *)A.taps;
    const float hc = taps[2 * K + 2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = t + 256 * q;
        if (j >= count)
            break;
        const int e0 = j + 2 * K + 1; // front_even_slot(j, 0, K)
        if constexpr (MODE == kFrontComplex) {
            float re = 0.0f, im = 0.0f;
            for (int i = 0; i <= K; ++i) {
                const float h = taps[i];
                const float2 x = win_e[e0 - i];
                re = re + h * x.x, im = im + h * x.y;
            }
            {
                const float2 x = win_o[j + K];
                re = re + hc * x.x, im = im + hc * x.y;
            }
            for (int i = K + 1; i <= 2 * K + 1; ++i) {
                const float h = taps[i];
                const float2 x = win_e[e0 - i];
                re = re + h * x.x, im = im + h * x.y;
            }
            tile[rs_tile_pos(j)] = make_float2(re, im);
        } else {
            // the absolute index of window position w is 2 (mod 4) + w: an even slot e holds n = 2 e + 2 -- Re z = +r where e is
            // odd, -r where it is even --, an odd slot o holds n = 2 o + 3 -- Im z = +r where o is even, -r where it is odd
            float re = 0.0f;
            for (int i = 0; i <= 2 * K + 1; ++i) {
                const int e = e0 - i;
                const float r = win_e[e];
                re = re + taps[i] * ((e & 1) ? r : -r);
            }
            const int o = j + K;
            const float r = win_o[o];
            tile[rs_tile_pos(j)] = make_float2(re, hc * ((o & 1) ? -r : r));
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int u = t + 256 * q, i2 = u >> 6, ln = u & 63; // unit (i2, ln) of the tile: samples 16 ln + 2 i2 and + 1
        if (ln * 16 < count)
            A.out[tile_unit(c, i2, ln)] = *reinterpret_cast<const float4 *>(tile + rs_tile_pos(ln * 16 + 2 * i2));
    }
}
