// spectrum.hip -- the spectrum display of MainWindow::fftHandlerSlot (mainwindow.cpp:411-478) on the device, batched: one
// workgroup per spectrum that is due this frame (included from sdrx.hip, launched by its frame sequence).
//
// Per update, for a stream x of n_in = min(len, 8192) samples (a shorter stream is zero-padded: every state is fed by one
// stream of constant length and starts zeroed, so the reference's stale `inr` tail is always zero):
//   inr[a] = x[a] * hann[a]                                   complex<float> * float           (mainwindow.cpp:418-425)
//   out    = kiss_fft(inr), nfft = 8192 = 4^6 * 2             kf_work's decimation in time: kf_bfly2, then six kf_bfly4
//   pwr[(i + N/2) mod N] = pwr*0.95 + 0.05*10*log10(fmax(100000.0*abs((1.0/N)*val), 1)),  val = (double)sqrtf(im*im + re*re)
//   maxval / aveval of pwr, then the "< 10 dB" rule                                            (mainwindow.cpp:427-467)
//
// Exactness: the window and the twiddles come from tables the host computed with the reference's double expressions; the
// input is stored digit-reversed, where kf_work's recursion leaves it before the first butterfly; every butterfly is
// kiss_fft's (same operands, same operation order, the twice-updated Fout[0] included) and the library is compiled with
// -ffp-contract=off, so no product is fused into an add.  Butterflies of one stage touch disjoint elements: running them in
// parallel changes no result.  The bins are therefore bit-identical to kiss_fft on the same input.  The power step is
// double arithmetic in the reference's order; only aveval is summed as a tree instead of sequentially (<= 1e-12 dB).
#pragma once

namespace sdrx {

constexpr int kSpecN = 8192;        // nFFT, mainwindow.cpp:243
constexpr int kSpecThreads = 512;   // 8 waves: 4 radix-4 butterflies per thread and stage
enum { kSpecNatural = 0, kSpecTiled = 1, kSpecRaw = 2 };

struct SpecRecord { // = sdrx_spectrum_info (include/sdrx.h)
    long long updates;
    int n_in, reserved;
    double maxval, aveval;
};

struct SpecDesc {
    const float2 *src[2]; // the stream per frame parity (kSpecNatural / kSpecTiled); kSpecRaw: SpecArgs::raw
    double *pwr;          // kSpecN doubles, the IIR state
    float2 *bins;         // kSpecN cf32: `out` of the last update, natural order
    SpecRecord *rec;
    int kind, n_in, level, pad;
};

struct SpecArgs {
    unsigned long long frame_level[kMaxLevels]; // the frame each tree level's streams hold in this launch
    const void *raw;                            // kSpecRaw: the frame (cf32 natural / tile layout, or dongle bytes)
    int raw_mode;                               // kRawF32 | kRawTiled | kRawU8
};

__device__ __forceinline__ float2 spec_cmul(float2 a, float2 b) // C_MUL, _kiss_fft_guts.h:89-91
{
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 spec_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 spec_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// where kf_work's recursion puts input n (factors 4,4,4,4,4,4,2): its base-4 digits d0..d5 (lowest first) reversed, times 2,
// plus the last radix-2 digit
__device__ __forceinline__ int spec_digit_rev(int n)
{
    int r = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        r = (r << 2) | (n & 3);
        n >>= 2;
    }
    return (r << 1) | n;
}

// One stream as k_spectrum and k_watch_psd (watch.hip) read it: natural order or tile layout cf32, or dongle bytes.
struct SpecSource {
    const float2 *src = nullptr;
    const unsigned char *bytes = nullptr;
    bool tiled = false;
};
__device__ __forceinline__ SpecSource spec_raw_source(const void *raw, int raw_mode)
{
    SpecSource S;
    if (raw_mode == kRawU8)
        S.bytes = static_cast<const unsigned char *>(raw);
    else
        S.src = static_cast<const float2 *>(raw);
    S.tiled = raw_mode == kRawTiled;
    return S;
}
// the frame that tree level `level` holds in this launch (a select chain, not a dynamic index into the kernel argument)
__device__ __forceinline__ unsigned long long spec_level_frame(const unsigned long long (&frame_level)[kMaxLevels], int level)
{
    unsigned long long f = frame_level[0];
#pragma unroll
    for (int l = 1; l < kMaxLevels; ++l)
        f = level == l ? frame_level[l] : f;
    return f;
}
__device__ __forceinline__ float2 spec_sample(const SpecSource &S, int g)
{
    if (S.bytes) // floats[b] = b - 127, jonti/sdr.cpp:43-49
        return make_float2((float)((int)S.bytes[2 * g] - 127), (float)((int)S.bytes[2 * g + 1] - 127));
    return S.src[S.tiled ? tile_index<int>(g) : g]; // (tile layout: sdrx_dev.h)
}

// kiss_fft of the kSpecN windowed samples input(0..kSpecN-1) into F (LDS, natural output order), by one workgroup of
// kSpecThreads threads; ends behind a barrier.
template <class Input>
__device__ __forceinline__ void spec_fft(float2 *F, Input input, const float2 *__restrict__ tw, int tid)
{
    // window + digit-reversed store, with the innermost stage (kf_bfly2, m = 1: the pair n, n + N/2 lands side by side) done
    // in registers on the way
    const float2 w0 = tw[0];
    for (int n = tid; n < kSpecN / 2; n += kSpecThreads) {
        float2 f0 = input(n), f1 = input(n + kSpecN / 2);
        const float2 t = spec_cmul(f1, w0);
        f1 = spec_sub(f0, t);
        f0 = spec_add(f0, t);
        const int pos = spec_digit_rev(n);
        *reinterpret_cast<float4 *>(&F[pos]) = make_float4(f0.x, f0.y, f1.x, f1.y);
    }
    __syncthreads();
    // kf_bfly4 for m = 2, 8, ..., 2048 (fstride = N / (4 m))
#pragma unroll 1
    for (int m = 2; m < kSpecN; m <<= 2) {
        const int fstride = kSpecN / (4 * m);
#pragma unroll
        for (int j = 0; j < kSpecN / 4 / kSpecThreads; ++j) {
            const int t = tid + j * kSpecThreads;
            const int k = t & (m - 1);
            float2 *Fo = &F[(t - k) * 4 + k];
            const float2 tw1 = tw[k * fstride], tw2 = tw[2 * k * fstride], tw3 = tw[3 * k * fstride];
            float2 f0 = Fo[0];
            const float2 f1 = Fo[m], f2 = Fo[2 * m], f3 = Fo[3 * m];
            const float2 s0 = spec_cmul(f1, tw1), s1 = spec_cmul(f2, tw2), s2 = spec_cmul(f3, tw3);
            const float2 s5 = spec_sub(f0, s1);
            f0 = spec_add(f0, s1);
            const float2 s3 = spec_add(s0, s2), s4 = spec_sub(s0, s2);
            Fo[2 * m] = spec_sub(f0, s3);
            Fo[0] = spec_add(f0, s3);
            Fo[m] = make_float2(s5.x + s4.y, s5.y - s4.x);
            Fo[3 * m] = make_float2(s5.x - s4.y, s5.y + s4.x);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kSpecThreads) void k_spectrum(const SpecDesc *__restrict__ descs, SpecArgs A,
                                                           const float2 *__restrict__ tw, const float *__restrict__ hann)
{
    __shared__ float2 F[kSpecN];
    __shared__ double red_max[kSpecThreads / 64], red_sum[kSpecThreads / 64];
    const SpecDesc &D = descs[blockIdx.x]; // (read in place: a dynamically indexed private copy would live in scratch)
    const int tid = threadIdx.x;
    SpecSource S;
    if (D.kind == kSpecRaw) {
        S = spec_raw_source(A.raw, A.raw_mode);
    } else {
        S.src = D.src[spec_level_frame(A.frame_level, D.level) & 1ull];
        S.tiled = D.kind == kSpecTiled;
    }
    const int n_in = D.n_in;
    spec_fft(
        F,
        [&](int a) -> float2 {
            if (a >= n_in)
                return make_float2(0.f, 0.f);
            const float2 x = spec_sample(S, a);
            const float h = hann[a];
            return make_float2(x.x * h, x.y * h);
        },
        tw, tid);
    // power, IIR, reductions (bin i feeds pwr[b], b = i + N/2 mod N: consecutive threads, consecutive doubles)
    double *pwr = D.pwr;
    float2 *bins = D.bins;
    double mx = 0.0, sum = 0.0;
    for (int i = tid; i < kSpecN; i += kSpecThreads) {
        const float2 o = F[i];
        bins[i] = o;
        const int b = (i + kSpecN / 2) & (kSpecN - 1);
        const double val = (double)sqrtf(o.y * o.y + o.x * o.x);
        const double p = pwr[b] * 0.95 + 0.05 * 10 * log10(fmax(100000.0 * fabs((1.0 / kSpecN) * val), 1.0));
        pwr[b] = p;
        if (p > mx)
            mx = p;
        sum += p;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double om = __shfl_xor(mx, off), os = __shfl_xor(sum, off);
        if (om > mx)
            mx = om;
        sum += os;
    }
    if ((tid & 63) == 0) {
        red_max[tid >> 6] = mx;
        red_sum[tid >> 6] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        mx = red_max[0];
        sum = red_sum[0];
        for (int w = 1; w < kSpecThreads / 64; ++w) {
            if (red_max[w] > mx)
                mx = red_max[w];
            sum += red_sum[w];
        }
        const double ave = sum / kSpecN;
        if (mx - ave < 10)
            mx = ave + 10.0;
        SpecRecord r = *D.rec;
        r.updates += 1;
        r.n_in = n_in;
        r.maxval = mx;
        r.aveval = ave;
        *D.rec = r;
    }
}

} // namespace sdrx
