// adcmeter.hip -- option adc_meter: exact integer statistics of a frame of integer samples AS IT ARRIVED (include/sdrx.h,
// sdrx_adc_meter): k_adc_meter<FMT>, a template on the format like the ingest family, reading the frame with the
// 16-byte loads k_dc_apply uses.  Nothing is decoded to float: there is no floating-point operation in this file.
// Relies on dev_helpers.hip (gldv4u) and ingest.hip (wave_inclusive_scan).
//
// Geometry (tests/adc_ref.py names the same four numbers): a 16-byte load holds 8 complex samples of an 8-bit format and 4 of
// int16; a thread owns kAdcThread = 16 consecutive samples (2 or 4 loads), a wave 1024, a workgroup kAdcWg = 4096.  Frames are
// multiples of 16 samples and nothing more, so a thread either lies inside the frame or holds nothing at all: a thread behind
// the frame's end loads nothing and carries the neutral element (no sample, no rail, no bin, min = INT_MAX, max = INT_MIN).
//
// The reduction is one associative element per arm -- sums, min / max, rail counts and the run element (length, prefix run,
// suffix run, best) -- folded thread -> wave (DPP scans for the sums, shuffles for min / max and, in lane order, for the runs)
// -> workgroup (four wave partials through LDS, merged in wave order) -> one AdcPartial per workgroup in global memory -> the
// workgroup that counts last merges the partials in workgroup order (a tree in LDS) and writes the record.  Release fence in
// front of the count, acquire fence behind the last one: k_watch_psd's and k_watch_drift's pattern.  No 64-bit global atomics.
// Widths: a thread's sum of squares reaches 16 * 2^30, so it is 64 bits wide from the first sample on; for the DPP scans it is
// split at bit 20 into two parts whose wave sums fit 32 bits (adc_wave_sum64 below).  Plain sums fit 32 bits up to a workgroup
// (4096 * 2^15 = 2^27) and are 64 bits wide from the partial on.

constexpr int kAdcThread = 16;                    // complex samples per thread
constexpr int kAdcThreads = 256;                  // threads per workgroup
constexpr int kAdcWg = kAdcThread * kAdcThreads;  // complex samples per workgroup
constexpr int kAdcBins = 17;

// sdrx_adc_arm / sdrx_adc_meter of include/sdrx.h, as the device writes them (the layout is asserted in sdrx.hip)
struct AdcArm {
    long long sum;
    unsigned long long sum_sq;
    int min, max;
    unsigned at_lo, at_hi, longest_rail_run, reserved;
};
struct AdcRecord {
    long long frame;
    unsigned n_complex;
    int fmt;
    unsigned measured, reserved;
    AdcArm i, q;
    long long sum_iq;
    unsigned bits[kAdcBins];
    unsigned reserved2;
};

// The associative element of a run of consecutive samples (everything but the histogram, which is a plain sum): [0] = I, [1] = Q.
struct AdcElem {
    long long sum[2], sum_iq;
    unsigned long long sq[2];
    int mn[2], mx[2];
    unsigned lo[2], hi[2];
    unsigned len;                    // samples
    unsigned pre[2], suf[2], best[2]; // rail run at the start, at the end (== len: all of it), the longest anywhere
};
struct AdcPartial { // what a workgroup leaves
    AdcElem e;
    unsigned bits[kAdcBins];
    unsigned pad;
};

// a := a followed by b
__device__ __forceinline__ void adc_merge(AdcElem &a, const AdcElem &b)
{
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        a.sum[c] += b.sum[c];
        a.sq[c] += b.sq[c];
        a.mn[c] = min(a.mn[c], b.mn[c]);
        a.mx[c] = max(a.mx[c], b.mx[c]);
        a.lo[c] += b.lo[c];
        a.hi[c] += b.hi[c];
        a.best[c] = max(max(a.best[c], b.best[c]), a.suf[c] + b.pre[c]);
        a.pre[c] = a.pre[c] == a.len ? a.len + b.pre[c] : a.pre[c];
        a.suf[c] = b.suf[c] == b.len ? b.len + a.suf[c] : b.suf[c];
    }
    a.sum_iq += b.sum_iq;
    a.len += b.len;
}

// The formats of 16-bit components: CS16, and the real formats RS16 and RU12, whose frame is read as pairs (even samples in arm
// I, odd samples in arm Q: include/sdrx.h "Front stage").
template <int FMT>
constexpr bool kAdcWide = FMT == SDRX_FMT_CS16 || FMT == SDRX_FMT_RS16 || FMT == SDRX_FMT_RU12;

// The integer code of component `comp` (0 = I, 1 = Q) of sample s of a 16-byte unit: CU8 b - 127, CS8 / CS16 / RS16 the integer
// itself, RU12 the 12-bit offset code (v & 4095) - 2048.
template <int FMT>
__device__ __forceinline__ int adc_code(const v4u q, int s, int comp)
{
    static_assert(FMT == SDRX_FMT_CU8 || FMT == SDRX_FMT_CS8 || kAdcWide<FMT>, "a format of include/sdrx.h");
    if constexpr (FMT == SDRX_FMT_RU12) {
        const unsigned w = q[s];
        return (int)((comp ? w >> 16 : w) & 4095u) - 2048;
    } else if constexpr (kAdcWide<FMT>) {
        const unsigned w = q[s];
        return comp ? (int)w >> 16 : (int)(short)(w & 0xffffu);
    } else {
        const unsigned w = q[s >> 1];
        const int sh = 16 * (s & 1) + 8 * comp;
        if constexpr (FMT == SDRX_FMT_CU8)
            return (int)((w >> sh) & 255u) - 127;
        else
            return (int)(w << (24 - sh)) >> 24;
    }
}
template <int FMT>
struct AdcRails {
    static constexpr int lo = FMT == SDRX_FMT_CU8 ? -127 : FMT == SDRX_FMT_CS8 ? -128 : FMT == SDRX_FMT_RU12 ? -2048 : -32768;
    static constexpr int hi = FMT == SDRX_FMT_CU8 ? 128 : FMT == SDRX_FMT_CS8 ? 127 : FMT == SDRX_FMT_RU12 ? 2047 : 32767;
};

// A 64-bit value of at most 35 significant bits (signed: arithmetic shift) as two parts whose sums over a wave fit 32 bits:
// x = (hi << 20) + lo with 0 <= lo < 2^20.
__device__ __forceinline__ long long adc_wave_sum64(long long x)
{
    const int hi = (int)(x >> 20), lo = (int)(x & 0xfffff);
    const int shi = __builtin_amdgcn_readlane(wave_inclusive_scan(hi), 63), slo = __builtin_amdgcn_readlane(wave_inclusive_scan(lo), 63);
    return ((long long)shi << 20) + (long long)slo;
}
__device__ __forceinline__ int adc_wave_sum(int x) { return __builtin_amdgcn_readlane(wave_inclusive_scan(x), 63); }

template <int FMT>
__global__ __launch_bounds__(kAdcThreads) void k_adc_meter(const unsigned *__restrict__ words, int n_complex, long long frame,
                                                           AdcPartial *__restrict__ part, unsigned *__restrict__ counter,
                                                           AdcRecord *__restrict__ rec, int per, int cnt)
{
    constexpr int kLoads = kAdcWide<FMT> ? 4 : 2, kPer = kAdcThread / kLoads; // 16-byte loads per thread, samples in each
    constexpr int LO = AdcRails<FMT>::lo, HI = AdcRails<FMT>::hi;
    __shared__ AdcElem sh_e[kAdcThreads]; // [0..3]: the waves' partials; the last workgroup: one element per thread
    __shared__ unsigned sh_bits[kAdcThreads / 64][kAdcBins];
    __shared__ unsigned sh_hist[kAdcBins];
    __shared__ bool sh_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long t = (long long)blockIdx.x * kAdcThreads + tid; // this thread's block of 16 samples
    const bool valid = t * kAdcThread < (long long)n_complex;

    // ---- the thread's own 16 samples, in registers
    int sum[2] = {0, 0}, mn[2] = {0x7fffffff, 0x7fffffff}, mx[2] = {(int)0x80000000, (int)0x80000000};
    unsigned long long sq[2] = {0ull, 0ull};
    long long iq = 0;
    unsigned lo[2] = {0u, 0u}, hi[2] = {0u, 0u}, cur[2] = {0u, 0u}, pre[2] = {0u, 0u}, best[2] = {0u, 0u}, all[2] = {1u, 1u};
    unsigned long long hb0 = 0ull, hb1 = 0ull; // 6-bit counters (at most 32 components): bins 0..9 | bins 10..16
    if (valid) {
        const v4u *src = reinterpret_cast<const v4u *>(words) + (size_t)t * kLoads;
        v4u q[kLoads];
#pragma unroll
        for (int h = 0; h < kLoads; ++h)
            q[h] = gldv4u(src + h);
#pragma unroll
        for (int h = 0; h < kLoads; ++h) {
#pragma unroll
            for (int s = 0; s < kPer; ++s) {
                int v[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    v[c] = adc_code<FMT>(q[h], s, c);
                    const unsigned a = (unsigned)(v[c] < 0 ? -v[c] : v[c]);
                    sum[c] += v[c];
                    sq[c] += (unsigned long long)(a * a); // |v| <= 2^15: the square fits 32 bits, the sum of four does not
                    mn[c] = min(mn[c], v[c]);
                    mx[c] = max(mx[c], v[c]);
                    const unsigned is_lo = v[c] == LO, is_hi = v[c] == HI, rail = is_lo | is_hi;
                    lo[c] += is_lo;
                    hi[c] += is_hi;
                    cur[c] = rail ? cur[c] + 1u : 0u;
                    best[c] = max(best[c], cur[c]);
                    all[c] &= rail;
                    pre[c] += all[c];
                    const unsigned k = 32u - (unsigned)__clz((int)a); // bit_length(|v|): 0 for 0, 16 for 32768
                    if constexpr (kAdcWide<FMT>) {
                        hb0 += (unsigned long long)(k < 10u) << ((6u * k) & 63u);
                        hb1 += (unsigned long long)(k >= 10u) << ((6u * k - 60u) & 63u);
                    } else {
                        hb0 += 1ull << (6u * k); // |v| <= 128: bins 0..8
                    }
                }
                iq += (long long)(v[0] * v[1]); // |vI vQ| <= 2^30
            }
        }
    }
    const unsigned len = valid ? (unsigned)kAdcThread : 0u;

    // ---- wave: sums by DPP scan (the total in lane 63, broadcast), min / max by butterfly, the runs in lane order towards lane 63
    AdcElem w;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        w.sum[c] = (long long)adc_wave_sum(sum[c]);
        w.sq[c] = (unsigned long long)adc_wave_sum64((long long)sq[c]);
        const unsigned lohi = (unsigned)adc_wave_sum((int)(lo[c] | (hi[c] << 16))); // at most 1024 each
        w.lo[c] = lohi & 0xffffu;
        w.hi[c] = lohi >> 16;
        int a = mn[c], b = mx[c];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            a = min(a, __shfl_xor(a, d));
            b = max(b, __shfl_xor(b, d));
        }
        w.mn[c] = a;
        w.mx[c] = b;
    }
    w.sum_iq = adc_wave_sum64(iq);
    {
        unsigned L = len, P[2] = {pre[0], pre[1]}, S[2] = {cur[0], cur[1]}, B[2] = {best[0], best[1]};
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { // lane l: the lanes (l - 2 d, l] in order; only lane 63's chain has to be whole
            const unsigned Ll = __shfl_up(L, d);
            const bool has = lane >= d;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const unsigned Pl = __shfl_up(P[c], d), Sl = __shfl_up(S[c], d), Bl = __shfl_up(B[c], d);
                if (has) { // (left part, then this lane's)
                    B[c] = max(max(Bl, B[c]), Sl + P[c]);
                    P[c] = Pl == Ll ? Ll + P[c] : Pl;
                    S[c] = S[c] == L ? L + Sl : S[c];
                }
            }
            if (has)
                L += Ll;
        }
        w.len = L;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            w.pre[c] = P[c], w.suf[c] = S[c], w.best[c] = B[c];
    }
    // the histogram: pairs of bins as 16-bit halves (a workgroup holds 8192 components), one DPP scan per pair
    unsigned wb[kAdcBins];
#pragma unroll
    for (int j = 0; j < (kAdcBins + 1) / 2; ++j) {
        const int k0 = 2 * j, k1 = 2 * j + 1;
        auto field = [&](int k) -> unsigned {
            if (k >= kAdcBins || (!kAdcWide<FMT> && k > 8))
                return 0u;
            return k < 10 ? (unsigned)(hb0 >> (6 * k)) & 63u : (unsigned)(hb1 >> (6 * (k - 10))) & 63u;
        };
        if (!kAdcWide<FMT> && k0 > 8) {
            wb[k0] = 0u;
            if (k1 < kAdcBins)
                wb[k1] = 0u;
            continue;
        }
        const unsigned s = (unsigned)adc_wave_sum((int)(field(k0) | (field(k1) << 16)));
        wb[k0] = s & 0xffffu;
        if (k1 < kAdcBins)
            wb[k1] = s >> 16;
    }
    if (lane == 63) {
        sh_e[wave] = w;
#pragma unroll
        for (int k = 0; k < kAdcBins; ++k)
            sh_bits[wave][k] = wb[k];
    }
    __syncthreads();

    // ---- workgroup: the four wave partials in wave order; one partial to global memory
    if (tid == 0) {
        AdcElem e = sh_e[0];
#pragma unroll
        for (int k = 1; k < kAdcThreads / 64; ++k)
            adc_merge(e, sh_e[k]);
        part[blockIdx.x].e = e;
    }
    if (tid < kAdcBins) {
        unsigned s = 0u;
#pragma unroll
        for (int k = 0; k < kAdcThreads / 64; ++k)
            s += sh_bits[k][tid];
        part[blockIdx.x].bits[tid] = s;
        sh_hist[tid] = 0u;
    }
    __threadfence();
    __syncthreads();
    if (tid == 0)
        sh_last = atomicAdd(counter, 1u) == gridDim.x - 1u;
    __syncthreads();
    if (!sh_last)
        return;
    __threadfence();

    // ---- the workgroup that counted last: every partial is there.  Thread j < cnt merges a contiguous stretch of `per` of them
    // in order (the host's division: per = ceil(nb / 256), cnt = ceil(nb / per) -- an integer division here would be the
    // compiler's float reciprocal), a tree in LDS merges the threads' elements in order; the histogram is a plain sum.
    const int nb = (int)gridDim.x;
    if (tid < cnt) {
        const int first = tid * per, last = min(first + per, nb);
        AdcElem e = part[first].e;
        for (int b = first + 1; b < last; ++b)
            adc_merge(e, part[b].e);
        sh_e[tid] = e;
    }
    for (int b = tid / 32, k = tid % 32; b < nb && k < kAdcBins; b += kAdcThreads / 32) // (half a wave per partial, a lane per bin)
        atomicAdd(&sh_hist[k], part[b].bits[k]);
    for (int s = 1; s < cnt; s <<= 1) {
        __syncthreads();
        if ((tid & (2 * s - 1)) == 0 && tid + s < cnt) {
            AdcElem e = sh_e[tid];
            adc_merge(e, sh_e[tid + s]);
            sh_e[tid] = e;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const AdcElem e = sh_e[0];
        AdcRecord r;
        r.frame = frame;
        r.n_complex = (unsigned)n_complex;
        r.fmt = FMT;
        r.measured = 1u;
        r.reserved = 0u;
        AdcArm *arm[2] = {&r.i, &r.q};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            arm[c]->sum = e.sum[c];
            arm[c]->sum_sq = e.sq[c];
            arm[c]->min = e.mn[c];
            arm[c]->max = e.mx[c];
            arm[c]->at_lo = e.lo[c];
            arm[c]->at_hi = e.hi[c];
            arm[c]->longest_rail_run = e.best[c];
            arm[c]->reserved = 0u;
        }
        r.sum_iq = e.sum_iq;
#pragma unroll
        for (int k = 0; k < kAdcBins; ++k)
            r.bits[k] = sh_hist[k];
        r.reserved2 = 0u;
        *rec = r;
        *counter = 0u; // (the next launch of this context is behind this one in stream order)
    }
}
