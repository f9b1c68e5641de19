// late.hip -- the late decimation by 5 or 6 as kernels of its own: the FIR half of vfo::usb_decimdemod (vfo.cpp:334-387 with
// FIR::FIRUpdateAndProcess / FIRUpdate, dsp.cpp:59-71,150-154) for the leaves whose low-pass does not run in the mix wave
// (late_item, mix.hip): k_late_decimate, one output per thread, and k_late_decimate4, one wave per 128 outputs.
// Relies on dev_helpers.hip (ldc, gld*, gst2, v2f, v4f, wave_sync).

// ------------------------------------------------------------------------------------ k_late_decimate
// Late decimation by L in {5,6} (vfo.cpp:334-387 with FIR::FIRUpdateAndProcess/FIRUpdate,
// dsp.cpp:59-71,150-154): z'[k] = sum_i hd[i] * x[L k - Nd + i]  -- the newest sample x[L k] is
// NOT part of the sum ((N+1)-slot ring).  The phase counter restarts every frame and frames are
// multiples of L, so k is frame-local.  256 outputs per block; the input window sits in LDS.
template <bool EXACT, bool PARK = false>
__global__ __launch_bounds__(256) void k_late_decimate(const K2aVfo *__restrict__ vfos, const BlockWork *__restrict__ work,
                                                       unsigned long long frame_no, ParkArg<PARK> P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *sx = reinterpret_cast<float2 *>(smem);
    const BlockWork bw = work[blockIdx.x];
    if constexpr (PARK)
        if (ldc(P.act + bw.vfo) == 0)
            return;
    const K2aVfo *Dp = vfos + bw.vfo;
    const int blk = bw.blk;
    const int par = (int)(frame_no & 1ull);
    const int tid = threadIdx.x;
    struct {
        const float *taps;
        int Hx, n, ndec, L, n_out;
    } D = {Dp->taps, Dp->Hx, Dp->n, Dp->ndec, Dp->L, Dp->n_out};
    const float2 *xbase = Dp->x[par];
    float2 *xnext = Dp->x_next[par];
    float2 *zout = Dp->z[par];
    const float2 *x = xbase + D.Hx; // sample 0 of this frame
    const int k0 = blk * 256;
    if (k0 >= D.n_out && blk != 0)
        return;
    // history for the next frame: the last Hx entries of [hist | data]
    if (blk == 0)
        for (int j = tid; j < D.Hx; j += 256)
            gst2(xnext + j, gld2(xbase + D.n + j));
    const int lo = D.L * k0 - D.ndec;              // first input index needed (>= -Hx)
    const int span = D.L * 255 + D.ndec;           // indices lo .. lo+span-1 feed the 256 outputs
    for (int t = tid; t < span; t += 256) {
        const int idx = lo + t;
        sx[t] = idx < D.n ? gld2(x + idx) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    const int k = k0 + tid;
    if (k >= D.n_out)
        return;
    const float2 *w = sx + D.L * tid; // w[i] = x[L k - Nd + i]
    float ar = 0.f, ai = 0.f;
    if (EXACT) {
        for (int i = 0; i < D.ndec; ++i) {
            const float h = gld(D.taps + i);
            ar = ar + h * w[i].x;
            ai = ai + h * w[i].y;
        }
    } else {
        for (int i = 0; i < D.ndec; ++i) {
            const float h = gld(D.taps + i);
            ar = fmaf(h, w[i].x, ar);
            ai = fmaf(h, w[i].y, ai);
        }
    }
    gst2(zout + k, make_float2(ar, ai));
}

// ------------------------------------------------------------------------------------ k_late_decimate4
// The same for L in {5,6} (all the reference configures, mainwindow.cpp:196-216) and Nd <= 96: ONE
// wave per 64 R outputs, R = 2 consecutive outputs per lane.  The R windows of a lane overlap
// (Nd + (R-1) L samples instead of R Nd), so a lane streams ITS window once (two ds_read_b128 per
// 4 samples) and feeds R accumulator pairs; output r uses tap j - L r for window sample j, read
// as aligned ds_read_b128 from a copy of the taps shifted by L r (zero outside [0, Nd): adding
// 0*x never changes a float sum).  The lane stride in LDS is padded to an odd multiple of 16
// bytes so that 8 lanes' b128 reads cover all 32 banks.  Same summation order as the reference:
// one accumulator per output and component, taps in ascending order.
// R = 2 (8 KB of LDS per wave, ~20 waves per CU) measured 38 us on config 4, R = 4 (fewer LDS reads, 16 KB, 10 waves per CU)
// 48 us, the one-output-per-thread kernel 54 us.
constexpr int kLateMaxTaps = 96;
constexpr int kLate4R = 2;
constexpr int kLateTapRow = 124; // shifted tap copies: u = i + L r < Nd + 3 L = 114 (+ b128 overrun), a multiple of 4
__host__ __device__ constexpr int late4_pad(int L) { return (2 * kLate4R * L) % 8 == 4 ? 0 : 2; } // float2 per R L samples
__host__ __device__ constexpr int late4_lds_bytes(int L, int ndec) // for the launch's largest L and Nd
{
    constexpr int R = kLate4R;
    const int span = L * (64 * R - 1) + ndec + (R - 1) * L;
    return 4 * R * kLateTapRow + 8 * (span + 2 * (span / (R * L)) + 16);
}

template <bool EXACT, int L>
__device__ __forceinline__ void late4_body(const float2 *__restrict__ x, float2 *__restrict__ zout, const float *__restrict__ taps, int n, int ndec,
                                           int n_out, int k0, int lane, v2f *__restrict__ sx, float *__restrict__ sh)
{
    constexpr int R = kLate4R;
    constexpr int kPad = late4_pad(L);
    constexpr int kStride = R * L + kPad;                                          // float2 per lane
    constexpr int kIters = (L * (64 * R - 1) + kLateMaxTaps + (R - 1) * L + 8 + 63) / 64; // window loads per lane (+8: zero tail)
    constexpr int kTapIters = (R * kLateTapRow + 63) / 64;
    const int lo = L * k0 - ndec;                       // first input index of the tile's window (>= -Hx)
    const int span = L * (64 * R - 1) + ndec + (R - 1) * L; // lanes' windows end at lo + R L lane + ndec + (R-1) L
    // every load of the lane is issued before the first LDS write (see k_usb_demod)
    v2f stage[kIters];
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const int t = lane + 64 * it, idx = lo + t;
        const v2f z2 = {0.f, 0.f};
        stage[it] = (t < span && idx < n) ? gldv2(x + idx) : z2;
    }
    float hst[kTapIters];
#pragma unroll
    for (int it = 0; it < kTapIters; ++it) {
        const int u = lane + 64 * it;
        const int r = u / kLateTapRow, i = u - r * kLateTapRow - L * r;
        hst[it] = (u < R * kLateTapRow && i >= 0 && i < ndec) ? gld(taps + i) : 0.f;
    }
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const int t = lane + 64 * it;
        if (t < span + 8) // the entries just past the span are read under zero taps only: they must be finite
            sx[t + kPad * (t / (R * L))] = stage[it];
    }
#pragma unroll
    for (int it = 0; it < kTapIters; ++it) {
        const int u = lane + 64 * it;
        if (u < R * kLateTapRow)
            sh[u] = hst[it];
    }
    wave_sync();
    const int k = k0 + R * lane;
    if (k >= n_out)
        return;
    const v2f *w = sx + kStride * lane; // window sample j sits at w[j + kPad * (j / (R L))]
    v2f acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
        acc[r] = v2f{0.f, 0.f};
    const int groups = (ndec + (R - 1) * L + 3) / 4;
    for (int g = 0; g < groups; ++g) {
        const int j = 4 * g;
        const v4f a = *reinterpret_cast<const v4f *>(w + j + kPad * (j / (R * L)));
        const v4f b = *reinterpret_cast<const v4f *>(w + j + 2 + kPad * ((j + 2) / (R * L)));
        const v2f xs[4] = {lo2(a), hi2(a), lo2(b), hi2(b)};
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const v4f h4 = *reinterpret_cast<const v4f *>(sh + r * kLateTapRow + j);
            const float h[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const v2f hh = {h[e], h[e]};
                if (EXACT)
                    acc[r] = acc[r] + hh * xs[e];
                else
                    acc[r] = __builtin_elementwise_fma(hh, xs[e], acc[r]);
            }
        }
    }
    if (k + R - 1 < n_out) {
#pragma unroll
        for (int r = 0; r < R; r += 2)
            gstv4(reinterpret_cast<float4 *>(zout + k + r), cat2(acc[r], acc[r + 1]));
    } else {
        for (int r = 0; r < R && k + r < n_out; ++r)
            gstv2(zout + k + r, acc[r]);
    }
}

constexpr int kLate4Waves = 6; // 76 VGPRs; measured 34.0 us vs 35.4 (5 waves) and 35.5 (8 waves) on config 4
template <bool EXACT, bool PARK = false>
__global__ __launch_bounds__(64, kLate4Waves) void k_late_decimate4(const K2aVfo *__restrict__ vfos, const BlockWork *__restrict__ work,
                                                       unsigned long long frame_no, ParkArg<PARK> P)
{
    constexpr int R = kLate4R;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *sh = reinterpret_cast<float *>(smem);
    v2f *sx = reinterpret_cast<v2f *>(smem + 4 * R * kLateTapRow);
    const BlockWork bw = work[blockIdx.x];
    if constexpr (PARK)
        if (ldc(P.act + bw.vfo) == 0)
            return;
    const K2aVfo *Dp = vfos + bw.vfo;
    const int par = (int)(frame_no & 1ull);
    const int lane = threadIdx.x;
    struct {
        const float *taps;
        int Hx, n, ndec, L, n_out;
    } D = {Dp->taps, Dp->Hx, Dp->n, Dp->ndec, Dp->L, Dp->n_out};
    const float2 *xbase = Dp->x[par];
    float2 *xnext = Dp->x_next[par];
    const int k0 = bw.blk * 64 * R;
    if (k0 >= D.n_out && bw.blk != 0)
        return;
    if (bw.blk == 0) // history for the next frame: the last Hx entries of [hist | data]
        for (int j = lane; j < D.Hx; j += 64)
            gst2(xnext + j, gld2(xbase + D.n + j));
    if (D.L == 5)
        late4_body<EXACT, 5>(xbase + D.Hx, Dp->z[par], D.taps, D.n, D.ndec, D.n_out, k0, lane, sx, sh);
    else
        late4_body<EXACT, 6>(xbase + D.Hx, Dp->z[par], D.taps, D.n, D.ndec, D.n_out, k0, lane, sx, sh);
}
