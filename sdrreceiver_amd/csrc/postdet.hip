// postdet.hip -- the post-detection filter of the detector leaves (include/sdrx.h "Post-detection filter"): a real
// FIR of the caller's taps over the detector's pre-quantisation floats, decimated by R, with its history carried from frame to
// frame.  No counterpart in the reference; sdrx_postdet.h is the per-output definition, sdrx_detect.h the detector's.
// Relies on detect.hip (detect_pair, k_env_sum), dev_helpers.hip, meter.hip, sdrx_detect.h and sdrx_postdet.h.
// k_detect's geometry: 256 threads per block of kDetBlock = 4096 STREAM samples, on BlockWork lists of their own per kind (a leaf
// without the filter keeps k_detect).  A block stages pre[b0 - (T-1) .. end) as floats in LDS (17 408 bytes at most), then forms
// the outputs m with b0 <= m R < end from it.

// pre of the stream sample i >= 1 of this frame, from the stream alone: what a block's halo is made of (blk >= 1: the halo lies
// inside the frame, so the carrier and the gain are this frame's, as the definition has it)
template <int KIND>
__device__ __forceinline__ float postdet_pre_at(const float2 *z, int i, float c, float gain)
{
    const float2 v = gld2(z + i);
    if constexpr (KIND == kDetAm) {
        return detect_am_pre(detect_env(v.x, v.y), c, gain);
    } else {
        const float2 w = gld2(z + i - 1);
        return detect_fm_pre(v.x, v.y, w.x, w.y, gain);
    }
}

constexpr int kPdGroup = 4; // outputs a thread forms side by side: independent chains, one tap load for all of them

template <int KIND, bool METER = false, bool PARK = false>
__global__ __launch_bounds__(256) void k_detect_post(const K5Vfo *__restrict__ vfos, const K5Post *__restrict__ posts, const BlockWork *__restrict__ work,
                                                     unsigned long long frame_no, ParkArg<PARK> P)
{
    const BlockWork bw = work[blockIdx.x];
    if constexpr (PARK)
        if (ldc(P.act + bw.vfo) == 0)
            return;
    __shared__ float pre_s[kDetBlock + kPdMaxTaps]; // pre_s[j] = pre[b0 - H + j], 0 <= j < H + cnt
    const K5Vfo *Dp = vfos + bw.vfo;
    const K5Post *Pp = posts + bw.vfo;
    const int par = (int)(frame_no & 1ull);
    const int blk = bw.blk, tid = (int)threadIdx.x;
    const float2 *z = ldc(&Dp->s[par]);
    short *pay = ldc(&Dp->pay[par]);
    const int n = ldc(&Dp->n);
    const int b0 = blk * kDetBlock, end = min(n, b0 + kDetBlock), cnt = end - b0;
    const float gain = ldc(&Dp->gain);
    const float *taps = ldc(&Pp->taps);
    const int T = ldc(&Pp->ntaps), R = ldc(&Pp->decim), H = T - 1;
    float c = 0.0f;
    if constexpr (KIND == kDetAm) {
        const unsigned long long *part = ldc(&Dp->part[par]);
        unsigned long long S = 0;
        for (int b = 0; b < (n + kDetBlock - 1) / kDetBlock; ++b)
            S += *(const SDRX_AS1 unsigned long long *)(part + b);
        c = detect_carrier(S, n);
    }
    // ---- the halo: block 0 takes it from the leaf's history slot of this parity, every other block from the stream
    if (tid < H) {
        float v;
        if (blk == 0)
            v = gld(ldc(&Pp->hist[par]) + tid);
        else
            v = postdet_pre_at<KIND>(z, b0 - H + tid, c, gain); // (b0 - H >= 4096 - 255: sample i - 1 exists)
        pre_s[tid] = v;
    }
    // ---- the block's own samples, as k_detect forms them
#pragma unroll
    for (int k = 0; k < kDetBlock / (2 * kDetThreads); ++k) {
        const int i = detect_pair(blk, k, tid);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i + 1 < end) {
            v = gld4(reinterpret_cast<const float4 *>(z + i));
        } else if (i < end) {
            const float2 w = gld2(z + i);
            v.x = w.x, v.y = w.y;
        }
        float pre0, pre1;
        if constexpr (KIND == kDetAm) {
            pre0 = detect_am_pre(detect_env(v.x, v.y), c, gain);
            pre1 = detect_am_pre(detect_env(v.z, v.w), c, gain);
        } else {
            float2 before = make_float2(0.0f, 0.0f);
            if ((tid & 63) == 0 && i < end)
                before = gld2(i == 0 ? ldc(&Dp->zprev[par]) : z + i - 1);
            const float p = shr1(before.x, v.z), q = shr1(before.y, v.w);
            pre0 = detect_fm_pre(v.x, v.y, p, q, gain);
            pre1 = detect_fm_pre(v.z, v.w, v.x, v.y, gain);
        }
        if (i < end)
            pre_s[H + i - b0] = pre0;
        if (i + 1 < end)
            pre_s[H + i - b0 + 1] = pre1;
    }
    if constexpr (KIND == kDetFm)
        if (tid == 0 && end == n)
            gst2(ldc(&Dp->zprev[par ^ 1]), gld2(z + n - 1));
    __syncthreads();
    // ---- the block that holds sample n - 1 leaves the last T - 1 values of [history | frame] in the other parity's slot
    if (end == n && tid < H)
        *(SDRX_AS1 float *)(ldc(&Pp->hist[par ^ 1]) + tid) = pre_s[cnt + tid];
    // ---- the outputs m with b0 <= m R < end.  t is wave-uniform: the tap is a scalar load; pre comes from LDS at stride R.
    const int m0 = (b0 + R - 1) / R, m1 = (end + R - 1) / R;
    MeterAcc macc = meter_zero();
    for (int g = m0; g < m1; g += kPdGroup * kDetThreads) {
        int at[kPdGroup];
        float acc[kPdGroup];
#pragma unroll
        for (int k = 0; k < kPdGroup; ++k) {
            const int m = g + k * kDetThreads + tid;
            at[k] = m < m1 ? H + m * R - b0 : H; // (a lane without an output reads pre_s[H - t]: inside the array, never stored)
            acc[k] = 0.0f;
        }
        for (int t = 0; t < T; ++t) {
            const float h = ldc(taps + t);
#pragma unroll
            for (int k = 0; k < kPdGroup; ++k) {
                const float p = h * pre_s[at[k] - t];
                acc[k] = acc[k] + p;
            }
        }
#pragma unroll
        for (int k = 0; k < kPdGroup; ++k) {
            const int m = g + k * kDetThreads + tid;
            short s;
            const float mv = quantise(acc[k], s);
            if (m < m1) {
                *(SDRX_AS1 short *)(pay + m) = s;
                if constexpr (METER)
                    meter_usb(macc, mv, s);
            }
        }
    }
    if constexpr (METER) {
        __shared__ MeterAcc red[4];
        meter_block_store(macc, reinterpret_cast<unsigned char *>(pay) + ldc(&Dp->meter_rel) + 16 * blk, tid, red);
    }
}
