// detect.hip -- the detector leaves (include/sdrx.h "Detector leaves"): the int16 payload of a non-USB leaf's stream
// as an AM envelope or an FM discriminator.  No counterpart in the reference; sdrx_detect.h is the per-sample definition.
// Relies on dev_helpers.hip (ldc, gld2, gld4, shr1), meter.hip (quantise, meter_usb, meter_block_store) and sdrx_detect.h.
// k_compress's geometry: 256 threads per block of kDetBlock = 4096 samples, on BlockWork lists; a thread takes eight sample PAIRS,
// 16-byte loads (the stream of such a leaf has no history in front: its base is a multiple of 16 bytes), one 4-byte store a pair.

// The samples of block `blk` a thread owns in turn k: the pair from sample i on; what lies at or past `end` is not touched.
__device__ __forceinline__ int detect_pair(int blk, int k, int tid) { return blk * kDetBlock + 2 * (k * kDetThreads + tid); }

// ------------------------------------------------------------------------------------ k_env_sum
// AM, first pass: S of this block -- the sum of detect_env_q over its samples, exact in 64-bit integers whatever the order -- into
// the block's slot of this frame parity.  Every slot is written every frame: no zeroing, no atomics (the meter's idiom).
template <bool PARK = false>
__global__ __launch_bounds__(256) void k_env_sum(const K5Vfo *__restrict__ vfos, const BlockWork *__restrict__ work, unsigned long long frame_no,
                                                 ParkArg<PARK> P)
{
    const BlockWork bw = work[blockIdx.x];
    if constexpr (PARK)
        if (ldc(P.act + bw.vfo) == 0)
            return;
    const K5Vfo *Dp = vfos + bw.vfo;
    const int par = (int)(frame_no & 1ull);
    const int blk = bw.blk, tid = (int)threadIdx.x;
    const float2 *z = ldc(&Dp->s[par]);
    const int end = min(ldc(&Dp->n), (blk + 1) * kDetBlock);
    unsigned long long sum = 0;
#pragma unroll
    for (int k = 0; k < kDetBlock / (2 * kDetThreads); ++k) {
        const int i = detect_pair(blk, k, tid);
        if (i + 1 < end) {
            const float4 v = gld4(reinterpret_cast<const float4 *>(z + i));
            sum += detect_env_q(detect_env(v.x, v.y)) + detect_env_q(detect_env(v.z, v.w)); // (2^24 at most: no carry out of 32 bits)
        } else if (i < end) {
            const float2 v = gld2(z + i);
            sum += detect_env_q(detect_env(v.x, v.y));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        sum += __shfl_xor(sum, o, 64);
    __shared__ unsigned long long red[4];
    if ((tid & 63) == 0)
        red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0)
        *(SDRX_AS1 unsigned long long *)(ldc(&Dp->part[par]) + blk) = red[0] + red[1] + red[2] + red[3];
}

// ------------------------------------------------------------------------------------ k_detect
// KIND = kDetAm: every block adds its leaf's partials of this parity in block order (exact: any order gives the same S), forms the
// carrier, and emits quantise(fl(fl(e - c) gain)).
// KIND = kDetFm: quantise(fl(ANG(z[i] conj(z[i-1])) gain)).  z[i-1] of a pair's first sample is the lane below's second one (one DPP
// move); lane 0 of a wave reads it from the stream, and sample 0 of the frame takes the leaf's 8-byte slot of this parity.  The block
// that holds sample n - 1 writes it to the other parity's slot: z[-1] of the next frame.
template <int KIND, bool METER = false, bool PARK = false>
__global__ __launch_bounds__(256) void k_detect(const K5Vfo *__restrict__ vfos, const BlockWork *__restrict__ work, unsigned long long frame_no,
                                                ParkArg<PARK> P)
{
    const BlockWork bw = work[blockIdx.x];
    if constexpr (PARK)
        if (ldc(P.act + bw.vfo) == 0)
            return;
    const K5Vfo *Dp = vfos + bw.vfo;
    const int par = (int)(frame_no & 1ull);
    const int blk = bw.blk, tid = (int)threadIdx.x;
    const float2 *z = ldc(&Dp->s[par]);
    short *pay = ldc(&Dp->pay[par]);
    const int n = ldc(&Dp->n);
    const int end = min(n, (blk + 1) * kDetBlock);
    const float gain = ldc(&Dp->gain);
    float c = 0.0f;
    if constexpr (KIND == kDetAm) {
        const unsigned long long *part = ldc(&Dp->part[par]);
        unsigned long long S = 0;
        for (int b = 0; b < (n + kDetBlock - 1) / kDetBlock; ++b)
            S += *(const SDRX_AS1 unsigned long long *)(part + b);
        c = detect_carrier(S, n);
    }
    MeterAcc macc = meter_zero();
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
            // (every lane of the wave is here: a lane with samples has a lane below that loaded a whole pair)
            const float p = shr1(before.x, v.z), q = shr1(before.y, v.w);
            pre0 = detect_fm_pre(v.x, v.y, p, q, gain);
            pre1 = detect_fm_pre(v.z, v.w, v.x, v.y, gain);
        }
        short s0, s1;
        const float m0 = quantise(pre0, s0), m1 = quantise(pre1, s1);
        if (i + 1 < end) {
            *(SDRX_AS1 unsigned *)(pay + i) = (unsigned)(unsigned short)s0 | ((unsigned)(unsigned short)s1 << 16);
            if constexpr (METER) {
                meter_usb(macc, m0, s0);
                meter_usb(macc, m1, s1);
            }
        } else if (i < end) {
            *(SDRX_AS1 short *)(pay + i) = s0;
            if constexpr (METER)
                meter_usb(macc, m0, s0);
        }
    }
    if constexpr (KIND == kDetFm)
        if (tid == 0 && end == n)
            gst2(ldc(&Dp->zprev[par ^ 1]), gld2(z + n - 1));
    if constexpr (METER) {
        __shared__ MeterAcc red[4];
        meter_block_store(macc, reinterpret_cast<unsigned char *>(pay) + ldc(&Dp->meter_rel) + 16 * blk, tid, red);
    }
}
