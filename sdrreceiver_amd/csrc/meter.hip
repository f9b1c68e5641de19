// meter.hip -- the last step of every payload: the reference's float -> integer conversions as its x86-64 build does them
// (`short = double`, vfo.cpp:328,364: to_short, quantise; `char = float`, vfo.cpp:389-424: to_schar), the double excursion
// of vfo::usb_demod (usb_difference, vfo.cpp:317-328), and the output meters over the emitted values (option "meter";
// no counterpart in the reference).
// Relies on dev_helpers.hip (v4u, SDRX_AS1).  demod.hip, mix.hip and compress.hip use it.

// ---- int16 payloads: the conversions of vfo::usb_demod ----------------------------------------------------------------------
// `short = double` of the reference's x86-64 build (vfo.cpp:328,364): cvttsd2si truncates toward zero to
// int32 and yields INT32_MIN ("integer indefinite") for anything outside int32 or NaN; the low 16 bits are
// kept.  (The C standard calls the out-of-range case undefined; this is what the reference's binary does,
// and what the oracle restates.)  v_cvt_i32_f64 truncates the same way but SATURATES, hence the select.
__device__ __forceinline__ short to_short(double d)
{
    const int t = (d >= -2147483648.0 && d < 2147483648.0) ? (int)d : (int)0x80000000;
    return (short)(unsigned short)(unsigned)t;
}
// The reference's two excursions into double on this path (vfo.cpp:317-328) are kept literally.  Both have
// an fp32 form with identical results -- the exact difference of two floats rounded to 53 and then to 24
// bits is the fp32 subtraction (double rounding is innocuous for + - * / when the wide format has
// >= 2*24 + 2 significand bits), and `float * 2^15` is exact in either format with v_cvt_i32_f32
// saturating like v_cvt_i32_f64: all 115 GPU parity tests passed with that form, and it was not faster (k_usb_demod
// 35.8-37.0 vs 35.7-36.6 us on config 3), so the literal form stays.
__device__ __forceinline__ float usb_difference(float delayed_i, float hilbert)
{
    return (float)((double)delayed_i - (double)hilbert);
}
__device__ __forceinline__ float quantise(float scaled, short &out)
{
    const double pre = (double)scaled * 32768.0;
    // |pre| < 2^31 <=> |scaled| < 2^16 (the product is exact): the range test of to_short() as ONE fp32 compare
    out = fabsf(scaled) < 65536.0f ? (short)(unsigned short)(unsigned)(int)pre : (short)0;
    return (float)pre; // exact: float * 2^15
}

// ---- output meters (option "meter") --------------------------------------------------------------------------
// A work unit (a demodulation / low-pass / compress block, or a fused-demodulation mix item) folds the payload values it
// emits into ONE 16-byte record {sum of v*v (u64), samples that wrapped, max |pre| as the bits of a non-negative float} and
// writes it to a slot of its own behind the payloads (the host sums a leaf's slots).  Every slot is written every frame:
// no zeroing, no atomics.  A lane's sum is 64-bit: four int16 -32768 squared already make 2^32.  The max of the bit
// patterns is the max of the magnitudes, and a NaN (bits above +inf) wins.
struct MeterAcc {
    unsigned long long sum_sq;
    unsigned clipped, peak;
};
__device__ __forceinline__ MeterAcc meter_zero() { return MeterAcc{0ull, 0u, 0u}; }
// an int16 value v = the short of quantise(), pre = its return value (exact): wrapped unless -32769 < pre < 32768
__device__ __forceinline__ void meter_usb(MeterAcc &m, float pre, short v)
{
    const int iv = v;
    m.sum_sq += (unsigned long long)(unsigned)(iv * iv);
    m.clipped += !(pre > -32769.0f && pre < 32768.0f);
    m.peak = max(m.peak, __float_as_uint(fabsf(pre)));
}
__device__ __forceinline__ void meter_wave_reduce(MeterAcc &m)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m.sum_sq += __shfl_xor(m.sum_sq, o, 64);
        m.clipped += (unsigned)__shfl_xor((int)m.clipped, o, 64);
        m.peak = max(m.peak, (unsigned)__shfl_xor((int)m.peak, o, 64));
    }
}
__device__ __forceinline__ void meter_put(unsigned char *slot, const MeterAcc &m)
{
    const v4u r = {(unsigned)m.sum_sq, (unsigned)(m.sum_sq >> 32), m.clipped, m.peak};
    *(SDRX_AS1 v4u *)slot = r;
}
// one wave's record (every lane of the wave calls it)
__device__ __forceinline__ void meter_wave_store(MeterAcc m, unsigned char *slot, int lane)
{
    meter_wave_reduce(m);
    if (lane == 0)
        meter_put(slot, m);
}
// one 256-thread block's record: every thread of the block calls it (a barrier inside); `red`: 64 bytes of LDS nothing else
// uses from here on (a static array would move the dynamic LDS of k_levels_tail's mix waves, and cost its exact form a spill)
__device__ __forceinline__ void meter_block_store(MeterAcc m, unsigned char *slot, int tid, MeterAcc *red)
{
    meter_wave_reduce(m);
    if ((tid & 63) == 0)
        red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            m.sum_sq += red[w].sum_sq;
            m.clipped += red[w].clipped;
            m.peak = max(m.peak, red[w].peak);
        }
        meter_put(slot, m);
    }
}

// ---- int8 payloads (k_compress, compress.hip) -------------------------------------------------------------------------------
__device__ __forceinline__ int to_schar(float f) // cvttss2si + the low 8 bits: out of int32 range or NaN -> INT32_MIN -> 0
{
    const int t = (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : (int)0x80000000;
    return (int)(signed char)(unsigned char)(unsigned)t;
}
// METER: n_values 2 n; v = each component's to_schar value (before cstyle 1's nibble masking), pre = what it converts; a
// sample wrapped when either component left -129 < pre < 128.
__device__ __forceinline__ void meter_iq(MeterAcc &m, float pre_re, float pre_im, int re, int im)
{
    m.sum_sq += (unsigned long long)(unsigned)(re * re + im * im);
    m.clipped += !(pre_re > -129.0f && pre_re < 128.0f && pre_im > -129.0f && pre_im < 128.0f);
    m.peak = max(m.peak, max(__float_as_uint(fabsf(pre_re)), __float_as_uint(fabsf(pre_im))));
}
