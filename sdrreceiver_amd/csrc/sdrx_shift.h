// sdrx_shift.h -- the frequency shift at the end of the ingest chain (include/sdrx.h "Frequency shift"): the rules of
// its settings, the three rotation tables, the split of a 32-bit phase into their indices, the product (three fp32 roundings a
// component, in one association and operand order), the frame advance, the Hz <-> increment conversion and the geometry of k_shift.
// Plain C++: shared by the kernels (shift.hip), the launch code (sdrx_frame.hip), the library (sdrx.hip, sdrx_finalize.hip) and a
// stand-alone check (host/shift_check.cpp).  Nothing here may be contracted into an FMA: the library is built with
// -ffp-contract=off, and a host build for a target without FMA instructions (the default) has none to contract to.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SDRX_SH_HD __host__ __device__
#else
#define SDRX_SH_HD
#endif

namespace sdrx {

constexpr int kShThread = 16;                    // samples per lane: one lane row of the tile layout
constexpr int kShThreads = 256;
constexpr int kShWg = kShThread * kShThreads;    // samples per workgroup: four tiles, a wave each
constexpr int kShTab = 256;                      // entries per table; three tables: A, B, C
constexpr uint32_t kShLoadPhase = 1u;            // SDRX_SHIFT_LOAD_PHASE
constexpr uint32_t kShNanBits = 0x7fc00000u;     // the one NaN a component is

struct ShiftCfg { // sdrx_shift_cfg of include/sdrx.h (the layout is asserted in sdrx.hip)
    uint32_t inc, phase0;
    uint32_t flags;
    uint32_t reserved[5];
};

struct ShiftC { // a cf32 value
    float re, im;
};

// nullptr, or why these settings are not offered (SDRX_EINVAL)
inline const char *shift_args(uint32_t flags, const uint32_t *reserved)
{
    if (flags & ~kShLoadPhase)
        return "flags: only bit 0 (SDRX_SHIFT_LOAD_PHASE) is defined";
    if (reserved && (reserved[0] | reserved[1] | reserved[2] | reserved[3] | reserved[4]))
        return "the reserved words must be 0";
    return nullptr;
}

// A[k] = (cos, sin)(2 pi k / 2^8), B[k] = (cos, sin)(2 pi k / 2^16), C[k] = (cos, sin)(2 pi k / 2^24): the C library's cos / sin
// in double, rounded once to float.  out: A | B | C, (re, im) interleaved.
inline void shift_tables(float out[3 * kShTab * 2])
{
    const double two_pi = 6.283185307179586476925286766559;
    const double denom[3] = {256.0, 65536.0, 16777216.0};
    for (int t = 0; t < 3; ++t)
        for (int k = 0; k < kShTab; ++k) {
            const double a = two_pi * (double)k / denom[t];
            out[(t * kShTab + k) * 2] = (float)std::cos(a);
            out[(t * kShTab + k) * 2 + 1] = (float)std::sin(a);
        }
}

// rint(hz / fs_tree 2^32) in double, ties to even, mod 2^32; false: not offered (non-finite, fs_tree <= 0, |hz| > fs_tree / 2)
inline bool shift_inc(double fs_tree, double hz, uint32_t *inc)
{
    if (!(fs_tree - fs_tree == 0.0) || !(hz - hz == 0.0) || !(fs_tree > 0.0) || !(std::fabs(hz) <= fs_tree / 2))
        return false;
    const double r = std::rint(hz / fs_tree * 4294967296.0); // |r| <= 2^31
    *inc = (uint32_t)(int64_t)r;
    return true;
}
// the signed inverse: inc as a two's complement number of fs_tree / 2^32
inline double shift_hz(double fs_tree, uint32_t inc) { return (double)(int32_t)inc * fs_tree / 4294967296.0; }

SDRX_SH_HD inline uint32_t shift_float_bits(float x)
{
    uint32_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u;
}
SDRX_SH_HD inline float shift_bits_float(uint32_t u)
{
    float x;
    __builtin_memcpy(&x, &u, sizeof x);
    return x;
}

// The indices of phase p: the high, the middle and the low byte of its top 24 bits.  The lowest 8 bits are dropped (truncated).
SDRX_SH_HD inline void shift_split(uint32_t p, int &h, int &m, int &l) { h = (int)(p >> 24), m = (int)((p >> 16) & 255u), l = (int)((p >> 8) & 255u); }

// a (x) b = ( fl(fl(ar br) - fl(ai bi)), fl(fl(ar bi) + fl(ai br)) )
SDRX_SH_HD inline ShiftC shift_mul(ShiftC a, ShiftC b)
{
    const float rr = a.re * b.re, ii = a.im * b.im, ri = a.re * b.im, ir = a.im * b.re;
    ShiftC y;
    y.re = rr - ii;
    y.im = ri + ir;
    return y;
}

// rot = (A[h] (x) B[m]) (x) C[l]
SDRX_SH_HD inline ShiftC shift_rot(const ShiftC *A, const ShiftC *B, const ShiftC *C, uint32_t p)
{
    int h, m, l;
    shift_split(p, h, m, l);
    return shift_mul(shift_mul(A[h], B[m]), C[l]);
}

// y = x (x) rot; a component that is a NaN is the quiet NaN 0x7fc00000, whatever produced it
SDRX_SH_HD inline ShiftC shift_apply(ShiftC x, ShiftC rot)
{
    ShiftC y = shift_mul(x, rot);
    if (!(y.re == y.re))
        y.re = shift_bits_float(kShNanBits);
    if (!(y.im == y.im))
        y.im = shift_bits_float(kShNanBits);
    return y;
}

// the phase behind a frame of n samples (and of sample j = n inside it): wrapping 32-bit arithmetic
SDRX_SH_HD inline uint32_t shift_advance(uint32_t phase, uint32_t n, uint32_t inc) { return phase + n * inc; }

inline int shift_workgroups(int n) { return (n + kShWg - 1) / kShWg; }

} // namespace sdrx
