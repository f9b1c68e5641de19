// sdrx_detect.h -- the detector leaves (include/sdrx.h "Detector leaves"): the rules of their settings and the
// per-sample arithmetic of the AM envelope and the FM discriminator -- every step ONE fp32 operation, separately rounded, in one
// association and operand order.  Plain C++: shared by the kernels (detect.hip), the library (sdrx.hip, sdrx_finalize.hip) and a
// stand-alone check (host/detect_check.cpp).  Nothing here may be contracted into an FMA: the library is built with
// -ffp-contract=off, and a host build for a target without FMA instructions (the default) has none to contract to.  No call into
// the C library's mathematics: the square root and the division are the machine's correctly rounded ones, ANG is spelled out.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SDRX_DT_HD __host__ __device__
#else
#define SDRX_DT_HD
#endif

namespace sdrx {

constexpr int kDetNone = 0, kDetAm = 1, kDetFm = 2; // SDRX_DETECT_*
constexpr int kDetBlock = 4096;                     // samples per block of k_env_sum / k_detect (k_compress's geometry)
constexpr int kDetThreads = 256;

struct DetectCfg { // sdrx_detect_cfg of include/sdrx.h (the layout is asserted in sdrx.hip)
    int32_t kind;
    int32_t reserved[3];
};

// nullptr, or why these settings are not offered (SDRX_EINVAL)
inline const char *detect_args(const DetectCfg &d)
{
    if (d.kind != kDetNone && d.kind != kDetAm && d.kind != kDetFm)
        return "kind must be SDRX_DETECT_NONE, SDRX_DETECT_AM or SDRX_DETECT_FM";
    if (d.reserved[0] | d.reserved[1] | d.reserved[2])
        return "the reserved words must be 0";
    return nullptr;
}

inline int detect_blocks(int n) { return (n + kDetBlock - 1) / kDetBlock; }

SDRX_DT_HD inline float detect_abs(float x) { return __builtin_fabsf(x); }

// ---- AM ------------------------------------------------------------------------------------------------------------------------
// e = sqrt(fl(fl(re re) + fl(im im))): the correctly rounded fp32 square root
SDRX_DT_HD inline float detect_env(float re, float im)
{
    const float rr = re * re, ii = im * im;
    const float s = rr + ii;
    return __builtin_sqrtf(s);
}
// q = min(e, 2^15) 2^8 rounded to nearest even, as an unsigned integer (a NaN counts as 2^15).  t <= 2^23, so fl(t + 2^23) IS the
// rounding to an integer, ties to even, and the difference is exact.
SDRX_DT_HD inline uint32_t detect_env_q(float e)
{
    const float capped = e < 32768.0f ? e : 32768.0f;
    const float t = capped * 256.0f;
    const float r = (t + 8388608.0f) - 8388608.0f;
    return (uint32_t)r;
}
// c = (float)((double)S / (double)(256 n)), S = the sum of q over the leaf-frame's n samples
SDRX_DT_HD inline float detect_carrier(uint64_t S, int n) { return (float)((double)S / (double)(256ll * (long long)n)); }
// pre = fl(fl(e - c) gain)
SDRX_DT_HD inline float detect_am_pre(float e, float c, float gain)
{
    const float d = e - c;
    return d * gain;
}

// ---- FM ------------------------------------------------------------------------------------------------------------------------
// ANG(y, x): the angle of x + j y in half-turns, in [-1, 1].  Octant reduction to t = min / max of the magnitudes (one correctly
// rounded division), atan(t) / pi = t P(t^2) with P of degree 5 in separately rounded Horner steps (an interpolant at Chebyshev
// nodes refined to equal ripple: 5.3e-7 half-turns before rounding), then the octant, the half-plane and the sign by compares.
// ANG(0, 0) = 0; a zero of either sign counts as not negative.
SDRX_DT_HD inline float detect_ang(float y, float x)
{
    const float ay = detect_abs(y), ax = detect_abs(x);
    const bool swap = ay > ax;
    const float mx = swap ? ay : ax, mn = swap ? ax : ay;
    const float t = mx == 0.0f ? 0.0f : mn / mx;
    const float u = t * t;
    float p = -0x1.e8f086p-9f;
    p = p * u;
    p = p + 0x1.1290d2p-6f;
    p = p * u;
    p = p + -0x1.2f97cep-5f;
    p = p * u;
    p = p + 0x1.f8acc0p-5f;
    p = p * u;
    p = p + -0x1.b1ac38p-4f;
    p = p * u;
    p = p + 0x1.45f120p-2f;
    float r = t * p;
    if (swap)
        r = 0.5f - r;
    if (x < 0.0f)
        r = 1.0f - r;
    if (y < 0.0f)
        r = -r;
    return r;
}
// z = (a, b), the sample before it (p, q): d = z conj(z_prev), pre = fl(ANG(d_im, d_re) gain)
SDRX_DT_HD inline float detect_fm_pre(float a, float b, float p, float q, float gain)
{
    const float ap = a * p, bq = b * q, bp = b * p, aq = a * q;
    const float d_re = ap + bq;
    const float d_im = bp - aq;
    return detect_ang(d_im, d_re) * gain;
}

} // namespace sdrx
