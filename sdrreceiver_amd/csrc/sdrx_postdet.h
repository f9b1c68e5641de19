// sdrx_postdet.h -- the post-detection filter of the detector leaves (include/sdrx.h "Post-detection filter"): the
// rules of its settings, the per-output arithmetic of the FIR -- per tap a product rounded to fp32, then a sum rounded to fp32, taps
// ascending, the idiom of the resampler and the front stage -- and the Kaiser low-pass design.  Plain C++: shared by the kernel
// (postdet.hip), the library (sdrx.hip, sdrx_finalize.hip) and a stand-alone check (host/postdet_check.cpp).  Nothing here may be
// contracted into an FMA: the library is built with -ffp-contract=off, and a host build for a target without FMA instructions
// (the default) has none to contract to.
#pragma once

#include <cmath>
#include <cstdint>

#include "sdrx_resample.h" // rs_bessel_i0

#if defined(__HIPCC__)
#define SDRX_PD_HD __host__ __device__
#else
#define SDRX_PD_HD
#endif

namespace sdrx {

constexpr int kPdMaxTaps = 256; // 1 <= T <= 256
constexpr int kPdMaxDecim = 16; // 1 <= R <= 16

struct PostCfg { // sdrx_postfilter_cfg of include/sdrx.h (the layout is asserted in sdrx.hip)
    int32_t decim, ntaps;
    int32_t reserved[2];
};

// nullptr, or why these settings are not offered (SDRX_EINVAL).  ntaps = 0 takes the filter away: decim is not looked at then.
inline const char *postdet_args(const PostCfg &p)
{
    if (p.reserved[0] | p.reserved[1])
        return "the reserved words must be 0";
    if (p.ntaps == 0)
        return nullptr;
    if (p.ntaps < 1 || p.ntaps > kPdMaxTaps)
        return "ntaps must be 0 (no filter) or 1 .. 256";
    if (p.decim < 1 || p.decim > kPdMaxDecim)
        return "decim must be 1 .. 16";
    return nullptr;
}

// y[m] of the definition: `at` points at pre[m R] and may be read T - 1 floats back.
//   acc_0 = +0.0f;  acc_{t+1} = fl(acc_t + fl(h[t] pre[m R - t])),  t ascending
SDRX_PD_HD inline float postdet_fir(const float *h, int T, const float *at)
{
    float acc = 0.0f;
    for (int t = 0; t < T; ++t) {
        const float p = h[t] * at[-t];
        acc = acc + p;
    }
    return acc;
}

// The built-in design, IEEE double rounded once to fp32 (include/sdrx.h).  0: fine; 1: atten_db outside (50, 120] or ntaps
// outside 1 .. 256 or fs, cutoff not positive; 2: the transition does not fit (fc - tw/2 <= 0 or fc + tw/2 > 0.5).  `taps` (N
// floats) may be null.
inline int postdet_design(double fs, double cutoff_hz, int N, double atten_db, float *taps, double *pass_hz, double *stop_hz)
{
    if (!(atten_db > 50.0 && atten_db <= 120.0) || N < 1 || N > kPdMaxTaps || !(fs > 0.0) || !(cutoff_hz > 0.0))
        return 1;
    if (N == 1)
        return 2; // (the transition of one tap is the whole band)
    const double pi = 3.141592653589793238462643383279502884;
    const double beta = 0.1102 * (atten_db - 8.7);
    const double tw = (atten_db - 7.95) / (2.285 * (N - 1) * 2 * pi);
    const double fc = cutoff_hz / fs;
    if (!(fc - tw / 2 > 0) || !(fc + tw / 2 <= 0.5))
        return 2;
    if (pass_hz)
        *pass_hz = (fc - tw / 2) * fs;
    if (stop_hz)
        *stop_hz = (fc + tw / 2) * fs;
    if (!taps)
        return 0;
    const double i0b = rs_bessel_i0(beta), mid = (N - 1) / 2.0;
    double h[kPdMaxTaps], sum = 0;
    for (int k = 0; k < N; ++k) {
        const double x = 2 * fc * (k - mid);
        const double sinc = x == 0 ? 1.0 : std::sin(pi * x) / (pi * x);
        const double r = 2.0 * k / (N - 1) - 1;
        const double arg = 1 - r * r;
        const double win = rs_bessel_i0(beta * std::sqrt(arg > 0 ? arg : 0)) / i0b;
        h[k] = 2 * fc * sinc * win;
        sum += h[k]; // (k ascending: the order is part of the definition)
    }
    for (int k = 0; k < N; ++k)
        taps[k] = (float)(h[k] / sum);
    return 0;
}

} // namespace sdrx
