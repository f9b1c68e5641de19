// sdrx_resample.h -- the rational resampler L/M in front of level 0 (include/sdrx.h "Resampler"): its ratio, its
// frame lengths, where output m reads the input (position) and what a chunk of 1024 outputs reads (window), and the built-in
// Kaiser design.  Plain C++: shared by the kernel (resample.hip), the library (sdrx_finalize.hip, sdrx.hip) and a stand-alone
// check (host/resample_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SDRX_RS_HD __host__ __device__
#else
#define SDRX_RS_HD
#endif

namespace sdrx {

constexpr int kRsChunk = 1024;      // outputs per workgroup: one tile of the tile layout
constexpr int kRsMaxL = 1024;       // phases
constexpr int kRsMinT = 8, kRsMaxT = 64; // taps per phase (a multiple of 4)
constexpr int kRsMaxTaps = 32768;   // L * T: the phase-major table is at most 128 KiB
constexpr int kRsHist = kRsMaxT;    // cf32 per slot of the history buffer (T - 1 are used)

struct ResamplePlan {
    int fs_in = 0, fs_out = 0;
    int L = 0, M = 0, T = 0;
    int n_in = 0, n_out = 0; // samples per frame at the input / the output rate (0: not decided yet)
};

inline long long rs_gcd(long long a, long long b)
{
    while (b) {
        const long long t = a % b;
        a = b, b = t;
    }
    return a;
}

// L = fs_out / g, M = fs_in / g.  nullptr, or why the ratio (with T taps per phase) is not offered.
inline const char *resample_ratio(int fs_in, int fs_out, int T, ResamplePlan &P)
{
    if (fs_in <= 0 || fs_out <= 0)
        return "sample rates must be positive";
    const long long g = rs_gcd(fs_in, fs_out);
    P.fs_in = fs_in, P.fs_out = fs_out, P.T = T;
    P.L = (int)(fs_out / g), P.M = (int)(fs_in / g);
    if (P.L > kRsMaxL)
        return "L = fs_out / gcd(fs_in, fs_out) exceeds 1024";
    if (2LL * P.M < P.L || P.M > 4LL * P.L)
        return "M / L outside 1/2 .. 4";
    if (T < kRsMinT || T > kRsMaxT || T % 4)
        return "taps_per_phase must be a multiple of 4 in 8 .. 64";
    if ((long long)P.L * T > kRsMaxTaps)
        return "L * taps_per_phase exceeds 32768";
    return nullptr;
}

// ... and the frame lengths for an output frame of n_out samples: n_in = n_out M / L.
inline const char *resample_frames(ResamplePlan &P, int n_out)
{
    if (n_out <= 0)
        return "the output frame must be positive";
    const long long p = (long long)n_out * P.M;
    if (p % P.L)
        return "n * M is not a multiple of L: a frame would not start at phase 0";
    const long long n_in = p / P.L;
    if (n_in % 16)
        return "the input frame n * M / L is not a multiple of 16";
    if (n_in < P.T || n_in >= (1LL << 31) - 2048)
        return "the input frame is shorter than taps_per_phase (or too long)";
    P.n_out = n_out, P.n_in = (int)n_in;
    return nullptr;
}

// Output m of a frame reads x[i - t], t = 0 .. T-1, with the taps of phase ph: p = m M in 64 bits, i = p div L, ph = p mod L.
SDRX_RS_HD inline void resample_pos(long long m, int M, int L, long long &i, int &ph)
{
    const long long p = m * (long long)M;
    i = p / L;
    ph = (int)(p - i * L);
}

// Chunk c (outputs 1024 c .. 1024 c + count - 1, count = min(1024, n_out - 1024 c)) reads the inputs lo .. hi:
//   lo = floor(1024 c M / L) - (T - 1),  hi = floor((1024 c + count - 1) M / L)
SDRX_RS_HD inline void resample_window(int c, int n_out, int M, int L, int T, long long &lo, long long &hi)
{
    const long long m0 = (long long)c * kRsChunk;
    const long long count = n_out - m0 < kRsChunk ? n_out - m0 : kRsChunk;
    int ph;
    resample_pos(m0, M, L, lo, ph);
    lo -= T - 1;
    resample_pos(m0 + count - 1, M, L, hi, ph);
}

// the longest window of any chunk of the frame, in samples
inline int resample_max_window(const ResamplePlan &P)
{
    long long w = 0;
    for (int c = 0; (long long)c * kRsChunk < P.n_out; ++c) {
        long long lo, hi;
        resample_window(c, P.n_out, P.M, P.L, P.T, lo, hi);
        if (hi - lo + 1 > w)
            w = hi - lo + 1;
    }
    return (int)w;
}

// The nearest valid pair to `seconds` of signal with the output frame a multiple of `multiple_of`: n_out = k L and n_in = k M
// with k a multiple of what makes n_in a multiple of 16 and n_out one of multiple_of; a tie goes to the shorter frame.
inline bool resample_nearest_frames(const ResamplePlan &P, double seconds, int multiple_of, int &n_in, int &n_out)
{
    if (multiple_of <= 0 || !(seconds > 0))
        return false;
    const long long k16 = 16 / rs_gcd(16, P.M), kmo = multiple_of / rs_gcd(multiple_of, P.L);
    const long long step = k16 / rs_gcd(k16, kmo) * kmo;
    const double q = seconds * (double)P.fs_out / ((double)step * P.L);
    long long j = (long long)std::floor(q);
    if (q - (double)j > 0.5)
        ++j;
    if (j < 1)
        j = 1;
    const long long k = j * step;
    if (k * P.M >= (1LL << 31) - 2048 || k * P.L >= (1LL << 31) - 2048)
        return false;
    n_in = (int)(k * P.M), n_out = (int)(k * P.L);
    return true;
}

inline double rs_bessel_i0(double x) // the power series: every term positive, converged to the last bit for x <= 13
{
    const double q = x * x / 4;
    double sum = 1, term = 1;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * k);
        sum += term;
        if (term < sum * 1e-18)
            break;
    }
    return sum;
}

// The built-in design, IEEE double rounded once to fp32 (include/sdrx.h).  0: fine; 1: atten_db outside (50, 120]; 2: the
// transition is wider than the band (fn - tw <= 0).  `taps` (L T floats, prototype order) may be null.
inline int resample_design(const ResamplePlan &P, double atten_db, float *taps, double *passband_hz)
{
    if (!(atten_db > 50.0 && atten_db <= 120.0))
        return 1;
    const double pi = 3.141592653589793238462643383279502884;
    const int N = P.L * P.T;
    const double beta = 0.1102 * (atten_db - 8.7);
    const double tw = (atten_db - 7.95) / (2.285 * (N - 1) * 2 * pi);
    const double fn = 0.5 / (P.L > P.M ? P.L : P.M);
    if (fn - tw <= 0)
        return 2;
    const double fc = fn - tw / 2;
    if (passband_hz)
        *passband_hz = (fn - tw) * P.L * (double)P.fs_in;
    if (!taps)
        return 0;
    const double i0b = rs_bessel_i0(beta), mid = (N - 1) / 2.0;
    for (int k = 0; k < N; ++k) {
        const double x = 2 * fc * (k - mid);
        const double sinc = x == 0 ? 1.0 : std::sin(pi * x) / (pi * x);
        const double r = 2.0 * k / (N - 1) - 1;
        const double arg = 1 - r * r;
        const double win = rs_bessel_i0(beta * std::sqrt(arg > 0 ? arg : 0)) / i0b;
        taps[k] = (float)(P.L * 2 * fc * sinc * win);
    }
    return 0;
}

inline double resample_delay(const ResamplePlan &P) { return ((double)P.L * P.T - 1) / (2.0 * P.M); }

} // namespace sdrx
