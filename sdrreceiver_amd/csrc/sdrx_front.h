// sdrx_front.h -- the half-band front stage in front of the resampler or of level 0 (include/sdrx.h "Front stage"):
// its frame lengths per stage, what a tile of 1024 outputs reads (window), where an output reads inside it, and the built-in
// Kaiser half-band design.  Plain C++: shared by the kernel's launch code (front.hip, sdrx_frame.hip), the library
// (sdrx_finalize.hip, sdrx.hip) and a stand-alone check (host/front_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#include "sdrx_resample.h" // rs_bessel_i0

namespace sdrx {

constexpr int kFrTile = 1024;               // outputs per workgroup: one tile of the tile layout
constexpr int kFrMinK = 2, kFrMaxK = 31;    // the prototype has N = 4 K + 3 taps
constexpr int kFrMaxStages = 3;
constexpr int kFrMaxN = 4 * kFrMaxK + 3;    // 127
constexpr int kFrHist = 128;                // samples per slot of a stage's history buffer (N - 1 <= 126 are used)
constexpr int kFrMaxWindow = 2 * kFrTile + kFrMaxN - 1; // 2174: the longest window of a tile
constexpr int kFrWinHalf = (kFrMaxWindow + 1) / 2;      // ... held in LDS as its even and its odd positions

struct FrontPlan {
    int real = 0, stages = 0, K = 0;
    int n0 = 0;       // the frame the stage feeds (0: not decided yet)
    int in_frame = 0; // n0 * 2^stages: what a frame call takes
};

inline int front_taps(int K) { return 4 * K + 3; }
inline int front_centre(int K) { return 2 * K + 1; }

// nullptr, or why these arguments are not offered (SDRX_EINVAL)
inline const char *front_args(int real_input, int stages, int K)
{
    if (real_input != 0 && real_input != 1)
        return "real_input must be 0 or 1";
    if (stages < 1 || stages > kFrMaxStages)
        return "stages must be 1, 2 or 3";
    if (K < kFrMinK || K > kFrMaxK)
        return "K must be in 2 .. 31 (N = 4 K + 3 taps)";
    return nullptr;
}

// every odd k != C must be +0.0f, bit for bit: -1, or the first k that is not
inline int front_bad_tap(const float *h, int K)
{
    const int N = front_taps(K), C = front_centre(K);
    for (int k = 1; k < N; k += 2) {
        if (k == C)
            continue;
        uint32_t u;
        static_assert(sizeof u == sizeof(float), "fp32");
        __builtin_memcpy(&u, h + k, sizeof u);
        if (u != 0u)
            return k;
    }
    return -1;
}

// Stage s (1 = the one that reads the caller's samples, `stages` = the last) has n0 2^(stages - s) outputs, twice as many inputs.
inline long long front_stage_out(const FrontPlan &P, int s) { return (long long)P.n0 << (P.stages - s); }
inline long long front_stage_in(const FrontPlan &P, int s) { return 2 * front_stage_out(P, s); }

// ... and the frame lengths for a fed frame of n0 samples
inline const char *front_frames(FrontPlan &P, int n0)
{
    if (n0 <= 0 || n0 % 16)
        return "the frame behind the stage must be a positive multiple of 16";
    const long long in = (long long)n0 << P.stages;
    if (in >= (1LL << 31) - 4096)
        return "the incoming frame is too long";
    if (2LL * n0 < front_taps(P.K) - 1)
        return "the last stage's input is shorter than the filter's history";
    P.n0 = n0, P.in_frame = (int)in;
    return nullptr;
}

// Tile c of a stage with n_out outputs (outputs 1024 c .. 1024 c + count - 1, count = min(1024, n_out - 1024 c)) reads the
// stage's inputs lo .. hi:  lo = 2 * 1024 c - (N - 1),  hi = 2 (1024 c + count - 1).  Output m reads z[2m - k], k = 0 .. N-1.
inline void front_window(int c, long long n_out, int N, long long &lo, long long &hi)
{
    const long long m0 = (long long)c * kFrTile;
    const long long count = n_out - m0 < kFrTile ? n_out - m0 : kFrTile;
    lo = 2 * m0 - (N - 1);
    hi = 2 * (m0 + count - 1);
}

// Inside the kernel the window lies in LDS as its even positions E[w / 2] and its odd ones O[w / 2], w = idx - lo (N - 1 is even,
// so even taps read E and the centre tap reads O): local output j reads, for the even tap k = 2 i, E[j + 2K + 1 - i], and for
// the centre tap O[j + K].
inline int front_even_slot(int j, int i, int K) { return j + 2 * K + 1 - i; }
inline int front_odd_slot(int j, int K) { return j + K; }

// The built-in design, IEEE double rounded once to fp32 (include/sdrx.h).  0: fine; 1: atten_db outside (50, 120]; 2: the
// transition is wider than the band (0.25 - tw / 2 <= 0).  `taps` (N floats) may be null.
inline int front_design(int K, double atten_db, float *taps, double *tw_out)
{
    if (!(atten_db > 50.0 && atten_db <= 120.0))
        return 1;
    const double pi = 3.141592653589793238462643383279502884;
    const int N = front_taps(K), C = front_centre(K);
    const double beta = 0.1102 * (atten_db - 8.7);
    const double tw = (atten_db - 7.95) / (2.285 * (N - 1) * 2 * pi);
    if (0.25 - tw / 2 <= 0)
        return 2;
    if (tw_out)
        *tw_out = tw;
    if (!taps)
        return 0;
    const double i0b = rs_bessel_i0(beta);
    for (int k = 0; k < N; ++k) {
        if (k != C && (k & 1)) {
            taps[k] = 0.0f;
            continue;
        }
        const double x = 0.5 * (k - C);
        const double sinc = x == 0 ? 1.0 : std::sin(pi * x) / (pi * x);
        const double r = 2.0 * k / (N - 1) - 1;
        const double arg = 1 - r * r;
        const double win = rs_bessel_i0(beta * std::sqrt(arg > 0 ? arg : 0)) / i0b;
        taps[k] = (float)(0.5 * sinc * win);
    }
    return 0;
}

} // namespace sdrx
