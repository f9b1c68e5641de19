// sdrx_blank.h -- the impulse blanker in front of the front stage, the resampler or level 0 (include/sdrx.h "Impulse blanker",
// DESIGN.md 4u): the rules of its four settings, the power bins and their edges, the threshold, the rank rule that picks the next
// reference bin, the carry between frames, and the geometry of k_blank.  Plain C++: shared by the kernels (blank.hip), the launch
// code (sdrx_frame.hip), the library (sdrx.hip, sdrx_finalize.hip) and a stand-alone check (host/blank_check.cpp).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SDRX_BLANK_HD __host__ __device__
#else
#define SDRX_BLANK_HD
#endif

namespace sdrx {

constexpr int kBlankBins = 2048;                       // bin(p) = (bits(p) & 0x7fffffff) >> 20
constexpr int kBlankMaxBin = 2040;                     // the bin of +inf: the highest a reference takes
constexpr int kBlankMaxGuard = 64;
constexpr int kBlankNoHit = kBlankMaxGuard + 1;        // tail_gap of a frame without a hit (and the most it is stored as)
constexpr int kBlankThread = 16;                       // samples per lane: one lane row of the tile layout
constexpr int kBlankThreads = 256;
constexpr int kBlankWg = kBlankThread * kBlankThreads; // samples per workgroup: four tiles, a wave each
constexpr int kBlankHalo = 128;                        // samples of hit bitmap on either side of a workgroup (>= guard + 1), two 64-bit words
constexpr uint32_t kBlankInfBits = 0x7f800000u;

struct BlankCfg { // sdrx_blanker_cfg of include/sdrx.h (the layout is asserted in sdrx.hip)
    float ratio, floor;
    int32_t rank_q16, guard;
    int32_t reserved[4];
};

// nullptr, or why these settings are not offered (SDRX_EINVAL).  (x - x == 0 holds for finite x only.)
inline const char *blank_args(float ratio, float floor, int rank_q16, int guard)
{
    if (!(ratio - ratio == 0.0f) || !(ratio >= 1.0f))
        return "ratio must be finite and at least 1";
    if (!(floor - floor == 0.0f) || !(floor >= 0.0f))
        return "floor must be finite and at least 0";
    if (rank_q16 < 1 || rank_q16 > 65536)
        return "rank_q16 must be in 1 .. 65536 (32768: the median)";
    if (guard < 0 || guard > kBlankMaxGuard)
        return "guard must be in 0 .. 64";
    return nullptr;
}

SDRX_BLANK_HD inline uint32_t blank_float_bits(float x)
{
    uint32_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u;
}
SDRX_BLANK_HD inline float blank_bits_float(uint32_t u)
{
    float x;
    __builtin_memcpy(&x, &u, sizeof x);
    return x;
}
SDRX_BLANK_HD inline int blank_bin(float p) { return (int)((blank_float_bits(p) & 0x7fffffffu) >> 20); }
// the bin's lower edge: the float whose bits are b << 20
SDRX_BLANK_HD inline float blank_edge(int b) { return blank_bits_float((uint32_t)b << 20); }

// The threshold a frame uses: +inf before the first reference, else max(fl(ratio * edge(ref_bin)), floor).  (One product and one
// comparison: nothing a contraction could fuse.)
SDRX_BLANK_HD inline float blank_threshold(int ref_bin, float ratio, float floor)
{
    if (ref_bin < 0)
        return blank_bits_float(kBlankInfBits);
    const float t = ratio * blank_edge(ref_bin);
    return t > floor ? t : floor;
}

// Whether the bins up to one whose cumulative count is `cum` hold the rank: 65536 cum >= rank_q16 n, in 64-bit unsigned
SDRX_BLANK_HD inline bool blank_rank_reached(uint64_t cum, uint32_t n, uint32_t rank_q16) { return 65536ull * cum >= (uint64_t)rank_q16 * n; }

// The next reference: min(2040, the smallest b whose cumulative count holds the rank); the histogram holds n samples
inline int blank_rank_bin(const uint32_t *hist, uint32_t n, uint32_t rank_q16)
{
    uint64_t cum = 0;
    for (int b = 0; b < kBlankBins; ++b) {
        cum += hist[b];
        if (blank_rank_reached(cum, n, rank_q16))
            return b < kBlankMaxBin ? b : kBlankMaxBin;
    }
    return kBlankMaxBin; // (a histogram that holds fewer than n samples)
}

// What a frame of n samples leaves for the next: the distance from its last sample to its last hit (last_hit < 0: none), at most
// kBlankNoHit, which no guard reaches
SDRX_BLANK_HD inline int blank_tail_gap(int n, int last_hit)
{
    if (last_hit < 0)
        return kBlankNoHit;
    const int gap = n - 1 - last_hit;
    return gap < kBlankNoHit ? gap : kBlankNoHit;
}
// The samples at the start of a frame that the previous frame's last hit still blanks: j <= guard - 1 - tail_gap
SDRX_BLANK_HD inline int blank_carry_in(int n, int guard, int tail_gap)
{
    const int k = guard - tail_gap;
    return k <= 0 ? 0 : k < n ? k : n;
}

inline int blank_workgroups(int n) { return (n + kBlankWg - 1) / kBlankWg; }

} // namespace sdrx
