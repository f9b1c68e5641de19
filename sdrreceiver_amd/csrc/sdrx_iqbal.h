// sdrx_iqbal.h -- the IQ balance correction behind the format conversion and the DC removal (include/sdrx.h "IQ balance", DESIGN.md
// 4w): the rules of its settings, the quantiser q() of the statistics, the step that moves the pair (c, d) from a frame's five
// integer sums (rule 4: every operation one IEEE double operation, in the order written), and the geometry of k_iqbal.  Plain C++:
// shared by the kernels (iqbal.hip), the launch code (sdrx_frame.hip), the library (sdrx.hip, sdrx_finalize.hip) and a stand-alone
// check (host/iq_check.cpp).  Nothing here may be contracted into an FMA: the library is built with -ffp-contract=off, and a host
// build for a target without FMA instructions (the default) has none to contract to.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SDRX_IQ_HD __host__ __device__
#else
#define SDRX_IQ_HD
#endif

namespace sdrx {

constexpr int kIqThread = 16;                    // samples per lane: one lane row of the tile layout
constexpr int kIqThreads = 256;
constexpr int kIqWg = kIqThread * kIqThreads;    // samples per workgroup: four tiles, a wave each
constexpr int kIqClamp = 32767;                  // |q(x)| at the most
constexpr uint32_t kIqLoad = 1u;                 // SDRX_IQ_LOAD
constexpr uint32_t kIqNanBits = 0x7fc00000u;     // the one NaN a Q' is
constexpr float kIqMaxC = 0.5f, kIqMinD = 0.5f, kIqMaxD = 2.0f;

struct IqCfg { // sdrx_iq_cfg of include/sdrx.h (the layout is asserted in sdrx.hip)
    float mu, min_power, c0, d0;
    uint32_t flags;
    uint32_t reserved[3];
};

struct IqSums { // rule 3, of q(I'), q(Q')
    int64_t s_i, s_q, s_iq;
    uint64_t s_ii, s_qq;
};

struct IqStep { // what rule 4 leaves
    float c_next, d_next;
    uint32_t measured, adapted, rejected;
};

// nullptr, or why these settings are not offered (SDRX_EINVAL).  (x - x == 0 holds for finite x only.)
inline const char *iq_args(float mu, float min_power, float c0, float d0, uint32_t flags, const uint32_t *reserved)
{
    if (!(mu >= 0.0f) || !(mu <= 1.0f))
        return "mu must be in 0 .. 1 (0: hold)";
    if (!(min_power - min_power == 0.0f) || !(min_power >= 0.0f))
        return "min_power must be finite and at least 0";
    if (!(c0 >= -kIqMaxC) || !(c0 <= kIqMaxC))
        return "c0 must be in -0.5 .. 0.5";
    if (!(d0 >= kIqMinD) || !(d0 <= kIqMaxD))
        return "d0 must be in 0.5 .. 2";
    if (flags & ~kIqLoad)
        return "flags: only bit 0 (SDRX_IQ_LOAD) is defined";
    if (reserved && (reserved[0] | reserved[1] | reserved[2]))
        return "the reserved words must be 0";
    return nullptr;
}

SDRX_IQ_HD inline uint32_t iq_float_bits(float x)
{
    uint32_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u;
}
SDRX_IQ_HD inline float iq_bits_float(uint32_t u)
{
    float x;
    __builtin_memcpy(&x, &u, sizeof x);
    return x;
}

// Rule 2: 0 for NaN, else round-to-nearest-even of fl(x 256) (exact, or +-inf), saturated to +-32767
SDRX_IQ_HD inline int iq_q(float x)
{
    const float v = x * 256.0f;
    if (!(v == v))
        return 0;
    if (v >= (float)kIqClamp)
        return kIqClamp;
    if (v <= -(float)kIqClamp)
        return -kIqClamp;
    return (int)__builtin_rintf(v); // (round to nearest even: the default rounding mode, v_rndne_f32 on the device)
}

SDRX_IQ_HD inline bool iq_pair_ok(float c, float d)
{
    return c - c == 0.0f && d - d == 0.0f && c >= -kIqMaxC && c <= kIqMaxC && d >= kIqMinD && d <= kIqMaxD;
}

// Rule 4.  One IEEE double operation per line element; conversions of 64-bit integers to double round to nearest even.
SDRX_IQ_HD inline IqStep iq_step(const IqSums &S, uint32_t n, float mu, float min_power, float c, float d)
{
    IqStep r;
    r.c_next = c, r.d_next = d;
    r.measured = r.adapted = r.rejected = 0u;
    const double N = (double)n;
    const double mi = (double)S.s_i / N;
    const double mq = (double)S.s_q / N;
    const double ii = (double)S.s_ii / N, mimi = mi * mi;
    const double A = ii - mimi;
    const double qq = (double)S.s_qq / N, mqmq = mq * mq;
    const double B = qq - mqmq;
    const double iq = (double)S.s_iq / N, mimq = mi * mq;
    const double C = iq - mimq;
    const double AB = A + B;
    const double pw = AB * (1.0 / 65536.0); // (a power of two: exact)
    if (!(A > 0.0 && B > 0.0 && pw >= (double)min_power))
        return r;
    r.measured = 1u;
    if (!(mu > 0.0f))
        return r;
    const double m = (double)mu;
    const double ep = C / A;
    const double AmB = A - B;
    const double eg = AmB / AB;
    const double meg = m * eg;
    const double g = 1.0 + meg;
    const double mep = m * ep;
    const double cm = (double)c - mep;
    const double gc = g * cm;
    const double gd = g * (double)d;
    const float cn = (float)gc, dn = (float)gd;
    if (iq_pair_ok(cn, dn)) {
        r.c_next = cn, r.d_next = dn;
        r.adapted = 1u;
    } else {
        r.rejected = 1u;
    }
    return r;
}

inline int iq_workgroups(int n) { return (n + kIqWg - 1) / kIqWg; }

} // namespace sdrx
