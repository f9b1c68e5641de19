// sdrx_notch.h -- the spur canceller in front of the frequency shift (include/sdrx.h "Spur canceller"): the rules of
// its settings with the spacing rule, the geometry of its kernels, the order of the block correlation's sums (lane, wave tree, four
// waves) and the step rule of a tone over a frame's blocks (amplitude loop, frequency estimate, frame end).  Plain C++: shared by
// the kernels (notch.hip), the launch code (sdrx_frame.hip), the library (sdrx.hip, sdrx_finalize.hip) and a stand-alone check
// (host/notch_check.cpp).  The oscillator is the shift's (sdrx_shift.h: tables, index split, product).  Nothing here may be
// contracted into an FMA: the library is built with -ffp-contract=off, and a host build for a target without FMA instructions
// (the default) has none to contract to.
#pragma once

#include "sdrx_shift.h"

namespace sdrx {

constexpr int kNtMax = 8;                        // SDRX_NOTCH_MAX: tone slots
constexpr int kNtBlock = kShWg;                  // L: samples per block, one workgroup of k_shift's geometry
constexpr int kNtThreads = kShThreads;
constexpr int kNtLane = kShThread;               // samples per lane
constexpr uint32_t kNtSpacing = 1u << 23;        // 8 2^32 / L: two tones closer than this (circular distance of inc0) are refused
constexpr uint32_t kNtLoad = 1u;                 // SDRX_NOTCH_LOAD
constexpr double kNtRadToInc = 166886.05360752725; // 2^20 / (2 pi) = 2^32 / (2 pi L): one radian of rotation per block, in inc units

struct NotchCfg { // sdrx_notch_cfg of include/sdrx.h (the layout is asserted in sdrx.hip)
    uint32_t n_tones, flags, max_pull, reserved0;
    float mu, afc_gain, min_coherence;
    uint32_t reserved1;
    uint32_t inc0[kNtMax];
    uint32_t reserved[8];
};

struct NotchTone { // a slot's state on the device; (0, inc0, 0) at sdrx_finalize
    uint32_t phase, inc, inc0; // of the next frame
    float a_re, a_im;
    uint32_t phase_used, inc_used; // what the last frame's k_notch_step found: k_notch_apply behind it reads these
    uint32_t pad;
};

struct NotchToneRecord { // sdrx_notch_tone
    uint32_t inc, inc_next;
    uint32_t a_re_bits, a_im_bits;
    uint32_t coherent, adapted, clamped, rejected;
    double s_re, s_im, p, e;
};

struct NotchRecord { // sdrx_notch_record
    int64_t frame;
    uint32_t n_complex, n_tones, blocks;
    uint32_t reserved[3];
    NotchToneRecord tone[kNtMax];
};

struct NotchLoad { // what k_notch_load writes: by value, no host buffer outlives the call
    uint32_t inc0[kNtMax];
    uint32_t restart; // bit k: slot k starts at (0, inc0[k], 0)
};

// circular distance of two increments
SDRX_SH_HD inline uint32_t notch_distance(uint32_t a, uint32_t b)
{
    const uint32_t d = a - b, e = b - a;
    return d < e ? d : e;
}

// nullptr, or why these settings are not offered (SDRX_EINVAL)
inline const char *notch_args(const NotchCfg &c)
{
    if (c.n_tones > (uint32_t)kNtMax)
        return "n_tones must lie in 0 .. SDRX_NOTCH_MAX";
    if (!(c.mu > 0.0f && c.mu <= 1.0f))
        return "mu must lie in (0, 1]";
    if (!(c.afc_gain >= 0.0f && c.afc_gain <= 1.0f))
        return "afc_gain must lie in [0, 1]";
    if (!(c.min_coherence > 0.0f && c.min_coherence <= 1.0f))
        return "min_coherence must lie in (0, 1]";
    if (c.flags & ~kNtLoad)
        return "flags: only bit 0 (SDRX_NOTCH_LOAD) is defined";
    uint32_t r = c.reserved0 | c.reserved1;
    for (int i = 0; i < 8; ++i)
        r |= c.reserved[i];
    for (int k = (int)c.n_tones; k < kNtMax; ++k)
        r |= c.inc0[k];
    if (r)
        return "the reserved words and the unused tone slots must be 0";
    for (int i = 0; i < (int)c.n_tones; ++i)
        for (int j = i + 1; j < (int)c.n_tones; ++j)
            if (notch_distance(c.inc0[i], c.inc0[j]) < kNtSpacing)
                return "two tones are closer than 2^23 increment units (8 blocks' resolution): a block correlation cannot tell them apart";
    return nullptr;
}

// The slots a change of the tone list restarts at (0, inc0, 0): all under SDRX_NOTCH_LOAD, else the new ones and those whose inc0 changed
inline uint32_t notch_restart_mask(const NotchCfg &before, const NotchCfg &after)
{
    uint32_t m = 0;
    for (int k = 0; k < (int)after.n_tones; ++k)
        if ((after.flags & kNtLoad) || k >= (int)before.n_tones || before.inc0[k] != after.inc0[k])
            m |= 1u << k;
    return m;
}

SDRX_SH_HD inline int notch_blocks(int n) { return (n + kNtBlock - 1) / kNtBlock; }
SDRX_SH_HD inline int notch_block_len(int n, int b) { return n - b * kNtBlock < kNtBlock ? n - b * kNtBlock : kNtBlock; }

// t = x (x) conj(rot): the conjugate is exact
SDRX_SH_HD inline ShiftC notch_corr_term(ShiftC x, ShiftC rot) { return shift_mul(x, ShiftC{rot.re, -rot.im}); }

// The wave's sum of 64 lane values: at distance s = 1, 2, 4, .., 32, lane l with l mod 2s = 0 takes fl(v[l] + v[l + s]); v[0] is the sum.
// (k_notch_corr does it with __shfl_down in every lane: a lane with l mod 2s = 0 reads a lane with (l + s) mod s = 0, whose value is
// this rule's, so lane 0 ends with the same sum.)
inline float notch_wave_sum(float v[64])
{
    for (int s = 1; s < 64; s *= 2)
        for (int l = 0; l < 64; l += 2 * s)
            v[l] = v[l] + v[l + s];
    return v[0];
}
// ... and the four waves of a workgroup
SDRX_SH_HD inline float notch_wg_sum(float w0, float w1, float w2, float w3)
{
    const float a = w0 + w1, b = w2 + w3;
    return a + b;
}

// c[b][k] of one block (host: the definition written out; k_notch_corr computes the same sums in the same order): x -- the block's
// len samples, p0 -- the phase of its first sample
inline ShiftC notch_block_corr(const ShiftC *x, int len, const ShiftC *A, const ShiftC *B, const ShiftC *C, uint32_t p0, uint32_t inc)
{
    float wr[4], wi[4];
    for (int w = 0; w < 4; ++w) {
        float vr[64], vi[64];
        for (int l = 0; l < 64; ++l) {
            float sr = 0.0f, si = 0.0f;
            const int s0 = (w * 64 + l) * kNtLane;
            for (int j = s0; j < s0 + kNtLane && j < len; ++j) {
                const ShiftC t = notch_corr_term(x[j], shift_rot(A, B, C, p0 + (uint32_t)j * inc));
                sr = sr + t.re;
                si = si + t.im;
            }
            vr[l] = sr, vi[l] = si;
        }
        wr[w] = notch_wave_sum(vr), wi[w] = notch_wave_sum(vi);
    }
    return ShiftC{notch_wg_sum(wr[0], wr[1], wr[2], wr[3]), notch_wg_sum(wi[0], wi[1], wi[2], wi[3])};
}

// y <- fl(y - (used (x) rot)) per component
SDRX_SH_HD inline ShiftC notch_subtract(ShiftC y, ShiftC used, ShiftC rot)
{
    const ShiftC q = shift_mul(used, rot);
    return ShiftC{y.re - q.re, y.im - q.im};
}
// a component that is a NaN is the quiet NaN 0x7fc00000
SDRX_SH_HD inline ShiftC notch_canonical(ShiftC y)
{
    if (!(y.re == y.re))
        y.re = shift_bits_float(kShNanBits);
    if (!(y.im == y.im))
        y.im = shift_bits_float(kShNanBits);
    return y;
}

// One tone over a frame of n samples: c and used point at the tone's entry of block 0 (stride kNtMax).  The amplitude loop (every
// operation one IEEE double operation in the written order), the frequency estimate over the full blocks, the frame end.
SDRX_SH_HD inline void notch_step_tone(const ShiftC *c, ShiftC *used, int n, NotchTone &T, float mu_f, float afc_f, float coh_f, uint32_t max_pull,
                                       NotchToneRecord &R)
{
    const int blocks = notch_blocks(n), nfull = n / kNtBlock;
    const double mu = (double)mu_f, afc = (double)afc_f, coh = (double)coh_f;
    float ar = T.a_re, ai = T.a_im;
    double s_re = 0.0, s_im = 0.0, p = 0.0, e = 0.0, pr = 0.0, pi = 0.0;
    uint32_t rejected = 0;
    for (int b = 0; b < blocks; ++b) {
        const double lb = (double)notch_block_len(n, b);
        const double mr = (double)c[b * kNtMax].re / lb, mi = (double)c[b * kNtMax].im / lb;
        used[b * kNtMax] = ShiftC{ar, ai};
        if (b >= 1 && b < nfull) {
            const double x1 = mr * pr, x2 = mi * pi, x3 = mi * pr, x4 = mr * pi, x5 = mr * mr, x6 = mi * mi;
            const double t1 = x1 + x2, t2 = x3 - x4, t3 = x5 + x6;
            s_re = s_re + t1, s_im = s_im + t2, p = p + t3;
            const double dr = mr - (double)ar, di = mi - (double)ai;
            const double y1 = dr * dr, y2 = di * di;
            const double t4 = y1 + y2;
            e = e + t4;
        }
        pr = mr, pi = mi;
        const double ur = mr - (double)ar, ui = mi - (double)ai;
        const double vr = mu * ur, vi = mu * ui;
        float nr = (float)((double)ar + vr), ni = (float)((double)ai + vi);
        if (!(nr - nr == 0.0f) || !(ni - ni == 0.0f)) {
            nr = 0.0f, ni = 0.0f;
            ++rejected;
        }
        ar = nr, ai = ni;
    }
    const uint32_t inc = T.inc;
    uint32_t inc_next = inc, coherent = 0, adapted = 0, clamped = 0;
    if (nfull >= 2) {
        coherent = (s_re > 0.0 && s_re >= coh * p) ? 1u : 0u;
        if (coherent && afc > 0.0) {
            double r = s_im / s_re;
            r = r > 1.0 ? 1.0 : r;
            r = r >= -1.0 ? r : -1.0; // (a NaN is -1)
            const double g = afc * r;
            const double d = __builtin_rint(g * kNtRadToInc); // ties to even
            inc_next = inc + (uint32_t)(int64_t)d;
            adapted = 1;
            const int64_t off = (int64_t)(int32_t)(inc_next - T.inc0);
            if (off > (int64_t)max_pull)
                inc_next = T.inc0 + max_pull, clamped = 1;
            else if (off < -(int64_t)max_pull)
                inc_next = T.inc0 - max_pull, clamped = 1;
        }
    }
    R.inc = inc, R.inc_next = inc_next;
    R.a_re_bits = shift_float_bits(ar), R.a_im_bits = shift_float_bits(ai);
    R.coherent = coherent, R.adapted = adapted, R.clamped = clamped, R.rejected = rejected;
    R.s_re = s_re, R.s_im = s_im, R.p = p, R.e = e;
    T.phase_used = T.phase, T.inc_used = inc;
    T.phase = shift_advance(T.phase, (uint32_t)n, inc);
    T.inc = inc_next;
    T.a_re = ar, T.a_im = ai;
}

inline int notch_workgroups(int n) { return notch_blocks(n); }

} // namespace sdrx
