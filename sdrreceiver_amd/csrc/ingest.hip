// ingest.hip -- the raw frame's way into the tile layout (sdrx_dev.h): k_ingest_f32, and for frames of integer samples one
// family of kernels templated on the format (include/sdrx.h: SDRX_FMT_CU8, floats[b] = b - 127 of jonti/sdr.cpp:43-49,122-129 and
// sdrj.cpp:155-160; SDRX_FMT_CS8 / SDRX_FMT_CS16, a wideband front end's signed samples) -- k_ingest_samples, and the DC-bias
// removal of sdrj::demodData (sdrj.cpp:271-286): bit-exact as k_dc_products -> k_dc_chain | k_dc_chain_spec -> k_dc_apply, in the
// tolerance arithmetic as k_dc_block_sums -> k_ingest_dc_fast -- with the DPP scans that only these kernels use.  What differs
// between the formats is how four floats are made out of one or two 32-bit words (sample_pair); the chain kernels, which only
// ever see products, are no templates.
// Relies on dev_helpers.hip (cu8_pair, gldv4, gldv4u, gst2, v16f) and on tile_unit (sdrx_dev.h).

// ------------------------------------------------------------------------------------ ingest
// natural cf32 frame -> tile layout (host-fed / broadcast raw frames enter the pipeline here)
__global__ __launch_bounds__(256) void k_ingest_f32(const float4 *__restrict__ nat, float4 *__restrict__ tiled, int n_pairs)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pairs)
        return;
    const int c = p >> 9, r = p & 511;
    tiled[tile_unit(c, r & 7, r >> 3)] = nat[p];
}

// Integer samples (include/sdrx.h, SDRX_FMT_*) -> cf32 in the reference's units, "dongle LSB, |x| <= 128": dongle bytes b - 127
// (cu8_pair), int8 of a wideband front end as it is, int16 times 2^-8 (an exact scaling: 16 significant bits, no rounding).
// One definition of a pair of complex samples for every kernel that reads such a frame; FMT is the header's constant.  A pair
// is one 32-bit word of the 8-bit formats and two of int16 (pair_words: .y unused for the former).
// The sample is computed FIRST and everything else from it -- fl(1e-6f * x) below is a product of x, never of b or v.
template <int FMT>
__device__ __forceinline__ float4 decode_pair(uint2 w)
{
    static_assert(FMT == SDRX_FMT_CU8 || FMT == SDRX_FMT_CS8 || FMT == SDRX_FMT_CS16, "a format of include/sdrx.h");
    if constexpr (FMT == SDRX_FMT_CU8) {
        return cu8_pair(w.x);
    } else if constexpr (FMT == SDRX_FMT_CS8) {
        return make_float4((float)(signed char)(w.x & 255u), (float)(signed char)((w.x >> 8) & 255u), (float)(signed char)((w.x >> 16) & 255u),
                           (float)((int)w.x >> 24));
    } else {
        const float s = 0.00390625f; // 2^-8
        return make_float4((float)(short)(w.x & 0xffffu) * s, (float)((int)w.x >> 16) * s, (float)(short)(w.y & 0xffffu) * s,
                           (float)((int)w.y >> 16) * s);
    }
}
template <int FMT>
__device__ __forceinline__ uint2 pair_words(const unsigned *__restrict__ words, int p) // the words of complex samples 2 p and 2 p + 1
{
    if constexpr (FMT == SDRX_FMT_CS16)
        return reinterpret_cast<const uint2 *>(words)[p];
    else
        return make_uint2(words[p], 0u);
}
template <int FMT>
__device__ __forceinline__ float4 sample_pair(const unsigned *__restrict__ words, int p) // complex samples 2 p and 2 p + 1
{
    return decode_pair<FMT>(pair_words<FMT>(words, p));
}
// ... and out of 16-byte units a thread has loaded itself: pair e of unit q (4 pairs of the 8-bit formats, 2 of int16)
template <int FMT>
__device__ __forceinline__ float4 sample_pair_of(const v4u q, int e)
{
    return decode_pair<FMT>(FMT == SDRX_FMT_CS16 ? make_uint2(q[2 * e], q[2 * e + 1]) : make_uint2(q[e], 0u));
}
// natural order -> tile layout: one thread = one float4 = 2 complex samples (4 bytes of the 8-bit formats, 8 of int16)
template <int FMT>
__global__ __launch_bounds__(256) void k_ingest_samples(const unsigned *__restrict__ words, float4 *__restrict__ tiled, int n_pairs)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pairs)
        return;
    const int c = p >> 9, r = p & 511;
    tiled[tile_unit(c, r & 7, r >> 3)] = sample_pair<FMT>(words, p);
}

// ------------------------------------------------------------------------------------ DC-bias removal, exact: products, the sequential chain
// The same with the DC-bias removal of sdrj::demodData (sdrj.cpp:271-286):
//   avept = avept*(1.0f-0.000001f) + 0.000001f*curr;  curr -= avept        (per component, fp32)
// with an accumulator that lives for the whole process (function-static there; `state` here).
// It is a true first-order recurrence in ROUNDED fp32 arithmetic -- fl(fl(avept*keep) + fl(k*curr)) -- so the
// bit-exact form is sequential in the frame.  What IS sequential is two dependent VALU operations per sample and
// component, and on this machine a dependent v_mul_f32 -> v_add_f32 pair of a lone wave takes 12.25 cycles whatever
// else is or is not going on (tools/dc_chain_probe.hip: one chain per wave 12.25 cycles per step; I and Q interleaved
// in one wave 20.25 for the two; a DPP systolic form 20.25; a scalar operand costs nothing) -- while every OTHER
// instruction the chain wave issues costs its ~4.5 cycles on top (the round-3 kernel's LDS traffic and register copies:
// 24.6 cycles per sample).  So the chain gets a kernel in which it is nearly alone:
//   k_dc_products   (parallel)  P[c][t] = fl(k * curr)                       all samples, both components
//   k_dc_chain      (2 waves)   A[c][j] = avept before sample 16 j           wave c = component c, on a CU of its own; per 32
//                                                                            samples two s_load_dwordx16 (the products arrive as
//                                                                            scalar operands, a group ahead), the 64 chain
//                                                                            operations, ONE 8-byte store
//   k_dc_apply      (parallel)  replays the 16 steps behind each A[c][j], curr - avept, tile layout
// Measured: 2.03 ms per 384 000-sample frame (4.5 ms for the one-workgroup pipeline of round 3, 9.3 ms for the one-wave
// version of rounds 1-2); the floor of the recurrence itself is 384 000 x 12.25 cycles = 1.96 ms at 2.4 GHz.
constexpr int kDcPad = 32 * 16 + 128; // floats behind the last sample of P / A: the chain's scalar prefetch runs two groups ahead, its line prefetch kDcAhead
// (all the chain kernels below ever see is P, products of samples with |x| <= 128 whatever the format: what they are proved for)
template <int FMT>
__global__ __launch_bounds__(256) void k_dc_products(const unsigned *__restrict__ words, float *__restrict__ P, int n_complex, int stride)
{
    const int w = blockIdx.x * 256 + threadIdx.x; // one pair = 2 complex samples
    if (2 * w >= n_complex)
        return;
    const float k = 0.000001f;
    const float4 x = sample_pair<FMT>(words, w);
    const v2f pi = {k * x.x, k * x.z};
    const v2f pq = {k * x.y, k * x.w};
    *(SDRX_AS1 v2f *)(P + 2 * w) = pi;
    *(SDRX_AS1 v2f *)(P + stride + 2 * w) = pq;
}

// 32 products as scalar operands: requested here, ARRIVED only behind dc_products_wait() (scalar loads return out of order:
// nothing short of lgkmcnt(0) orders them).  The values the chain uses are the OUTPUTS of the wait, so no use of them can
// be scheduled above it.  (`before`: a value whose further uses must come AFTER the request -- the accumulator: the chain
// then cannot be scheduled above the loads it is meant to cover.)
// The products were written by other CUs: a scalar load of them misses all the way to the Infinity Cache (~500 cycles, more
// than the 392 cycles of chain a group of 32 samples covers).  So one VECTOR load per group touches the line kDcAhead groups
// further on -- its result is never used and never waited for (another counter: vmcnt) -- and the scalar loads find their
// lines in this XCD's L2.
constexpr int kDcAhead = 16; // groups of 32 samples = 2 KiB
// (`junk`: the register the line prefetches land in, some time after their issue and unknown to the compiler: one register,
// handed through every request, so that it is never anything else's.)
__device__ __forceinline__ void dc_products_request(v16f &lo, v16f &hi, const float *p, float &before, float &junk)
{
    asm volatile("s_load_dwordx16 %0, %4, 0x0\n\ts_load_dwordx16 %1, %4, 0x40\n\tglobal_load_dword %2, %5, off"
                 : "=s"(lo), "=s"(hi), "+v"(junk), "+v"(before)
                 : "s"(p), "v"(p + 32 * kDcAhead));
}
__device__ __forceinline__ void dc_products_wait(v16f &lo, v16f &hi) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(lo), "+s"(hi)); }

__device__ __forceinline__ float dc_block16(float acc, const v16f p)
{
    const float keep = 1.0f - 0.000001f;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        acc = acc * keep + p[i]; // -ffp-contract=off: v_mul_f32, v_add_f32 -- two roundings, like the reference's -O2 build
    return acc;
}

// A[c][j] = avept BEFORE sample 16 j of component c: one value per 16 samples is all the chain wave stores (every store is
// an instruction it issues on top of its chain); k_dc_apply replays the 16 steps behind each of them -- the same operations
// on the same values, so the same bits -- in parallel.
__global__ __launch_bounds__(64) void k_dc_chain(const float *__restrict__ P, float *__restrict__ A, int n_complex, int stride,
                                                 float *__restrict__ state)
{
    if (threadIdx.x != 0) // the chain is one value: one lane computes and stores it (exec is set once, here)
        return;
    const int c = blockIdx.x; // component
    const float *p = P + (size_t)c * stride;
    float2 *a = reinterpret_cast<float2 *>(A + (size_t)c * (stride >> 4)); // (start of block 2 g, start of block 2 g + 1)
    float acc = state[c];
    const int ngrp = (n_complex + 31) >> 5; // groups of 32 samples (the last one may reach 16 samples into the padding behind the frame)
    v16f c0, c1, n0, n1;
    float junk = 0.f;
    dc_products_request(c0, c1, p, acc, junk);
    int g = 0;
    for (; g + 1 < ngrp; g += 2) {
        dc_products_wait(c0, c1);
        dc_products_request(n0, n1, p + 32 * (g + 1), acc, junk);
        float s0 = acc;
        acc = dc_block16(acc, c0);
        gst2(a + g, make_float2(s0, acc));
        acc = dc_block16(acc, c1);
        dc_products_wait(n0, n1);
        dc_products_request(c0, c1, p + 32 * (g + 2), acc, junk); // (past the frame's end: the padding behind it)
        s0 = acc;
        acc = dc_block16(acc, n0);
        gst2(a + g + 1, make_float2(s0, acc));
        if (32 * (g + 1) + 16 < n_complex)
            acc = dc_block16(acc, n1);
    }
    dc_products_wait(c0, c1);
    if (g < ngrp) {
        const float s0 = acc;
        acc = dc_block16(acc, c0);
        gst2(a + g, make_float2(s0, acc));
        if (32 * g + 16 < n_complex)
            acc = dc_block16(acc, c1);
    }
    state[c] = acc;
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(junk)); // the last line prefetches have landed: the register is free again
}

// ------------------------------------------------------------------------------------ DC-bias removal, exact: the chain a block at a time (k_dc_chain_spec)
// The SAME recurrence, bit for bit, a block of 1024 samples at a time in parallel: k_dc_chain_spec.
//
// What makes fl(fl(a keep) + p) sequential is its two roundings.  Write a = s m 2^e with the 24-bit mantissa 2^23 <= m < 2^24
// (ulp = 2^e) and keep = 1 - 17 2^-24:
//   fl(a keep) = s (m - r(m)) 2^e,   r(m) = floor(17 m / 2^24 + 1/2)     the product m (2^24 - 17) 2^(e-24) rounded to 24 bits; it
//                                                                        stays in the binade for m >= 2^23 + 9 and is a tie only
//                                                                        for m = 2^23.  r is one of 9 .. 17 and constant over
//                                                                        runs of ~987 000 consecutive m; T = where it steps
//   fl(u + p)  = s (m_u + q) 2^e,    q = s RN(p / 2^e)                   u and the result multiples of the same ulp as long as the
//                                                                        sum stays in the binade; which way an exact tie of
//                                                                        p / 2^e goes depends on the parity of m_u
// So WHILE the binade and the sign stay what they are at the block's first sample and no p is an exact tie, the recurrence is
// one in INTEGERS:  m' = m + q - r_lo - [m >= T]  around the threshold T of r nearest to the block's first m (r = r_lo below
// it, r_lo + 1 from it on).  q comes out of ONE float addition that does the rounding for us -- v = fl(C + p) with C =
// s 1.5 2^23 2^e has a's ulp, so the mantissa bits of v are those of C plus q (C's mantissa is even: its ties go where an even
// m_u's would, and ties are excluded anyway) --, the tie test out of the exact residual p - (v - C).
// (The reference's estimate LIVES at such a threshold: below T the decrement r_lo is smaller than the mean of q, above it
// r_lo + 1 is larger, so m climbs to T and then hovers around it -- 1.2353 for an offset of 1.3 LSB, not 1.3.)
// One workgroup per component walks the frame, NW blocks per step, one wave each; lane l owns samples 16 l .. 16 l + 15 of its
// wave's block.  Every lane runs the integer recurrence for its 16 samples from a SPECULATED start value; a step stands once
// every lane -- of every wave -- started where its predecessor ended (dc_spec_blocks below: how the start values are found).
// Lane 0 of wave 0 always starts from the true value, lane l does if all before it did: then the 16 steps of every lane are the
// recurrence itself.  Such a step is then VERIFIED: every m it visited, INCLUDING the last, inside [start of r_lo's run, end of
// (r_lo + 1)'s run) and >= 2^23 + 32 (nothing may touch the binade's lower end, where fl(a keep) falls into the finer grid
// below), no exact tie.  A step that does not stand within kDcMaxIter rounds or fails the verification -- the binade or the
// sign changes inside it, a tie, |a| < 2^-9 (start-up: p is no longer small against a) -- is taken again block by block, each
// with its own context, and a block that fails on its own is redone with the rounded float operations themselves, one dependent
// mul + add pair per sample: k_dc_chain's arithmetic, 1024 steps.
// Verified blocks are bit-exact BY CONSTRUCTION, the others by definition (sdrx_stats.dc_blocks / dc_retried_blocks /
// dc_fallback_blocks say how many there were of each).  Output as k_dc_chain's: A[c][j] = avept before sample 16 j, for k_dc_apply.
constexpr int kDcBlock = 64 * kRun; // samples per block: a lane's run is one stored estimate's 16 samples
constexpr int kDcMaxIter = 24;      // rounds of "every lane from its speculated start value" before a step is given up (a quiet front end takes up to ~16)
__device__ __forceinline__ int wave_inclusive_scan(int x)
{
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true); // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true); // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true); // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true); // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false); // row_bcast:15 -> rows 1, 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false); // row_bcast:31 -> rows 2, 3
    return x;
}
// NW waves, NW consecutive blocks side by side: what one wave does for its block, one 16-byte record per wave and round exchanged
// through LDS (two sets alternating: one barrier per round).  Every wave derives the SAME context (binade, sign, T, r_lo) from the
// accumulator before the first of the NW blocks.
// Finding the start values.  A lane's total is a function of its start value: tot(x + d) - tot(x) is between -d and 0 (every step
// merges the states -1 and 0: two trajectories only ever come closer).  Each round EVALUATES every lane's run at its current start
// value (the integer recurrence itself) and looks at the gaps  g_l = start_l + tot_l - start_(l+1)  between a run's end and the
// start the next lane assumed: all gaps zero = every lane started where its predecessor ended = the recurrence itself.
// Otherwise the starts move by the solution u of  u_(l+1) = (1 + s_l) u_l + g_l,  u_0 = 0  (a scan of affine maps: DPP inside a
// wave, the waves' composed maps through LDS), s_l = the lane's secant slope out of its last two evaluations; in the first
// round, when there is only one, -min(1, 16 / range) for a run that saw both sides of T (its 16 merge points are spread over
// about the range it covered) and 0 otherwise.  With all slopes 0 the step is "every start := the sum of the totals before
// it", and that iteration needs as many rounds as there are lanes whose runs come across T one after the other; an estimate
// hovering at T with small steps (a quiet front end) or pinned to it (an offset many times the noise) has slopes near -1 --
// every run forgets where it started -- and the plain sums overshoot for dozens of rounds, where the affine step lands next to
// the answer (tools/dc_iteration_model.py: the iteration as a numpy model, rounds by noise level and waves per step).
// Nothing here has to be exact except the evaluation: a block is only accepted in a round that found every gap zero, and then
// VERIFIED (that round's runs all stayed inside the context, no tie).  NW = 1: no LDS, no barrier.
// In: `acc` (uniform over the workgroup), the lane's 16 products `p`, nv = lanes of this wave that hold samples, last_wave = the
// last wave that holds any.  Out: `start` = avept before the lane's first sample, `acc_out` = avept after the last block;
// false = nothing to be used.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f32(float old, float src)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), CTRL, ROW_MASK, 0xf, false));
}
// Inclusive scan over the wave's lanes of the maps x -> A x + B (lane l: its own map after those of the lanes before it).  One
// step = two instructions with the DPP operand in place: B += A * B[l - n] (lanes without a source read 0), A *= A[l - n] (lanes
// without a source are disabled: A stays) -- and the two wait states a DPP read of a just-written VGPR needs.
#define SDRX_AFFINE_STEP(ctrl, fill) "v_fmac_f32_dpp %1, %1, %0 " ctrl " bank_mask:0xf bound_ctrl:1\n\tv_mul_f32_dpp %0, %0, %0 " ctrl " bank_mask:0xf\n\t" fill
__device__ __forceinline__ void affine_scan_wave(float &A, float &B)
{
    asm volatile("s_nop 1\n\t"
                 SDRX_AFFINE_STEP("row_shr:1 row_mask:0xf", "s_nop 0\n\t")
                 SDRX_AFFINE_STEP("row_shr:2 row_mask:0xf", "s_nop 0\n\t")
                 SDRX_AFFINE_STEP("row_shr:4 row_mask:0xf", "s_nop 0\n\t")
                 SDRX_AFFINE_STEP("row_shr:8 row_mask:0xf", "s_nop 0\n\t")
                 SDRX_AFFINE_STEP("row_bcast:15 row_mask:0xa", "s_nop 0\n\t")
                 SDRX_AFFINE_STEP("row_bcast:31 row_mask:0xc", "s_nop 1")
                 : "+v"(A), "+v"(B));
}
__device__ __forceinline__ void affine_scan_lanes8(float &A, float &B, int n) // the same over the first n <= 8 lanes
{
    if (n > 4)
        asm volatile("s_nop 1\n\t" SDRX_AFFINE_STEP("row_shr:1 row_mask:0xf", "s_nop 0\n\t") SDRX_AFFINE_STEP("row_shr:2 row_mask:0xf", "s_nop 0\n\t")
                         SDRX_AFFINE_STEP("row_shr:4 row_mask:0xf", "s_nop 1")
                     : "+v"(A), "+v"(B));
    else if (n > 2)
        asm volatile("s_nop 1\n\t" SDRX_AFFINE_STEP("row_shr:1 row_mask:0xf", "s_nop 0\n\t") SDRX_AFFINE_STEP("row_shr:2 row_mask:0xf", "s_nop 1") : "+v"(A), "+v"(B));
    else
        asm volatile("s_nop 1\n\t" SDRX_AFFINE_STEP("row_shr:1 row_mask:0xf", "s_nop 1") : "+v"(A), "+v"(B));
}
template <int NW, typename AfterInputs>
__device__ __forceinline__ bool dc_spec_blocks(float acc, const float *p, int nv, int lane, int wave, int last_wave, int4 *xch, int &par, int rounds,
                                               float &start, float &acc_out, AfterInputs &&after_inputs)
{
    const unsigned bits = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, acc));
    const unsigned ex = (bits >> 23) & 255u, sign = bits & 0x80000000u;
    const int m0 = (int)((bits & 0x7fffffu) | 0x800000u);
    // r(m) = r for  r 2^24 <= 17 m + 2^23 < (r + 1) 2^24, i.e. from run_start(r) up to run_start(r + 1)
    auto run_start = [](int r) { return (int)((((unsigned)r << 24) - (1u << 23) + 16u) / 17u); };
    const int r0 = (int)((17u * (unsigned)m0 + (1u << 23)) >> 24);
    const int lo0 = run_start(r0), hi0 = run_start(r0 + 1);
    const bool near_lo = m0 - lo0 < hi0 - m0;
    const int T = near_lo ? lo0 : hi0, rlo = near_lo ? r0 - 1 : r0;
    const int lo = max(run_start(rlo), (1 << 23) + 32), hi = min(run_start(rlo + 2), 1 << 24);
    const bool ctx_ok = ex >= 118u && ex < 255u && m0 >= lo && m0 < hi; // |a| >= 2^-9: |p| / ulp < 2^21
    if (!ctx_ok) // (the same decision in every wave: they hold the same accumulator)
        return false;
    const unsigned cb = sign | (ex << 23) | 0x400000u;
    const float C = __builtin_bit_cast(float, cb);                                   // s 1.5 2^23 ulp
    const float half_ulp = __builtin_bit_cast(float, (ex >= 25u ? ex - 24u : 1u) << 23);
    // bits(v) - bits(C) = the change of the MAGNITUDE's mantissa (for a negative accumulator -RN(p / ulp), as it must be);
    // e[i] = that - r_lo - 1, so that a step is  z' = z + e[i] + [z < 0]  for z = m - T
    const int ebase = (int)cb + rlo + 1;
    float worst = 0.f; // max |residual|: never above half an ulp, equal to it = an exact tie
    int e[kRun], tot = 0;
#pragma unroll
    for (int i = 0; i < kRun; i += 2) {
        const v2f pp = {p[i], p[i + 1]}, CC = {C, C};
        const v2f v = CC + pp;           // (v_pk_add_f32: two samples per instruction)
        const v2f resid = pp - (v - CC); // exact
        const float v0 = v.x, v1 = v.y;  // (not __builtin_bit_cast(int, v.y): this compiler takes element 0 for it)
        worst = fmaxf(worst, fmaxf(fabsf(resid.x), fabsf(resid.y)));
        e[i] = __builtin_bit_cast(int, v0) - ebase;
        e[i + 1] = __builtin_bit_cast(int, v1) - ebase;
        tot += e[i] + e[i + 1];
    }
    asm volatile("" : "+v"(tot) : : "memory"); // (the products have arrived and are consumed)
    after_inputs();
    const bool tie = worst == half_ulp;
    const bool mine = lane < nv;
    const int S = m0 - T;
    // a lane behind this one takes over where this one ends (in this wave, or lane 0 of the next)
    const bool linked = lane + 1 < nv || (NW > 1 && lane == 63 && wave < last_wave);
    // the waves' records of a round -> what the waves before this one make of u = 0, the same for the next wave, the flags of all
    // (1: a gap somewhere, 2: a run left the context) and the last block's end
    auto exchange = [&](float A, float B, int flags, int end, float &u_in, float &u_next, int &end_last) {
        if constexpr (NW == 1) {
            u_in = 0.f, u_next = B, end_last = end;
            return flags;
        } else {
            if (lane == 0)
                xch[par * NW + wave] = make_int4(__builtin_bit_cast(int, A), __builtin_bit_cast(int, B), flags, end);
            __syncthreads();
            // lane w < NW takes wave w's record; the maps composed over those lanes (three DPP steps), the flags by ballot
            const int4 r = xch[par * NW + (lane < NW ? lane : NW - 1)];
            const bool rec = lane < NW;
            float Ar = rec ? __builtin_bit_cast(float, r.x) : 1.0f, Br = rec ? __builtin_bit_cast(float, r.y) : 0.0f;
            affine_scan_lanes8(Ar, Br, NW);
            const int Bi = __builtin_bit_cast(int, Br);
            u_in = wave > 0 ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(Bi, wave > 0 ? wave - 1 : 0)) : 0.f;
            u_next = __builtin_bit_cast(float, __builtin_amdgcn_readlane(Bi, wave));
            end_last = __builtin_amdgcn_readlane(r.w, last_wave);
            par ^= 1;
            return (__builtin_amdgcn_ballot_w64(rec && (r.z & 1)) != 0ull ? 1 : 0) | (__builtin_amdgcn_ballot_w64(rec && (r.z & 2)) != 0ull ? 2 : 0);
        }
    };
    // first guess.  With t steps before it a lane's start value lies between  a = S + (the sum of their e)  -- no step saw the
    // estimate below T -- and  b = a + t  -- every step did --: take the one of a, 0, b in the middle ("at T, unless not even the
    // extreme count gets it there").  An estimate that stays on its side of T through the block makes that exact; one that hovers
    // at T is guessed to within its excursion.  In integers (these sums go up to 2^31; the gaps of the rounds are counts of steps).
    int zs, next0; // this lane's start value minus T; the same of the lane behind lane 63
    {
        tot = mine ? tot : 0;
        const int incl = wave_inclusive_scan(tot);
        const int total = __builtin_amdgcn_readlane(incl, 63);
        int before = 0;
        if constexpr (NW > 1) {
            if (lane == 0)
                xch[par * NW + wave] = make_int4(total, 0, 0, 0);
            __syncthreads();
            int t = lane < NW ? xch[par * NW + (lane < NW ? lane : NW - 1)].x : 0; // lane w: wave w's total
            t += __builtin_amdgcn_update_dpp(0, t, 0x111, 0xf, 0xf, true);        // row_shr:1, 2, 4: the sums up to wave w
            if constexpr (NW > 2)
                t += __builtin_amdgcn_update_dpp(0, t, 0x112, 0xf, 0xf, true);
            if constexpr (NW > 4)
                t += __builtin_amdgcn_update_dpp(0, t, 0x114, 0xf, 0xf, true);
            before = wave > 0 ? __builtin_amdgcn_readlane(t, wave > 0 ? wave - 1 : 0) : 0;
            par ^= 1;
        }
        const int a = S + before + (incl - tot), a_next = S + before + total;
        zs = a >= 0 ? a : min(0, a + kRun * (64 * wave + lane));
        next0 = a_next >= 0 ? a_next : min(0, a_next + kRun * 64 * (wave + 1));
    }
    float slope = 0.f;
    int zs_prev = 0, tot_prev = 0;
    for (int it = 0; it < rounds; ++it) {
        int z = zs, zmin = zs, zmax = zs;
#pragma unroll
        for (int i = 0; i < kRun; ++i) {
            z = z + e[i] + (int)((unsigned)z >> 31);
            zmin = min(zmin, z);
            zmax = max(zmax, z);
        }
        tot = mine ? z - zs : 0;
        const int end = zs + tot;
        const int zs_behind = __builtin_amdgcn_update_dpp(next0, zs, 0x130, 0xf, 0xf, false); // wave_shl:1 (lane 63: next0)
        const int gap = linked ? end - zs_behind : 0;
        const bool ok = !mine || (!tie && zmin + T >= lo && zmax + T < hi);
        const int flags = (__builtin_amdgcn_ballot_w64(gap != 0) != 0ull ? 1 : 0) | (__builtin_amdgcn_ballot_w64(!ok) != 0ull ? 2 : 0);
        // the slope of this lane's total in its start value: the secant of its last two evaluations; before there are two, out
        // of the run itself -- one that saw both sides of T has its 16 merge points spread over about the range it covered
        if (it == 0)
            slope = zmin < 0 && zmax >= 0 ? -fminf(1.f, (float)kRun * __builtin_amdgcn_rcpf((float)(zmax - zmin + 1))) : 0.f;
        else if (zs != zs_prev)
            slope = fminf(0.f, fmaxf(-1.f, (float)(tot - tot_prev) * __builtin_amdgcn_rcpf((float)(zs - zs_prev))));
        zs_prev = zs, tot_prev = tot;
        float A = linked ? 1.0f + slope : 1.0f, B = (float)gap;
        affine_scan_wave(A, B);
        const float Aw = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, A), 63));
        const float Bw = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, B), 63));
        const int end_mine = __builtin_amdgcn_readlane(end, nv > 0 ? nv - 1 : 0);
        float u_in = 0.f, u_next = 0.f;
        int end_last = end_mine;
        const int f = exchange(Aw, Bw, flags, end_mine, u_in, u_next, end_last);
        if (!(f & 1)) { // every lane of every wave started this round where its predecessor ended
            if (f & 2)
                return false;
            const unsigned hi_bits = sign | ((ex - 1u) << 23); // + a mantissa with its leading one = the float
            start = __builtin_bit_cast(float, hi_bits + (unsigned)(zs + T));
            acc_out = __builtin_bit_cast(float, hi_bits + (unsigned)(end_last + T));
            return true;
        }
        const float Ae = dpp_f32<0x138, 0xf>(1.0f, A), Be = dpp_f32<0x138, 0xf>(0.0f, B); // wave_shr:1: the maps of the lanes BEFORE this one
        zs += (int)__builtin_rintf(__builtin_fmaf(Ae, u_in, Be));
        next0 += (int)__builtin_rintf(u_next);
    }
    return false;
}
// The rounded operations themselves on one wave's block, lane after lane: every lane runs the 16 steps on its own products from
// the uniform accumulator, lane l's result is the accumulator of the next round.  Returns the accumulator after the block.
__device__ __forceinline__ float dc_sequential_block(float acc, const float *p, int nv, int lane, float &start)
{
    const float keep = 1.0f - 0.000001f;
    start = acc;
    for (int l = 0; l < nv; ++l) {
        float t = acc;
        if (lane == l)
            start = acc;
#pragma unroll
        for (int i = 0; i < kRun; ++i)
            t = t * keep + p[i]; // -ffp-contract=off: v_mul_f32, v_add_f32
        acc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t), l));
    }
    return acc;
}
// One workgroup of NW waves per component walks the frame NW blocks at a time.  A step that does not verify as a whole is
// taken again wave after wave -- each block on its own, from the accumulator its predecessor leaves in LDS: with its own
// context, and with the rounded operations if that does not verify either -- so that one bad spot costs its own 1024 samples
// the sequential time and its NW - 1 neighbours the one-wave time.
// counters: [0] blocks walked, [1] blocks redone with the sequential operations, [2] blocks taken again on their own
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_dc_chain_spec(const float *__restrict__ P, float *__restrict__ A, int n_complex, int stride,
                                                           float *__restrict__ state, unsigned long long *__restrict__ counters, int rounds)
{
    __shared__ int4 xch[2 * NW];
    __shared__ float handover[2];
    const int c = blockIdx.x, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // component; lane; wave
    const float *p_c = P + (size_t)c * stride;
    float *a_c = A + (size_t)c * (stride >> 4);
    float acc = state[c]; // (uniform over the workgroup throughout)
    const int nblk = (n_complex + kDcBlock - 1) / kDcBlock;
    unsigned fallbacks = 0, retried = 0;
    int par = 0;
    float p[kRun], pn[kRun];
    auto load = [&](int b, float *dst) { // lane's 16 products of block b; behind the frame the last block's again (never used) --
        // ALWAYS four loads: behind a branch the compiler could not count them and would wait for the prefetch where it only
        // needs the block before it
        const float4 *src = reinterpret_cast<const float4 *>(p_c + (size_t)min(b, nblk - 1) * kDcBlock + lane * kRun);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const v4f v = gldv4(src + i);
            dst[4 * i] = v.x, dst[4 * i + 1] = v.y, dst[4 * i + 2] = v.z, dst[4 * i + 3] = v.w;
        }
    };
    // A step's start values leave in the NEXT step, right behind the point where that one has waited for its products: loads and
    // stores share one counter here, and a store issued at the end of a step would be waited for along with the products (its
    // acknowledgement takes longer than the step's arithmetic up to there).
    float held = 0.f;
    int held_at = -1;
    auto store_held = [&]() {
        if (held_at >= 0)
            *(SDRX_AS1 float *)(a_c + held_at) = held;
        held_at = -1;
    };
    // one step: `p` holds the lane's products of block b, `pn` receives those of block b + NW meanwhile
    auto step = [&](int b, float *p, float *pn) {
        load(b + NW, pn);
        const int nv = max(0, min(64, (n_complex - b * kDcBlock) >> 4)); // lanes that hold samples (frames are multiples of 16)
        const int last_wave = min(NW, nblk - (b - wave)) - 1;            // the last wave that holds any
        float start = acc, acc_out = acc;
        if (dc_spec_blocks<NW>(acc, p, nv, lane, wave, last_wave, xch, par, rounds, start, acc_out, store_held)) {
            acc = acc_out;
        } else if constexpr (NW == 1) {
            ++fallbacks;
            acc = dc_sequential_block(acc, p, nv, lane, start);
        } else {
            for (int w = 0; w < NW; ++w) {
                if (wave == w) {
                    int none = 0;
                    if (nv > 0 && dc_spec_blocks<1>(acc, p, nv, lane, 0, 0, nullptr, none, rounds, start, acc_out, [] {})) {
                        ++retried;
                        acc = acc_out;
                    } else if (nv > 0) {
                        ++fallbacks;
                        acc = dc_sequential_block(acc, p, nv, lane, start);
                    }
                    if (lane == 0)
                        handover[w & 1] = acc;
                }
                __syncthreads();
                acc = handover[w & 1];
            }
        }
        store_held(); // (only if this step never came to its inputs' end: no context)
        held = start, held_at = lane < nv ? b * 64 + lane : -1;
    };
    load(wave, p);
    for (int b = wave; b - wave < nblk; b += 2 * NW) { // (two steps per round: the product registers swap roles instead of being copied)
        step(b, p, pn);
        if (b - wave + NW < nblk)
            step(b + NW, pn, p);
    }
    store_held();
    if (lane == 0) {
        if (wave == 0)
            state[c] = acc;
        if (counters) {
            if (wave == 0)
                atomicAdd(counters + 0, (unsigned long long)nblk);
            if (fallbacks)
                atomicAdd(counters + 1, (unsigned long long)fallbacks);
            if (retried)
                atomicAdd(counters + 2, (unsigned long long)retried);
        }
    }
}

// ------------------------------------------------------------------------------------ DC-bias removal, exact: apply
// curr - avept in tile layout: one thread = the 16 samples behind one stored estimate = one lane's run of a tile.  They are
// 32 bytes of an 8-bit format (two 16-byte loads of 4 pairs) or 64 bytes of int16 (four loads of 2 pairs), all inside the
// frame: 16 j < n_complex and frames are multiples of 16
template <int FMT>
__global__ __launch_bounds__(256) void k_dc_apply(const unsigned *__restrict__ words, const float *__restrict__ A, float4 *__restrict__ tiled,
                                                  int n_complex, int stride)
{
    const int j = blockIdx.x * 256 + threadIdx.x; // block of 16 samples
    if (16 * j >= n_complex)
        return;
    constexpr int kLoads = FMT == SDRX_FMT_CS16 ? 4 : 2, kPairs = FMT == SDRX_FMT_CS16 ? 2 : 4; // 16-byte loads per thread, pairs in each
    const float keep = 1.0f - 0.000001f, k = 0.000001f;
    float ai = A[j], aq = A[(stride >> 4) + j];
    const v4u *src = reinterpret_cast<const v4u *>(words) + kLoads * j;
    const int ch = j >> 6, lane = j & 63;
#pragma unroll
    for (int h = 0; h < kLoads; ++h) {
        const v4u q = gldv4u(src + h);
#pragma unroll
        for (int e = 0; e < kPairs; ++e) {
            const float4 x = sample_pair_of<FMT>(q, e);
            ai = ai * keep + k * x.x;
            aq = aq * keep + k * x.y;
            float4 v;
            v.x = x.x - ai, v.y = x.y - aq;
            ai = ai * keep + k * x.z;
            aq = aq * keep + k * x.w;
            v.z = x.z - ai, v.w = x.w - aq;
            tiled[tile_unit(ch, kPairs * h + e, lane)] = v;
        }
    }
}

// ------------------------------------------------------------------------------------ DC-bias removal, tolerance arithmetic
// The fast-arithmetic form of the same DC-bias removal (option "exact" = 0): the recurrence is
// linear, a_t = A a_{t-1} + B x_t, so it is evaluated as a blocked scan -- per 1024-sample chunk
// one wave runs 16 sequential steps per lane from zero, combines the 64 lane totals with a
// log-step scan of affine maps, and adds the carry-in  A^(16 l + i + 1) * (state before the chunk).
// k_dc_block_sums leaves each chunk's zero-state response; k_ingest_dc_fast folds the responses
// of all earlier chunks into its own carry-in (<= 375 terms, powers of A^1024 from a host table)
// and writes the corrected chunk in tile layout.  Chunk-level sums are kept in double; against the
// reference's sequentially ROUNDED fp32 recurrence the estimate differs by ~1e-5 of the DC offset
// itself (a random walk of half-ulp roundings over the filter's 1e6-sample memory), far below 1e-5
// of the signal.  dctab: [0..16] = A^k, [32..95] = A^(16 l), [96 + k] = A^(1024 k).
struct DcLocal {
    float ai[kRun], aq[kRun]; // zero-state response at each of the lane's 16 samples
    float xi[kRun], xq[kRun];
};
// Behind a short last chunk the lanes go on with the format's neutral WORD -- the one whose samples are 0: 0x7f bytes, the
// integer 0 of the signed formats -- decoded like a loaded one (a select between words, in front of the decode, not between
// float4s behind it): nothing is read past the frame's n_complex samples.
template <int FMT>
__device__ __forceinline__ void dc_local(const unsigned *__restrict__ words, int base, int valid, int lane, DcLocal &L)
{
    constexpr unsigned kNeutral = FMT == SDRX_FMT_CU8 ? 0x7f7f7f7fu : 0u;
    const float keep = 1.0f - 0.000001f, k = 0.000001f;
    float ai = 0.f, aq = 0.f;
#pragma unroll
    for (int i2 = 0; i2 < 8; ++i2) {
        const int s0 = lane * kRun + 2 * i2;
        const float4 v = decode_pair<FMT>(s0 < valid ? pair_words<FMT>(words, (base + s0) >> 1) : make_uint2(kNeutral, kNeutral));
        const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            ai = fmaf(ai, keep, k * x[2 * h]);
            aq = fmaf(aq, keep, k * x[2 * h + 1]);
            L.ai[2 * i2 + h] = ai, L.aq[2 * i2 + h] = aq;
            L.xi[2 * i2 + h] = x[2 * h], L.xq[2 * i2 + h] = x[2 * h + 1];
        }
    }
}
// inclusive scan over the lanes of S_l = T_l + A16 * S_{l-1}
__device__ __forceinline__ void dc_wave_scan(double &si, double &sq, const double *__restrict__ dctab, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double m = dctab[32 + d]; // A^(16 d)
        const double ti = __shfl_up(si, d), tq = __shfl_up(sq, d);
        if (lane >= d) {
            si = fma(m, ti, si);
            sq = fma(m, tq, sq);
        }
    }
}
template <int FMT>
__global__ __launch_bounds__(64) void k_dc_block_sums(const unsigned *__restrict__ words, int n_complex, const double *__restrict__ dctab,
                                                      double2 *__restrict__ sums)
{
    const int c = blockIdx.x, lane = threadIdx.x, base = c * kChunk;
    DcLocal L;
    dc_local<FMT>(words, base, min(kChunk, n_complex - base), lane, L);
    double si = L.ai[kRun - 1], sq = L.aq[kRun - 1];
    dc_wave_scan(si, sq, dctab, lane);
    if (lane == 63)
        sums[c] = make_double2(si, sq);
}
template <int FMT>
__global__ __launch_bounds__(64) void k_ingest_dc_fast(const unsigned *__restrict__ words, float4 *__restrict__ tiled, int n_complex,
                                                       const float *__restrict__ state_in, float *__restrict__ state_out,
                                                       const double *__restrict__ dctab, const double2 *__restrict__ sums)
{
    const int c = blockIdx.x, lane = threadIdx.x, base = c * kChunk;
    const int valid = min(kChunk, n_complex - base);
    // carry-in of the chunk: the state before the frame and every earlier chunk's response
    double ci = 0.0, cq = 0.0;
    for (int j = lane; j < c; j += 64) {
        const double m = dctab[96 + (c - 1 - j)];
        const double2 b = sums[j];
        ci = fma(m, b.x, ci);
        cq = fma(m, b.y, cq);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        ci += __shfl_xor(ci, d);
        cq += __shfl_xor(cq, d);
    }
    ci = fma(dctab[96 + c], (double)state_in[0], ci);
    cq = fma(dctab[96 + c], (double)state_in[1], cq);
    DcLocal L;
    dc_local<FMT>(words, base, valid, lane, L);
    double si = L.ai[kRun - 1], sq = L.aq[kRun - 1];
    dc_wave_scan(si, sq, dctab, lane);
    double pi = __shfl_up(si, 1), pq = __shfl_up(sq, 1); // S_{l-1}
    if (lane == 0)
        pi = 0.0, pq = 0.0;
    const double inc_i = fma(dctab[32 + lane], ci, pi), inc_q = fma(dctab[32 + lane], cq, pq); // state before this lane's run
    float ai_last = 0.f, aq_last = 0.f;
#pragma unroll
    for (int i2 = 0; i2 < 8; ++i2) {
        float y[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = 2 * i2 + h;
            const float ai = (float)fma(dctab[i + 1], inc_i, (double)L.ai[i]);
            const float aq = (float)fma(dctab[i + 1], inc_q, (double)L.aq[i]);
            y[2 * h] = L.xi[i] - ai;
            y[2 * h + 1] = L.xq[i] - aq;
            ai_last = ai, aq_last = aq;
        }
        if (lane * kRun + 2 * i2 < valid)
            tiled[tile_unit(c, i2, lane)] = make_float4(y[0], y[1], y[2], y[3]);
    }
    if (base + valid == n_complex && lane == (valid >> 4) - 1) { // the frame's last sample (frames are multiples of 16)
        state_out[0] = ai_last;
        state_out[1] = aq_last;
    }
}
