// mix.hip -- the work item of the mix launches: the vfo::process mix loop (vfo.cpp:237-245) and the half-band cascade
// (HalfBandDecimator::decimate, halfbanddecimator.cpp:43-72, with FIR::FIRUpdateAndProcessHalfBandQueue and
// FIRQueueBackToFront, dsp.cpp:96-173) as mix_item; the first half of vfo::usb_decimdemod (vfo.cpp:334-356) for a d = 0 leaf
// inside the same wave as late_item; run_item, which picks the body, and the kernel k_mix_decimate.  k_mix_levels and
// k_levels_tail (levels.hip) run the same items.
// Relies on dev_helpers.hip (v2f, fir_mac*, static_for, the buffer stores, shr1, wave_sync), nco.hip (nco_step_pk,
// nco_mix_fast16, cmul_fast2), meter.hip and demod.hip (demod_prologue, demod_chunk), and on tile_unit / tile_index
// (sdrx_dev.h).

// ------------------------------------------------------------------------------------ half-band
// hbcoeff11, halfbanddecimator.h:66-79 (only the 11-tap case is ever instantiated, vfo.cpp:130).
#define HB0 0.0060431029837374152f
#define HB2 (-0.049372515458761493f)
#define HB4 0.29332944952052842f
#define HB5 0.5f

// FIR::FIRUpdateAndProcessHalfBandQueue case 11 (dsp.cpp:137-143): symmetric-pair form,
// evaluated left to right, then `0 + ...`.
template <bool EXACT>
__device__ __forceinline__ float hb_dot(float w0, float w2, float w4, float w5, float w6, float w8, float w10)
{
    if (EXACT) {
        float s = HB0 * (w0 + w10) + HB2 * (w2 + w8) + HB4 * (w4 + w6) + HB5 * w5;
        return 0.0f + s;
    } else {
        return fmaf(HB0, w0 + w10, fmaf(HB2, w2 + w8, fmaf(HB4, w4 + w6, HB5 * w5)));
    }
}

// the same on a packed complex sample (both components in one instruction each)
template <bool EXACT>
__device__ __forceinline__ v2f hb_dot2(v2f w0, v2f w2, v2f w4, v2f w5, v2f w6, v2f w8, v2f w10)
{
    if (EXACT) {
        const v2f s = HB0 * (w0 + w10) + HB2 * (w2 + w8) + HB4 * (w4 + w6) + HB5 * w5;
        return 0.0f + s;
    } else {
        const v2f h0 = {HB0, HB0}, h2 = {HB2, HB2}, h4 = {HB4, HB4};
        return __builtin_elementwise_fma(h0, w0 + w10,
                                         __builtin_elementwise_fma(h2, w2 + w8, __builtin_elementwise_fma(h4, w4 + w6, HB5 * w5)));
    }
}

// ------------------------------------------------------------------------------------ a wave's LDS
// LDS of k_mix_decimate (per wave): two 8-entry carry rows for the register stages, then the
// linear stage arrays A_s = [16 carry | 1024 >> s data] for the stages s >= 2 that run in LDS,
// and (only when a d == 0 VFO must emit natural order) a padded transpose tile.
constexpr int kRegStages = 2;                       // stages 0 and 1 live in registers
constexpr int kCarryBytes = 2 * 8 * 8;              // car0[8], car1[8] float2
__host__ __device__ constexpr int stage_elems(int s) { return kCarry + (s >= 3 ? 2 : 1) * (kChunk >> s); } // (stages >= 3: two chunks' worth, hb_stage_fixed)
__host__ __device__ constexpr int stage_offset(int s) // float2 index of A_s, s >= kRegStages
{
    int o = 0;
    for (int t = kRegStages; t < s; ++t)
        o += stage_elems(t);
    return o;
}
__host__ __device__ constexpr int pad0(int p) { return p + 2 * (p >> 4); }
constexpr int kTransposeElems = kChunk + 2 * (kChunk >> 4); // 1152 float2
__host__ __device__ constexpr int k1_lds_bytes(int d, bool need_transpose)
{
    int stages = 8 * stage_offset(d < kRegStages ? kRegStages : d);
    if (d == kRegStages && stages < 64 * 32)
        stages = 64 * 32; // a d = 2 leaf parks its four outputs per lane here until the next chunk's loads are issued (HeldStores)
    int tr = need_transpose ? 8 * kTransposeElems : 0;
    return kCarryBytes + (stages > tr ? stages : tr);
}
// a d = 2 leaf that demodulates in its wave (option fuse_demod): the carry rows, then demod_chunk's map (demod.hip)
__host__ __device__ constexpr int demod_lds_bytes() { return kCarryBytes + 4 * kDmFloats; }

// ------------------------------------------------------------------------------------ half-band stages, in LDS and in registers
// One half-band stage of one chunk in LDS (stages >= 2): A = [16 carry | cnt data] -> B data, or
// the output stream when this is the last stage.
template <bool EXACT>
__device__ __forceinline__ void hb_stage_lds(v2f *__restrict__ A, v2f *__restrict__ B, float2 *__restrict__ gout, int gbase,
                                             bool tiled, bool last, int jmin, int cnt, int lane, bool save,
                                             float2 *__restrict__ hbsave)
{
    wave_sync(); // stage input (written by the previous phase) is visible
    const int nout = cnt >> 1;
    for (int j = lane; j < nout; j += 64) {
        const v2f *w = A + kCarry + 2 * j - 10; // w[0..10], newest = input sample 2j of this chunk
        const v2f y = hb_dot2<EXACT>(w[0], w[2], w[4], w[5], w[6], w[8], w[10]);
        if (!last)
            B[kCarry + j] = y;
        else if (j >= jmin) { // outputs below jmin belong to the warm-up of a segment that starts inside the frame
            if (tiled)
                gstv2(gout + tile_index<size_t>(gbase + j), y);
            else
                gstv2(gout + (size_t)(gbase + j), y);
        }
    }
    wave_sync(); // all window reads done before the carry is overwritten
    // FIRQueueBackToFront (dsp.cpp:163-173) at the end of the FRAME: x[-k] := x[size-1-k]
    if (save && lane < kHbHist)
        gstv2(hbsave + lane, A[kCarry + cnt - 2 - lane]);
    v2f t;
    if (lane < kCarry)
        t = A[cnt + lane]; // the last 16 of [carry | data]
    wave_sync();
    if (lane < kCarry)
        A[lane] = t;
}

// The same LDS stages 2 .. D-1 for the common case -- a FULL chunk (1024 inputs) of a leaf VFO (natural-order output)
// that does not hold the frame's last sample -- with the depth as a compile-time constant: every count, LDS offset
// and trip count folds, the per-stage loop, the tiled / natural and last / not-last selects and the save branch
// disappear (the generic routine spends about as many VALU instructions on them as on the 11-operation dot product).
// Same arithmetic, same order, same LDS contents afterwards.
constexpr int kFixedDepth = 5; // 1.536 MS/s / 384 kS/s -> 48 / 12 kS/s: the depth of the reference's sub VFOs below a 384 k main
// Stage S of a full chunk: A_S = [16 carry | M * (1024 >> S) inputs] -> outputs into B's data from entry `boff` on, or -- the last stage --
// to the leaf's stream.  M = 2: the stage runs every SECOND chunk on two chunks' worth of input (paired stages: stages >= 3
// of a d = 5 leaf, whose last stage otherwise fills 32 of the 64 lanes; one carry hand-over and one set of phase fences per
// two chunks).  Same arithmetic on the same values in the same order: an output does not know how many of its neighbours
// were computed in the same pass.
// A chunk's output stores, held back until the NEXT chunk's loads have been issued (mix_item's chunk loop): vmcnt counts a
// wave's loads and stores in ONE in-order queue, so a wave that waits for loads issued behind its stores also waits for the
// stores' acknowledgements -- measured on the tolerance-arithmetic kernel, the stores in front of the next chunk's loads cost
// the launch 13 of its 63 us (profiles/README.md, round 5).  Stores issued behind the loads are never waited for.
struct HeldStores {
    v2f one;       // units == 1: the cf32 itself (last LDS stage of a d = 5 leaf)
    int units = 0; // (everything below is wave-uniform: SGPRs) 0 nothing held; 1: `one` = output gbase + lane, held by the lanes
                   //   jmin <= lane < nout; 2: z[0..3] of a d = 2 leaf, parked in the lane's 32 bytes of LDS, of the chunk at `base`
    int gbase = 0, jmin = 0, nout = 0;
    int base = 0, lv = 0;
};
template <bool EXACT, int S, int D, int M, int boff = 0>
__device__ __forceinline__ void hb_stage_fixed1(v2f *__restrict__ lds, HeldStores &held, int gbase, int jmin, int lane)
{
    constexpr int cnt = M * (kChunk >> S), nout = cnt >> 1;
    v2f *A = lds + stage_offset(S);
    v2f *B = lds + stage_offset(S + 1); // (not touched by the last stage)
    asm volatile("" : "+v"(lane)); // (the pass's LDS addresses are computed here, from this: hoisted out of the chunk loop they spill)
    wave_sync(); // stage input (written by the previous phase) is visible
    if constexpr (nout >= 64) {
#pragma unroll
        for (int it = 0; it < nout / 64; ++it) {
            const int j = lane + 64 * it;
            const v2f *w = A + kCarry + 2 * j - 10;
            const v2f y = hb_dot2<EXACT>(w[0], w[2], w[4], w[5], w[6], w[8], w[10]);
            if constexpr (S + 1 < D) {
                B[kCarry + boff + j] = y;
            } else { // the leaf's stream: one output per lane, stored behind the next chunk's loads
                static_assert(nout <= 64, "the last stage of a fixed-depth leaf has at most one output per lane");
                held.one = y;
                held.units = 1, held.gbase = gbase, held.jmin = jmin, held.nout = nout;
            }
        }
    } else {
        if constexpr (S + 1 == D)
            held.units = 1, held.gbase = gbase, held.jmin = jmin, held.nout = nout;
        if (lane < nout) {
            const v2f *w = A + kCarry + 2 * lane - 10;
            const v2f y = hb_dot2<EXACT>(w[0], w[2], w[4], w[5], w[6], w[8], w[10]);
            if constexpr (S + 1 < D) {
                B[kCarry + boff + lane] = y;
            } else {
                held.one = y;
            }
        }
    }
    wave_sync(); // all window reads done before the carry is overwritten
    v2f t;
    if (lane < kCarry)
        t = A[cnt + lane]; // the last 16 of [carry | data]
    wave_sync();
    if (lane < kCarry)
        A[lane] = t;
}
// stages S .. D-1, each on M chunks' worth of input
template <bool EXACT, int S, int D, int M>
__device__ __forceinline__ void hb_stage_fixed(v2f *__restrict__ lds, HeldStores &held, int gbase, int jmin, int lane)
{
    hb_stage_fixed1<EXACT, S, D, M>(lds, held, gbase, jmin, lane);
    if constexpr (S + 1 < D)
        hb_stage_fixed<EXACT, S + 1, D, M>(lds, held, gbase, jmin, lane);
}

// NOUT outputs of a register-resident stage.  ext[k] holds input sample k-10 of this lane's run
// (k = 0..9: the halo, only the needed ones set).
template <bool EXACT, int NOUT>
__device__ __forceinline__ void hb_regs(const v2f *ext, v2f *y)
{
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        const v2f *w = ext + 2 * j; // w[t] = input sample 2j - 10 + t
        y[j] = hb_dot2<EXACT>(w[0], w[2], w[4], w[5], w[6], w[8], w[10]);
    }
}

// halo slot q (0..7) <-> distance k back from the lane's first sample: -10,-8,-6,-5,-4,-3,-2,-1
__device__ __forceinline__ constexpr int halo_k(int q) { return q == 0 ? 10 : q == 1 ? 8 : q == 2 ? 6 : 8 - q; }

// ---- the pieces of a chunk that mix_item and late_item share ---------------------------------------------------------------
// The lane's 16 consecutive samples of a raw (natural-order) frame: cf32 as the caller handed it -- each lane reads its own
// 128 contiguous bytes: uncoalesced across the wave, but a level of 2-3 main VFOs is latency bound and this saves the layout
// pass over the raw frame -- or dongle bytes, floats[b] = b - 127 (jonti/sdr.cpp:43-49), 32 bytes per lane.
__device__ __forceinline__ void load_run_raw(const void *__restrict__ raw, int raw_mode, int p16, bool active, v2f *x)
{
    if (raw_mode == kRawF32) {
        const float4 *nat = reinterpret_cast<const float4 *>(raw) + (size_t)p16 * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const v4f z4 = {0.f, 0.f, 0.f, 0.f};
            const v4f v = active ? gldv4(nat + i) : z4;
            x[2 * i] = lo2(v);
            x[2 * i + 1] = hi2(v);
        }
    } else {
        const v4u *nat = reinterpret_cast<const v4u *>(raw) + (size_t)p16 * 2;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const v4u z4 = {0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu}; // 127 -> 0.0f
            const v4u q = active ? gldv4u(nat + h) : z4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 s = cu8_pair(q[k]);
                const v2f a = {s.x, s.y}, b = {s.z, s.w};
                x[8 * h + 2 * k] = a;
                x[8 * h + 2 * k + 1] = b;
            }
        }
    }
}
// The same out of a tile-layout stream: 8 coalesced 16-byte loads, unit (i2, lane) of the tile at `src`.
__device__ __forceinline__ void load_run_tile(const float4 *__restrict__ src, v2f *x)
{
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const v4f v = gldv4(src + 64 * i); // tile_unit(c, i, l) = tile_unit(c, 0, l) + 64 i
        x[2 * i] = lo2(v);
        x[2 * i + 1] = hi2(v);
    }
}
// NCO + mixer on the lane's run (oscillator.cpp:20-28,39-50; vfo.cpp:241): regenerate table[idx .. idx + 16) from the
// checkpoint `o` before it -- the exact recurrence, or in the tolerance arithmetic rotations of the checkpoint where the
// chunk's `span` table entries from position i0 on are settled ones and do not wrap -- and multiply.  The very first sample
// after start-up is multiplied by the LAST table entry (`last`: oscillator.cpp:30,39-50).
// Three arithmetics (option "exact"): EXACT -- the reference's operations in its order, every product and sum rounded.
// !EXACT && ROT ("tolerance") -- table entries as rotations of the exact checkpoint, FMA mixer and filters: cheapest, but the
// table's error (~1e-6 of |v|) multiplies the TOTAL input power, so a strong out-of-band carrier eats the 1e-5 bar.
// !EXACT && !ROT ("robust") -- the table entries from the exact recurrence (error 0: bit-identical to the reference's table),
// FMA mixer and filters: what remains is FMA-versus-two-roundings noise, ~6e-8 per operation, whatever is out of band.
template <bool EXACT, bool ROT>
__device__ __forceinline__ void nco_mix(v2f o, v2f rot, const float2 *__restrict__ rk, const float2 *__restrict__ last, bool first_ever, int i0,
                                        int span, int L, v2f *x)
{
    static_assert(!(EXACT && ROT), "the exact arithmetic replays the table");
    if constexpr (!EXACT && !ROT) {
#pragma unroll
        for (int i = 0; i < kRun; i += 2) {
            o = nco_step_pk(o, rot);
            v2f m0 = o;
            if (i == 0 && first_ever)
                m0 = gldv2(last);
            o = nco_step_pk(o, rot);
            cmul_fast2(m0, o, x[i], x[i + 1]);
        }
        return;
    }
    bool replay = true;
    if constexpr (!EXACT) // (wave-uniform)
        replay = i0 < kNcoSettle || i0 + span > L;
    if (replay) {
#pragma unroll
        for (int i = 0; i < kRun; ++i) {
            o = nco_step_pk(o, rot);
            v2f m = o;
            if (i == 0 && first_ever)
                m = gldv2(last);
            x[i] = cmul(m, x[i]);
        }
    } else {
        nco_mix_fast16(o, rk, x);
    }
}
// Stage 0's halo: ext0[0..9] = x[-10..-1] = the previous lane's x[6, 8, 10 .. 15] (one whole-wave DPP shift each); lane 0 takes
// the previous chunk's lane 63 from the 8-entry LDS row car0, which lane 63 then refills for the next chunk.
__device__ __forceinline__ void halo_stage0(v2f *car0, v2f *ext0, int lane)
{
    const v2f zero2 = {0.f, 0.f};
    const v2f *x = ext0 + 10;
    wave_sync(); // car0 of the previous chunk (or the initial state) is visible
    {
        const v4f *c4 = reinterpret_cast<const v4f *>(car0); // broadcast reads
        const v4f q0 = c4[0], q1 = c4[1], q2 = c4[2], q3 = c4[3];
        ext0[0] = shr1(lo2(q0), x[6]);   // x[-10]
        ext0[2] = shr1(hi2(q0), x[8]);   // x[-8]
        ext0[4] = shr1(lo2(q1), x[10]);  // x[-6]
        ext0[5] = shr1(hi2(q1), x[11]);  // x[-5]
        ext0[6] = shr1(lo2(q2), x[12]);  // x[-4]
        ext0[7] = shr1(hi2(q2), x[13]);  // x[-3]
        ext0[8] = shr1(lo2(q3), x[14]);  // x[-2]
        ext0[9] = shr1(hi2(q3), x[15]);  // x[-1]
        ext0[1] = ext0[3] = zero2;       // x[-9], x[-7]: never read
    }
    wave_sync(); // every lane holds its halo: lane 63 may now leave ITS tail for the next chunk
    if (lane == 63) {
        v4f *c4 = reinterpret_cast<v4f *>(car0);
        c4[0] = cat2(x[6], x[8]);
        c4[1] = cat2(x[10], x[11]);
        c4[2] = cat2(x[12], x[13]);
        c4[3] = cat2(x[14], x[15]);
    }
}
// Stage 1's: y[-8, -6, -5, -4, -3, -2, -1] = the previous lane's y[0, 2 .. 7], y[-10] = the lane before that one's y[6] (a second
// shift of the shifted y[6]); lanes 63 and 62 refill car1.
__device__ __forceinline__ void halo_stage1(v2f *car1, v2f *ext1, int lane)
{
    const v2f zero2 = {0.f, 0.f};
    const v2f *y = ext1 + 10;
    {
        const v4f *c4 = reinterpret_cast<const v4f *>(car1);
        const v4f q0 = c4[0], q1 = c4[1], q2 = c4[2], q3 = c4[3];
        ext1[2] = shr1(hi2(q0), y[0]);  // y[-8]
        ext1[4] = shr1(lo2(q1), y[2]);  // y[-6]
        ext1[5] = shr1(hi2(q1), y[3]);  // y[-5]
        ext1[6] = shr1(lo2(q2), y[4]);  // y[-4]
        ext1[7] = shr1(hi2(q2), y[5]);  // y[-3]
        ext1[8] = shr1(lo2(q3), y[6]);  // y[-2]
        ext1[9] = shr1(hi2(q3), y[7]);  // y[-1]
        ext1[0] = shr1(lo2(q0), ext1[8]); // y[-10]
        ext1[1] = ext1[3] = zero2;
    }
    wave_sync(); // every lane has read car1
    if (lane == 63) {
        car1[1] = y[0]; // slot 1 (y[-8]); slot 0 comes from lane 62
        v4f *d4 = reinterpret_cast<v4f *>(car1);
        d4[1] = cat2(y[2], y[3]);
        d4[2] = cat2(y[4], y[5]);
        d4[3] = cat2(y[6], y[7]);
    }
    if (lane == 62)
        car1[0] = y[6];
}

// ------------------------------------------------------------------------------------ mix_item
// Fused NCO + mixer + half-band cascade.
// Waves per SIMD the register allocator must leave room for: 5 (at 6, 80 VGPRs, the tolerance arithmetic spills inside its
// chunk loop: k_mix_levels 102 vs 60 us on config 3; profiles/README.md round 6).
constexpr int kK1MinWaves = 5;
// The body of one work item, run by ONE wave on LDS of its own (`smem`: k1_lds_bytes()); `level0`: the
// item's VFO is fed by the raw frame (`raw`, `raw_mode`), otherwise by its parent's tile-layout stream.
// DM: the leaf demodulates its stream in this very wave (demod_chunk; DEPTH == 2 only) -- decimate[2] itself is then written only
// where it is wanted (K1Vfo::tap: the spectrum tap, option keep_streams).
// METER (with DM): the item's output meter goes to the leaf's record s_first_out >> s (K2Vfo::meter_rel).  (Only the
// descriptor the chunks use anyway is read: the exact k_levels_tail has no SGPR to spare for another pointer.)
template <bool EXACT, int DEPTH, bool ROT, bool DM = false, bool METER = false>
__device__ __forceinline__ void mix_item(const K1Vfo *__restrict__ vfos, const K1Work W, unsigned long long frame_no,
                                         const void *__restrict__ raw, int raw_mode, bool level0_arg, unsigned char *smem, int lane)
{
    v2f *car0 = reinterpret_cast<v2f *>(smem);             // [8]
    v2f *car1 = car0 + 8;                                  // [8]
    v2f *lds = reinterpret_cast<v2f *>(smem + kCarryBytes);

    const int par = (int)(frame_no & 1ull);
    const K1Vfo *Dp = vfos + W.vfo;
    struct {
        const float2 *cp;
        int n_in, d, L, out_tiled;
    } D = {ldc(&Dp->cp), ldc(&Dp->n_in), ldc(&Dp->d), ldc(&Dp->L), ldc(&Dp->out_tiled)};
    // DEPTH >= 0: the item is a LEAF with that many half-band stages below a parent (the shapes the time goes into: the
    // reference's sub VFOs, 5 and 2 stages) -- depth, input form and output form are compile-time constants, every branch on
    // them folds, and the chunk loop keeps only what that shape needs in registers.  DEPTH < 0: any VFO (run-time fields).
    constexpr bool kShape = DEPTH >= 0;
    const int dd = kShape ? DEPTH : D.d;
    const bool level0 = kShape ? false : level0_arg;
    const int otiled = kShape ? 0 : D.out_tiled;
    const v2f rot = {ldc(&Dp->rot_re), ldc(&Dp->rot_im)};
    const float4 *in = reinterpret_cast<const float4 *>(ldc(&Dp->in[par]));
    float2 *out = ldc(&Dp->out[par]);
    const float2 *hb_load = ldc(&Dp->hb[par]);
    float2 *hb_save = ldc(&Dp->hb[par ^ 1]);
    const bool from_state = W.s_begin == 0;
    const v2f zero2 = {0.f, 0.f};

    // Filter state at the start of this segment: segment 0 continues from the previous frame's
    // history (zero at start-up, dsp.cpp:40-49); a later segment starts from zeros and runs
    // warm-up chunks until every stage's window holds real samples again.
    if (lane < 8) {
        const int k = halo_k(lane);
        car0[lane] = (from_state && dd > 0) ? gldv2(hb_load + 0 * kHbHist + k - 1) : zero2;
        car1[lane] = (from_state && dd > 1) ? gldv2(hb_load + 1 * kHbHist + k - 1) : zero2;
    }
    for (int s = kRegStages; s < dd; ++s)
        if (lane < kCarry) {
            const int k = kCarry - lane; // carry position `lane` is x[-k]
            lds[stage_offset(s) + lane] = (from_state && k <= kHbHist) ? gldv2(hb_load + s * kHbHist + k - 1) : zero2;
        }
    static_assert(!DM || DEPTH == 2, "the in-wave demodulation is laid out for 256 stream samples per chunk");
    float *dm = reinterpret_cast<float *>(lds); // (DM: the demodulation's arrays live where a d = 2 leaf would park its held stores)
    DemodCtx dmc;
    if constexpr (DM)
        demod_prologue(dm, ldc(&Dp->dm), par, from_state, lane, dmc);
    MeterAcc macc = meter_zero();
    const unsigned long long origin = ldc(&Dp->origin); // (frame_no >= origin: set between frames)
    const int phase_frame = (int)(((frame_no - origin) * (unsigned long long)D.n_in) % (unsigned long long)D.L);

    // The item walks 1024-sample chunks from sample s_begin (any multiple of 16: a chunk need not
    // coincide with a tile of the input) and emits the outputs whose input position is >= s_first_out.
    const int first_out = W.s_first_out;
    const int lane16 = (W.s_begin >> 4) + lane; // this lane's run in the item's first chunk, in units of 16 samples
    // the lane's first 16-byte unit of the item as a 32-bit index (a frame has < 2^20 units): the loads below then take the
    // uniform stream pointer from SGPRs and one 32-bit VGPR offset instead of keeping a 64-bit pointer alive per lane
    const unsigned unit_item = (unsigned)(lane16 >> 6) * 512u + (unsigned)(lane16 & 63);
    // this lane's NCO checkpoint for the chunk at `at`: cp[idx >> 4], idx = table position of the lane's first sample
    auto cp_of = [&](int at) {
        int ix = phase_frame + at; // both < L
        ix -= ix >= D.L ? D.L : 0;
        ix += lane * kRun;         // L >= kChunk (checked by sdrx_finalize)
        ix -= ix >= D.L ? D.L : 0;
        return D.cp + (ix >> 4);
    };
    // (the shaped bodies only: the any-VFO body has no register to spare -- it requests its checkpoint and stores its outputs
    // where they arise)
    v2f o_next = zero2;                   // the next chunk's checkpoint, requested a chunk ahead: the whole NCO hangs on these 8 bytes
    if constexpr (kShape)
        o_next = gldv2(cp_of(W.s_begin));
    HeldStores held;                      // the previous chunk's output stores (issued behind this chunk's loads)
    held.one = zero2;
    auto flush_held = [&]() {
        if constexpr (DM) { // (nothing is ever held: the payload leaves where it arises, 8 bytes per lane and chunk)
        } else if constexpr (!kShape) { // (the any-VFO body stores at once: an ordinary conditional store)
            if (held.units == 1 && lane >= held.jmin && lane < held.nout)
                gstv2(out + (size_t)(held.gbase + lane), held.one);
        } else if constexpr (DEPTH == 2) {
            const __amdgpu_buffer_rsrc_t out_rsrc = stream_rsrc(out);
            // (a lane reads back what it wrote itself: no fence needed; before the first chunk the LDS holds anything -- and
            // units is 0, so nothing is stored)
            const bool mine = held.units == 2 && (((held.base >> 4) + lane) << 4) >= first_out && lane <= held.lv;
            const unsigned off = mine ? 8u * (unsigned)((held.base >> 2) + lane * 4) : kNoStore;
            const v4f *park = reinterpret_cast<const v4f *>(lds) + 2 * lane;
            bst4(out_rsrc, off, park[0]);
            bst4(out_rsrc, off + 16u, park[1]);
        } else {
            const __amdgpu_buffer_rsrc_t out_rsrc = stream_rsrc(out);
            // outputs below jmin belong to the warm-up of a segment that starts inside the frame
            const bool mine = held.units == 1 && lane >= held.jmin && lane < held.nout;
            bst2(out_rsrc, mine ? 8u * (unsigned)(held.gbase + lane) : kNoStore, held.one);
        }
        held.units = 0;
    };
    int pair_base = -1; // >= 0: the stage-2 outputs of the chunk at this position wait in A_3 for the next chunk's (paired stages)
    for (int base = W.s_begin; base < W.s_end; base += kChunk) {
        const int valid = min(kChunk, D.n_in - base);
        const int p16 = (base >> 4) + lane;               // this lane's run, in units of 16 samples
        const bool emit = base + kChunk > first_out;      // the chunk reaches into the emitted range
        const bool emit_l = (p16 << 4) >= first_out;      // ... and this lane's run lies inside it
        const bool save = base + valid == D.n_in;         // the chunk that holds the frame's last sample
        const int lv = (valid >> 4) - 1; // last lane holding real samples
        const bool active = lane <= lv;

        // 1. this lane's run of 16 consecutive samples: 8 coalesced 16-byte loads
        v2f ext0[10 + kRun]; // ext0[10 + t] = x[t]; ext0[0..9] = halo x[-10..-1]
        v2f *x = ext0 + 10;
        if (level0 && raw_mode != kRawTiled) {
            load_run_raw(raw, raw_mode, p16, active, x);
        } else {
            // The lane's position inside its tile is the same in every chunk of the item (the walk advances by exactly one tile
            // per chunk): unit_item is computed once, a chunk adds 512 units.  A shifted walk straddles two tiles; its idle lanes
            // in the frame's last chunk may read the (zero) tile behind the last one, which every tile-layout buffer has.
            load_run_tile(in + (unit_item + (unsigned)((base - W.s_begin) >> 10) * 512u), x);
        }

        // 2. NCO and mixer (nco_mix).  The shaped bodies have this chunk's checkpoint already and request the next one.
        v2f o;
        if constexpr (kShape) {
            o = o_next; // (its load was issued a chunk ago)
            o_next = gldv2(cp_of(base + kChunk < W.s_end ? base + kChunk : base)); // (always issued -- and therefore counted, like the stores)
            flush_held(); // the previous chunk's outputs leave BEHIND this chunk's loads: nothing ever waits for them
        } else {
            o = gldv2(cp_of(base));
        }
        {
            int i0 = phase_frame + base;
            i0 -= i0 >= D.L ? D.L : 0;
            nco_mix<EXACT, ROT>(o, rot, Dp->rk, D.cp + (D.L >> 4), frame_no == origin && base == 0 && lane == 0, i0, kChunk, D.L, x);
        }

        if (dd == 0) {
            // no decimation: decimate[0] is the mixed stream itself
            if (otiled) {
                if (emit_l && active) {
                    float4 *o4 = reinterpret_cast<float4 *>(out);
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        gstv4(o4 + tile_unit(p16 >> 6, i, p16 & 63), cat2(x[2 * i], x[2 * i + 1]));
                }
            } else {
                // natural order wanted: transpose through LDS so the stores are coalesced
                wave_sync();
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    *reinterpret_cast<v4f *>(lds + pad0(lane * kRun + 2 * i)) = cat2(x[2 * i], x[2 * i + 1]);
                wave_sync();
                if (emit) {
                    // pad0(128 i + 2 lane) = 144 i + pad0(2 lane): one base address, constant offsets
                    const v2f *src = lds + pad0(2 * lane);
                    // (a 32-bit sample index per lane on top of the uniform stream pointer: a 64-bit per-lane pointer kept
                    // alive across the chunk loop was what the register allocator spilled)
                    const unsigned at = (unsigned)base + 2u * (unsigned)lane;
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (128 * i + 2 * lane < valid && base + 128 * i + 2 * lane >= first_out)
                            gstv4(reinterpret_cast<float4 *>(out + (at + 128u * i)), *reinterpret_cast<const v4f *>(src + 144 * i));
                }
            }
            continue;
        }

        // 3. stage 0 in registers
        halo_stage0(car0, ext0, lane);
        v2f ext1[10 + 8]; // ext1[10 + t] = y[t] (stage-0 outputs of this lane), ext1[0..9] halo
        v2f *y = ext1 + 10;
        hb_regs<EXACT, 8>(ext0, y);
        if (save && lane == lv) // next frame's stage-0 history: x[size-1-k], k = 1..10
#pragma unroll
            for (int k = 1; k <= kHbHist; ++k)
                gstv2(hb_save + 0 * kHbHist + k - 1, x[15 - k]);

        if (dd == 1) {
            if (emit_l && active) {
                const int g = (base >> 1) + lane * 8;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const size_t pos = otiled ? tile_index<size_t>(g + 2 * i) : (size_t)(g + 2 * i);
                    gstv4(reinterpret_cast<float4 *>(out + pos), cat2(y[2 * i], y[2 * i + 1]));
                }
            }
            continue;
        }

        // 4. stage 1 in registers
        halo_stage1(car1, ext1, lane);
        if (save) { // next frame's stage-1 history: y[size1-1-k]
            if (lane == lv)
#pragma unroll
                for (int k = 1; k <= 7; ++k)
                    gstv2(hb_save + 1 * kHbHist + k - 1, y[7 - k]);
            if (lane == lv - 1)
#pragma unroll
                for (int k = 8; k <= kHbHist; ++k)
                    gstv2(hb_save + 1 * kHbHist + k - 1, y[15 - k]);
        }
        v2f z[4];
        hb_regs<EXACT, 4>(ext1, z);

        if (dd == 2) {
            if (emit_l && active) {
                const int g = (base >> 2) + lane * 4;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if (otiled)
                        gstv4(reinterpret_cast<float4 *>(out + tile_index<size_t>(g + 2 * i)), cat2(z[2 * i], z[2 * i + 1]));
                }
            }
            if constexpr (DM) {
                float2 *dm_tap = ldc(&Dp->tap[par]);
                if (dm_tap && emit_l && active) { // decimate[2] is wanted too (fftVFOSlot, parity tests): natural order
                    const int g = (base >> 2) + lane * 4;
                    gstv4(reinterpret_cast<float4 *>(dm_tap + (size_t)g), cat2(z[0], z[1]));
                    gstv4(reinterpret_cast<float4 *>(dm_tap + (size_t)(g + 2)), cat2(z[2], z[3]));
                }
                demod_chunk<EXACT, METER>(dm, dmc, z, lane, valid >> 2, base >> 2, first_out >> 2, save, macc);
            } else if constexpr (kShape) { // its four outputs wait (in LDS) for the next chunk's loads to be on their way
                v4f *park = reinterpret_cast<v4f *>(lds) + 2 * lane;
                park[0] = cat2(z[0], z[1]);
                park[1] = cat2(z[2], z[3]);
                held.units = 2, held.base = base, held.lv = lv;
            } else if (!otiled && emit_l && active) {
                const int g = (base >> 2) + lane * 4;
                gstv4(reinterpret_cast<float4 *>(out + (size_t)g), cat2(z[0], z[1]));
                gstv4(reinterpret_cast<float4 *>(out + (size_t)(g + 2)), cat2(z[2], z[3]));
            }
            continue;
        }

        // 5. stages >= 2 in LDS: this lane's 4 stage-2 inputs go to A_2, then the generic stage
        {
            v2f *A2 = lds + stage_offset(2) + kCarry + lane * 4;
            *reinterpret_cast<v4f *>(A2) = cat2(z[0], z[1]);
            *reinterpret_cast<v4f *>(A2 + 2) = cat2(z[2], z[3]);
        }
        if (kShape && valid == kChunk && !save && dd == kFixedDepth) { // (uniform) a full chunk, not the frame's last (the shaped body of a d = 5 leaf only)
            // stage 2 every chunk; stages 3 and 4 every second chunk on both chunks' stage-2 outputs -- when the NEXT chunk
            // of this item is such a chunk too (otherwise this one is finished alone: nothing pending ever meets another path)
            if (pair_base < 0 && base + kChunk < W.s_end && base + 2 * kChunk < D.n_in) {
                hb_stage_fixed1<EXACT, 2, kFixedDepth, 1>(lds, held, 0, 0, lane);
                pair_base = base;
                continue;
            }
            if (pair_base >= 0) {
                hb_stage_fixed1<EXACT, 2, kFixedDepth, 1, (kChunk >> 3)>(lds, held, 0, 0, lane);
                // outputs below jmin belong to the warm-up of a segment that starts inside the frame
                hb_stage_fixed<EXACT, 3, kFixedDepth, 2>(lds, held, pair_base >> dd, max(0, (first_out - pair_base) >> dd), lane);
                pair_base = -1;
                if constexpr (!kShape)
                    flush_held();
                continue;
            }
            const int jmin = max(0, (first_out - base) >> dd), gbase = base >> dd;
            hb_stage_fixed<EXACT, 2, kFixedDepth, 1>(lds, held, gbase, jmin, lane);
            if constexpr (!kShape)
                flush_held();
            continue;
        }
        for (int s = kRegStages; s < dd; ++s) {
            hb_stage_lds<EXACT>(lds + stage_offset(s), lds + stage_offset(s + 1), out, base >> dd, otiled != 0, s + 1 == dd,
                                max(0, (first_out - base) >> dd), valid >> s, lane, save, hb_save + s * kHbHist);
        }
    }
    flush_held(); // the last chunk's outputs
    if constexpr (DM && METER) {
        const int rel = ldc(&dmc.Kp->meter_rel);
        meter_wave_store(macc, reinterpret_cast<unsigned char *>(ldc(&dmc.Kp->pay[par])) + (rel & ~15) + 16 * (first_out >> (rel & 15)), lane);
    }
}

// ------------------------------------------------------------------------------------ late_item
// vfo::usb_decimdemod's first half (vfo.cpp:334-356) for a d = 0 leaf, INSIDE the mix wave: NCO + mixer as in mix_item,
// then the decimating low-pass on the mixed samples while they are still on the CU,
//     z'[k] = sum_{t < Nd} hd[t] * x[L k - Nd + t]         (FIR::FIRUpdateAndProcess: the (Nd+1)-slot ring leaves the newest
//                                                            sample x[L k] out, dsp.cpp:59-71; FIRUpdate for the samples
//                                                            in between, dsp.cpp:150-154; the phase counter restarts with
//                                                            every frame, vfo.cpp:338-339, and frames are multiples of L)
// so that only z' (1 / L of the bytes) goes to HBM: the two-kernel form wrote the mixed 240 kS/s stream for
// k_late_decimate4 to read back, 246 MB per frame on BASELINE config 4.  One accumulator per output and component, taps in
// ascending order, every product and sum rounded (EXACT): the reference's summation, bit for bit.
//
// A chunk is LateGeom<L>::kChunkLen samples (960 | 1008): kMixLanes lanes replay the NCO and mix 16 consecutive samples each,
// write them to LDS as rows of 3 L samples (row stride kStride: the b64 reads below are conflict-free), and lane l then
// computes the three outputs k = base / L + 3 l + r from ONE pass over the 3 L - 1 + Nd samples that end in its row: window
// sample u of lane l sits at l * kStride + const(u), the taps are wave-uniform scalars.  The last kCarryRows rows of a chunk
// are the next chunk's history; the frame's last late_hist<L>() mixed samples are the next frame's (hb[]).
template <bool EXACT, int LD, bool ROT>
__device__ __forceinline__ void late_item(const K1Vfo *__restrict__ vfos, const K1Work W, unsigned long long frame_no, unsigned char *smem,
                                          int lane)
{
    using G = LateGeom<LD>;
    constexpr int N = G::kTaps, kRow = G::kRow, kStride = G::kStride, kHc = late_hist<LD>();
    constexpr int kCarryElems = G::kCarryRows * kStride;
    v2f *buf = reinterpret_cast<v2f *>(smem); // [(kCarryRows + kRows) * kStride]; sample p of the chunk (p >= -kHc) sits in row (p + kHc) / kRow
    float *sh = reinterpret_cast<float *>(smem + late_window_bytes<LD>()); // the taps, zero-padded to kLateTapPad floats
    const int par = (int)(frame_no & 1ull);
    const K1Vfo *Dp = vfos + W.vfo;
    struct {
        const float2 *cp;
        int n_in, L;
    } D = {ldc(&Dp->cp), ldc(&Dp->n_in), ldc(&Dp->L)};
    const v2f rot = {ldc(&Dp->rot_re), ldc(&Dp->rot_im)};
    const float4 *in = reinterpret_cast<const float4 *>(ldc(&Dp->in[par]));
    float2 *zout = ldc(&Dp->out[par]);
    float2 *tap = ldc(&Dp->tap[par]);
    const float2 *hist_load = ldc(&Dp->hb[par]);
    float2 *hist_save = ldc(&Dp->hb[par ^ 1]);
    const float *taps = ldc(&Dp->late_taps);
    const v2f zero2 = {0.f, 0.f};

    // history in front of the segment's first sample: the previous frame's last kHc mixed samples (zero at start-up,
    // dsp.cpp:40-49), or zeros for a segment that starts inside the frame (its first kWarm samples are warm-up)
    for (int t = lane; t < kHc; t += 64)
        buf[(t / kRow) * kStride + t % kRow] = W.s_begin == 0 ? gldv2(hist_load + t) : zero2;
    for (int t = lane; t < kLateTapPad; t += 64)
        sh[t] = t < N ? gld(taps + t) : 0.f;
    // where this lane's 16-sample run goes: it starts in row q0 at column r0 and crosses into row q0 + 1 at sample wr_T
    const int q0 = (16 * lane) / kRow, r0 = 16 * lane - kRow * q0;
    const int wr_lo = (G::kCarryRows + q0) * kStride + r0;
    int wr_T = kRow - r0;
    const v2f *rd = buf + lane * kStride; // window sample u of this lane: rd[(kCarryRows + floor(u / kRow)) * kStride + u mod kRow]
    const unsigned long long origin = ldc(&Dp->origin); // (frame_no >= origin: set between frames)
    const int phase_frame = (int)(((frame_no - origin) * (unsigned long long)D.n_in) % (unsigned long long)D.L);
    // As in mix_item: the checkpoint the whole NCO hangs on is requested a chunk ahead (always issued: a load the compiler can
    // count).  (Holding the chunk's outputs back behind the next chunk's loads, as mix_item's shaped bodies do, measured
    // +2 % on config 4 here -- the parking in the window rows' padding and the three buffer stores cost more than the
    // waits they avoid -- so this body stores where the outputs arise.)
    auto cp_of = [&](int at) {
        int ix = phase_frame + at; // both < L
        ix -= ix >= D.L ? D.L : 0;
        ix += lane * kRun;
        ix -= ix >= D.L ? D.L : 0;
        return D.cp + (ix >> 4);
    };
    v2f o_next = gldv2(cp_of(W.s_begin));
    int kb = W.s_begin / LD; // index of the first output of the chunk (s_begin is a multiple of L)
    for (int base = W.s_begin; base < W.s_end; base += G::kChunkLen, kb += G::kChunkLen / LD) {
        const int valid = min(G::kChunkLen, D.n_in - base);
        // 1. this lane's run of 16 consecutive samples out of the parent's tile-layout stream.  (Lanes past the chunk or
        //    the frame read on into the stream's spare tile: finite values nobody uses.)
        const unsigned run = (unsigned)(base >> 4) + (unsigned)lane;
        const float4 *src = in + ((run >> 6) * 512u + (run & 63u));
        v2f x[kRun];
        load_run_tile(src, x);
        // 2. NCO and mixer, exactly as in mix_item
        const v2f o = o_next; // (its load was issued a chunk ago)
        o_next = gldv2(cp_of(base + G::kChunkLen < W.s_end ? base + G::kChunkLen : base)); // (always issued, hence counted)
        {
            int i0 = phase_frame + base;
            i0 -= i0 >= D.L ? D.L : 0;
            // (kChunk, not kChunkLen: the lanes past the chunk replay entries nobody uses -- up to 64 x 16 of them must not wrap either)
            nco_mix<EXACT, ROT>(o, rot, Dp->rk, D.cp + (D.L >> 4), frame_no == origin && base == 0 && lane == 0, i0, kChunk, D.L, x);
        }
        if (tap && lane < G::kMixLanes && 16 * lane < valid && base + 16 * lane >= W.s_first_out) {
            // decimate[0] is wanted (the GUI's spectrum tap, parity tests)
            float4 *t4 = reinterpret_cast<float4 *>(tap + (size_t)(base + 16 * lane));
#pragma unroll
            for (int i = 0; i < 8; ++i)
                gstv4(t4 + i, cat2(x[2 * i], x[2 * i + 1]));
        }
        // 3. to LDS, rows of 3 L samples
        wave_sync(); // the previous chunk's window reads and its carry rows are done
        if (LD == 6 || !EXACT) // (16 selects per chunk instead of 16 addresses kept across the loop -- there they spill; exact /5 keeps them)
            asm volatile("" : "+v"(wr_T));
        if (lane < G::kMixLanes) {
#pragma unroll
            for (int i = 0; i < kRun; ++i)
                buf[wr_lo + i + (i >= wr_T ? kStride - kRow : 0)] = x[i];
        }
        wave_sync();
        // 4. three outputs per lane from one pass over the window, a row of it at a time.  The taps come as broadcast b128
        //    reads (the same address in every lane): as scalars they would be SGPR PAIRS (a packed instruction's scalar
        //    operand is 64 bits wide), twice the SGPR file.  Window samples are read two at a time (b128) where the row
        //    stride keeps pairs 16-byte aligned; single b64 reads otherwise.
        if (lane < G::kRows) {
            v2f acc[3] = {zero2, zero2, zero2};
            static_for<G::kCarryRows + 1>([&](auto row_ic) {
                constexpr int fl = decltype(row_ic)::value - G::kCarryRows; // window row, -kCarryRows .. 0
                constexpr int u_lo = kRow * fl < -N ? -N : kRow * fl, u_hi = kRow * (fl + 1) > 2 * LD ? 2 * LD : kRow * (fl + 1);
                // taps this row touches: t = u - L r + N for u in [u_lo, u_hi), r in 0..2
                constexpr int t_lo = (u_lo + N - 2 * LD < 0 ? 0 : u_lo + N - 2 * LD) & ~3;
                constexpr int kHv = (kRow + 2 * LD + 8) / 2;
                v2f hv[kHv]; // tap PAIRS (t_lo + 2 q, + 1): a packed multiply takes either half for both of its lanes
#pragma unroll
                for (int g = 0; g < kHv / 2; ++g)
                    if (t_lo + 4 * g < N && t_lo + 4 * g < u_hi + N) {
                        const v4f q = *reinterpret_cast<const v4f *>(sh + t_lo + 4 * g);
                        hv[2 * g] = lo2(q), hv[2 * g + 1] = hi2(q);
                    }
                const v2f *row = rd + (G::kCarryRows + fl) * kStride;
                v2f w[kRow];
#pragma unroll
                for (int col = 0; col < kRow; ++col) {
                    const int u = kRow * fl + col;
                    if (u < u_lo || u >= u_hi)
                        continue;
                    const bool pairs = kStride % 2 == 0;
                    if (pairs && col % 2 == 0 && col + 1 < kRow && u + 1 < u_hi) {
                        const v4f q = *reinterpret_cast<const v4f *>(row + col);
                        w[col] = lo2(q), w[col + 1] = hi2(q);
                    } else if (!(pairs && col % 2 == 1 && u - 1 >= u_lo)) {
                        w[col] = row[col];
                    }
                }
                static_for<kRow>([&](auto col_ic) {
                    constexpr int col = decltype(col_ic)::value, u = kRow * fl + col;
                    if constexpr (u >= u_lo && u < u_hi) {
                        // output r takes tap t_r = u - L r + N of this sample if 0 <= t_r < N: r in [r_lo, r_hi]
                        constexpr int i0 = u + N - t_lo, i1 = i0 - LD, i2 = i0 - 2 * LD; // tap index - t_lo per output
                        constexpr bool on0 = u + N >= 0 && u + N < N, on1 = u - LD + N >= 0 && u - LD + N < N, on2 = u - 2 * LD + N >= 0 && u - 2 * LD + N < N;
                        if constexpr (on0 && on1 && on2)
                            fir_mac3<EXACT, i0 & 1, i1 & 1, i2 & 1>(acc[0], acc[1], acc[2], hv[i0 >> 1], hv[i1 >> 1], hv[i2 >> 1], w[col]);
                        else if constexpr (on0 && on1)
                            fir_mac2<EXACT, i0 & 1, i1 & 1>(acc[0], acc[1], hv[i0 >> 1], hv[i1 >> 1], w[col]);
                        else if constexpr (on1 && on2)
                            fir_mac2<EXACT, i1 & 1, i2 & 1>(acc[1], acc[2], hv[i1 >> 1], hv[i2 >> 1], w[col]);
                        else if constexpr (on0)
                            fir_mac1<EXACT, i0 & 1>(acc[0], hv[i0 >> 1], w[col]);
                        else if constexpr (on2)
                            fir_mac1<EXACT, i2 & 1>(acc[2], hv[i2 >> 1], w[col]);
                        else
                            static_assert(!on1, "a window sample feeds a contiguous range of outputs");
                    }
                });
                __builtin_amdgcn_sched_barrier(0); // a row's reads stay in the row (all hoisted to the top they spill)
            });
            const int pos = base + kRow * lane; // input position L k of the lane's first output
#pragma unroll
            for (int r = 0; r < 3; ++r)
                if (pos + LD * r >= W.s_first_out && kRow * lane + LD * r < valid)
                    gstv2(zout + (size_t)(kb + 3 * lane + r), acc[r]);
        }
        wave_sync();
        if (base + valid == D.n_in) {
            // the frame's last kHc mixed samples are the next frame's history (sample valid - kHc + t of this chunk)
            int lane_here = lane; // (the per-lane address is computed HERE: hoisted above the chunk loop it is one live 64-bit value too many)
            asm volatile("" : "+v"(lane_here));
            for (int t = lane_here; t < kHc; t += 64) {
                const int pp = valid + t;
                gstv2(hist_save + t, buf[(pp / kRow) * kStride + pp % kRow]);
            }
        } else {
            // the last kCarryRows rows become the next chunk's history rows
            v2f c0 = zero2, c1 = zero2;
            if (lane < kCarryElems)
                c0 = buf[G::kRows * kStride + lane];
            if (kCarryElems > 64 && lane + 64 < kCarryElems)
                c1 = buf[G::kRows * kStride + lane + 64];
            wave_sync();
            if (lane < kCarryElems)
                buf[lane] = c0;
            if (kCarryElems > 64 && lane + 64 < kCarryElems)
                buf[lane + 64] = c1;
        }
    }
}

// ------------------------------------------------------------------------------------ run_item, k_mix_decimate
// which body a work item runs: the fused late decimation for the leaves marked so at finalize, the half-band cascade otherwise
template <bool EXACT, bool ROT, bool METER>
__device__ __forceinline__ void run_item(const K1Vfo *__restrict__ vfos, const K1Work W, unsigned long long frame_no,
                                         const void *__restrict__ raw, int raw_mode, bool level0, unsigned char *smem, int lane)
{
    const int late = ldc(&vfos[W.vfo].late_L);
    if (late == 5)
        late_item<EXACT, 5, ROT>(vfos, W, frame_no, smem, lane);
    else if (late == 6)
        late_item<EXACT, 6, ROT>(vfos, W, frame_no, smem, lane);
    else {
        // a leaf fed from a tile-layout stream: the two shapes of the reference's sub VFOs have bodies of their own (0: any VFO)
        const bool leaf_on_tiles = !(level0 && raw_mode != kRawTiled) && !ldc(&vfos[W.vfo].out_tiled);
        const int d = ldc(&vfos[W.vfo].d);
        const int shape = leaf_on_tiles && d == kFixedDepth ? kFixedDepth : leaf_on_tiles && d == 2 ? 2 : 0;
        if (shape == 2 && ldc(&vfos[W.vfo].dm) != nullptr) // (set at finalize for exactly such leaves: option fuse_demod)
            mix_item<EXACT, 2, ROT, true, METER>(vfos, W, frame_no, raw, raw_mode, false, smem, lane);
        else if (shape == kFixedDepth)
            mix_item<EXACT, kFixedDepth, ROT>(vfos, W, frame_no, raw, raw_mode, false, smem, lane);
        else if (shape == 2)
            mix_item<EXACT, 2, ROT>(vfos, W, frame_no, raw, raw_mode, false, smem, lane);
        else
            mix_item<EXACT, -1, ROT>(vfos, W, frame_no, raw, raw_mode, level0, smem, lane);
    }
}

// One wave per workgroup, one workgroup per K1Work.  LEVEL only gives the root launch and the sub
// launches distinct kernel names in profiles.
// METER: option "meter" (the fused-demodulation items write output meters).
// PARK: option "park" (the items of a parked leaf return at once; ParkArg, sdrx_dev.h).
template <bool EXACT, int LEVEL, bool ROT = !EXACT, bool METER = false, bool PARK = false>
__global__ __launch_bounds__(64, kK1MinWaves) void k_mix_decimate(const K1Vfo *__restrict__ vfos, const K1Work *__restrict__ work,
                                                     unsigned long long frame_no, const void *__restrict__ raw, int raw_mode, ParkArg<PARK> P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if constexpr (PARK)
        if (ldc(P.act + ldc(&work[blockIdx.x].vfo)) == 0)
            return;
    run_item<EXACT, ROT, METER>(vfos, work[blockIdx.x], frame_no, raw, raw_mode, LEVEL == 0, smem, (int)threadIdx.x);
}
