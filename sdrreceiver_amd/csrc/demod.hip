// demod.hip -- vfo::usb_demod (vfo.cpp:300-332; the tail of vfo::usb_decimdemod, vfo.cpp:350-364, is the same code): Hilbert
// filter, delayed I minus it, audio low-pass, int16.  Three forms of the same sums: demod_chunk, inside a d = 2 leaf's mix wave
// (mix.hip, option fuse_demod); demod_block, a 256-thread block per 1024 outputs, as the kernel k_usb_demod and inside
// k_levels_tail (levels.hip); and k_lpf_long, the audio low-pass alone when it is longer than kMaxFir taps.
// Relies on dev_helpers.hip (ldc, gld*, static_for, wave_sync, v16f) and meter.hip (usb_difference, quantise, meter_*).
// demod_lds_bytes(), the LDS of a mix wave that runs demod_chunk, is in mix.hip beside the wave's own.

// ------------------------------------------------------------------------------------ demod_chunk
// ---- the USB demodulation INSIDE the leaf's wave (vfo::usb_demod, vfo.cpp:300-332) -----------------------------------------
// A d = 2 leaf below a parent (the reference's 48 kS/s sub VFOs: 83 % of BASELINE config 3's demodulation work) turns every
// 1024-sample chunk into 256 stream samples, four per lane -- and demodulates them on the spot: the leaf's cf32 stream never
// reaches HBM (round 5: 63 MB written by the mix launch and 75 MB read back by k_usb_demod per frame of config 3), only
// the int16 payload does.  Same arithmetic, same order as demod_block (one accumulator per output, taps ascending, every
// product and sum rounded in the exact arithmetic):
//   usb[m]  = I[m-62] - sum_{s<62} hnz[s] Q[m-123+2s]       (the 62 odd Hilbert taps; the even ones are exactly 0)
//   usb'[m] = sum_{i<N} hu[i] usb[m-N+i]                    (FIR::FIRUpdateAndProcess: newest sample excluded, dsp.cpp:59-71)
//   out[m]  = short(usb' * gain * 32768.0)
// LDS of the wave (floats; all histories in FRONT of the chunk's new values, so a window is one contiguous run):
//   QO [62 | 128]   odd-indexed Q of the stream (local index 2j+1 -> entry 62 + j): what the EVEN outputs read
//   QE [3 + 62 | 128]  even-indexed Q, stored 3 floats up so that the b128 window reads of the odd outputs are aligned
//   I  [2 + 62 | 256]  I, stored 2 floats up so that a lane's four new values are one aligned b128 write
//   U  [Nh | 256 | 8]  usb: Nh = N rounded up to a multiple of 4 values of history, then the chunk's, then zeros the low-pass
//                      reads under its zero padding taps
//   H  [N + 15]        the low-pass taps with 3 zeros in front (K2Vfo::lpf_pad)
// Output t = p + 8 q + 2 rr of lane (p = lane / 32, q = lane % 32) -- four outputs of equal parity share one contiguous run of
// 65 plane entries (17 b128 reads for 248 MACs), the Hilbert taps are wave-uniform scalars (re-requested every chunk: 62 SGPRs
// that are free again for the mix phase).  The low-pass then takes four CONSECUTIVE outputs per lane from U.
// Between chunks the last 62 / 62 / 62 / Nh entries move to the front; between frames they live in K2Vfo::state (256 floats per
// frame parity: QO | QE | I | U at 64-float strides), zero at start-up like every filter state of the reference (dsp.cpp:40-49).
constexpr int kDmHist = 62;
constexpr int kDmQO = 0, kDmQE = 192, kDmI = 388, kDmU = 708, kDmH = 1036, kDmFloats = 1116;
constexpr int kDmMaxLpf = 64; // longest audio low-pass the wave applies itself (the reference's 10 kHz filter at 48 kS/s has 47 taps)
static_assert(kDmQE - kDmQO >= kDmHist + 128 + 2 && kDmI - kDmQE >= 3 + kDmHist + 128 + 3 && kDmU - kDmI >= 2 + kDmHist + 256, "plane sizes");
static_assert(kDmH - kDmU >= kDmMaxLpf + 256 + 8 && kDmFloats - kDmH >= kDmMaxLpf + 15, "usb / tap sizes");
static_assert(kDmQE % 4 == 0 && kDmI % 4 == 0 && kDmU % 4 == 0 && kDmH % 4 == 0, "b128 alignment of the arrays");

struct DemodCtx { // wave-uniform (SGPRs): as little as possible lives across the mix phase -- the descriptor's fields are
    const K2Vfo *Kp; //   re-read (scalar loads from the constant address space) where a chunk needs them
    int par, nlpf, Nh;
};
__device__ __forceinline__ void demod_prologue(float *dm, const K2Vfo *Kp, int par, bool from_state, int lane, DemodCtx &C)
{
    C.Kp = Kp;
    C.par = par;
    C.nlpf = ldc(&Kp->nlpf);
    C.Nh = (C.nlpf + 3) & ~3;
    const float *st = ldc(&Kp->state[par]);
    const float *lpf = ldc(&Kp->lpf_pad);
    // all loads first, then the LDS writes
    float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f, t0 = 0.f, t1 = 0.f;
    if (from_state && lane < kDmHist)
        h0 = gld(st + lane), h1 = gld(st + 64 + lane), h2 = gld(st + 128 + lane);
    if (from_state && lane < C.Nh)
        h3 = gld(st + 192 + lane);
    if (lane < C.nlpf + 15 && C.nlpf > 0)
        t0 = gld(lpf + lane);
    if (lane + 64 < C.nlpf + 15 && C.nlpf > 0)
        t1 = gld(lpf + lane + 64);
    const v4f z4 = {0.f, 0.f, 0.f, 0.f};
    for (int t = lane; t < kDmFloats / 4; t += 64)
        reinterpret_cast<v4f *>(dm)[t] = z4;
    wave_sync();
    if (lane < kDmHist)
        dm[kDmQO + lane] = h0, dm[kDmQE + 3 + lane] = h1, dm[kDmI + 2 + lane] = h2;
    if (lane < C.Nh)
        dm[kDmU + lane] = h3;
    dm[kDmH + lane] = t0;
    if (lane + 64 < kDmMaxLpf + 15)
        dm[kDmH + 64 + lane] = t1;
}
// One chunk: z[0..3] = the lane's stream samples 4 lane .. 4 lane + 3 of the chunk (stream index g0 + ...), nv = how many of
// the chunk's 256 are real (a multiple of 4), fo = first stream index this item emits, `last` = the chunk holds the frame's end.
// METER: the emitted values are folded into `macc` (the item's record, written by mix_item at its end).
template <bool EXACT, bool METER>
__device__ __forceinline__ void demod_chunk(float *dm, const DemodCtx &C, const v2f *z, int lane, int nv, int g0, int fo, bool last,
                                            MeterAcc &macc)
{
    const K2Vfo *Kp = C.Kp;
    asm volatile("" : "+s"(Kp)); // (what is read through it below is read in THIS chunk, not once in front of the chunk loop)
    wave_sync(); // the previous chunk's reads and its hand-over are done
    {
        const v2f qo = {z[1].y, z[3].y};
        *reinterpret_cast<v2f *>(dm + kDmQO + kDmHist + 2 * lane) = qo;
        dm[kDmQE + 3 + kDmHist + 2 * lane] = z[0].y;
        dm[kDmQE + 3 + kDmHist + 2 * lane + 1] = z[2].y;
        const v4f iv = {z[0].x, z[1].x, z[2].x, z[3].x};
        *reinterpret_cast<v4f *>(dm + kDmI + 2 + kDmHist + 4 * lane) = iv;
    }
    wave_sync();
    // ---- Hilbert: four outputs of one parity per lane
    {
        const int p = lane >> 5, q = lane & 31;
        const float *plane = p == 0 ? dm + kDmQO + 4 * q : dm + kDmQE + 4 + 4 * q;
        // The taps sixteen at a time, each batch requested right in front of its pass (every chunk: hoisted out of the chunk
        // loop, or all at once, they would hold 62 SGPRs -- the mix phase needs its own -- and spill into a VGPR that every
        // body of the kernel then loses).  An accumulator still takes its taps in ascending order: pass k has s = 16 k .. 16 k + 15,
        // i.e. plane entries rr + s in 16 k .. 16 k + 18: groups 4 k .. 4 k + 4 (20 b128 reads per chunk instead of 17).
        const float *hnz_all = ldc(&Kp->hnz);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        static_for<4>([&](auto pass_ic) {
            constexpr int pass = decltype(pass_ic)::value, s_lo = 16 * pass, s_hi = s_lo + 16 < kHilbertNz ? s_lo + 16 : kHilbertNz, g_lo = 4 * pass;
            const float *hp = hnz_all + s_lo;
            asm volatile("" : "+s"(hp));
            float hnz[s_hi - s_lo];
#pragma unroll
            for (int s = 0; s < s_hi - s_lo; ++s)
                hnz[s] = ldc(hp + s);
#pragma unroll
            for (int g = g_lo; g < g_lo + 5 && g < 17; ++g) {
                const v4f v4 = *reinterpret_cast<const v4f *>(plane + 4 * g);
                const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int s = 4 * g + e - rr;
                        if (s >= s_lo && s < s_hi) {
                            if (EXACT)
                                acc[rr] = acc[rr] + hnz[s - s_lo] * v[e];
                            else
                                acc[rr] = fmaf(hnz[s - s_lo], v[e], acc[rr]);
                        }
                    }
            }
            __builtin_amdgcn_sched_barrier(0); // (the next batch of taps is not requested while this one is live)
        });
        const int t0 = p + 8 * q;
        const float *iv = dm + kDmI + 2 + t0; // I[t - 62]
        float *u = dm + kDmU + C.Nh + t0;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
            u[2 * rr] = usb_difference(iv[2 * rr], acc[rr]);
    }
    wave_sync();
    // ---- audio low-pass (newest sample excluded) on four consecutive outputs, int16
    {
        const int N = C.nlpf;
        float u4[4];
        if (N > 0) {
            // output 4 lane + rr, tap i reads U[Nh + 4 lane + rr - N + i]; H[i + 3] = hu[i], zeros around
            const float *w = dm + kDmU + (C.Nh - N) + 4 * lane;
            const float *H = dm + kDmH;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            const int groups = (N + 6) / 4;
            for (int g = 0; g < groups; ++g) {
                const v4f v4 = *reinterpret_cast<const v4f *>(w + 4 * g);
                const float v[4] = {v4.x, v4.y, v4.z, v4.w};
                const v4f ha = *reinterpret_cast<const v4f *>(H + 4 * g), hb4 = *reinterpret_cast<const v4f *>(H + 4 * g + 4);
                const float h[8] = {ha.x, ha.y, ha.z, ha.w, hb4.x, hb4.y, hb4.z, hb4.w}; // h[k] = hu[4g + k - 3]
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        if (EXACT)
                            acc[rr] = acc[rr] + h[e - rr + 3] * v[e];
                        else
                            acc[rr] = fmaf(h[e - rr + 3], v[e], acc[rr]);
                    }
            }
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                u4[rr] = acc[rr];
        } else {
            const v4f v4 = *reinterpret_cast<const v4f *>(dm + kDmU + 4 * lane); // (Nh = 0)
            u4[0] = v4.x, u4[1] = v4.y, u4[2] = v4.z, u4[3] = v4.w;
        }
        short o4[4];
        float pq[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
            pq[rr] = quantise(u4[rr] * ldc(&Kp->gain), o4[rr]);
        const int g = g0 + 4 * lane;
        if (4 * lane < nv && g >= fo) { // (nv and fo are multiples of 4: a lane's four outputs are emitted together or not at all)
            const v4s o = {o4[0], o4[1], o4[2], o4[3]};
            *(SDRX_AS1 v4s *)(ldc(&Kp->pay[C.par]) + g) = o;
            float *prequant = ldc(&Kp->prequant);
            if (prequant)
                gst4(reinterpret_cast<float4 *>(prequant + g), make_float4(pq[0], pq[1], pq[2], pq[3]));
            if constexpr (METER)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
                    meter_usb(macc, pq[rr], o4[rr]);
        }
    }
    wave_sync();
    // ---- the last 62 / 62 / 62 / Nh values: the next chunk's history, or -- at the frame's end -- the next frame's
    if (last) {
        const int h = nv >> 1;
        float *state_save = ldc(&Kp->state[C.par ^ 1]);
        if (lane < kDmHist) {
            *(SDRX_AS1 float *)(state_save + lane) = dm[kDmQO + h + lane];
            *(SDRX_AS1 float *)(state_save + 64 + lane) = dm[kDmQE + 3 + h + lane];
            *(SDRX_AS1 float *)(state_save + 128 + lane) = dm[kDmI + 2 + nv + lane];
        }
        if (lane < C.Nh)
            *(SDRX_AS1 float *)(state_save + 192 + lane) = dm[kDmU + nv + lane];
    } else {
        float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
        if (lane < kDmHist)
            a = dm[kDmQO + 128 + lane], b = dm[kDmQE + 3 + 128 + lane], c = dm[kDmI + 2 + 256 + lane];
        if (lane < C.Nh)
            d = dm[kDmU + 256 + lane];
        wave_sync();
        if (lane < kDmHist)
            dm[kDmQO + lane] = a, dm[kDmQE + 3 + lane] = b, dm[kDmI + 2 + lane] = c;
        if (lane < C.Nh)
            dm[kDmU + lane] = d;
    }
}

// ------------------------------------------------------------------------------------ demod_block, k_usb_demod
// USB demodulation + optional audio low-pass + int16 (vfo.cpp:300-332):
//   usb[m]  = I[m-62] - sum_{i<125} hp[i] Q[m-124+i]      DelayThing (dsp.h:101-106) and
//                                                         FIRHilbert (dsp.cpp:218-231, newest
//                                                         sample included; float sum, the
//                                                         subtraction in double)
//   usb'[m] = sum_{i<N} hu[i] usb[m-N+i]                  FIR::FIRUpdateAndProcess, newest excluded
//   out[m]  = short(usb' * gain * 32768.0)                float product, then double
// Only the 62 odd-index Hilbert taps are non-zero (the even ones are exactly 0.0f and adding
// 0*x leaves a float sum unchanged), so the sum runs over those, in index order:
//   sum = sum_{s<62} hnz[s] Q[m - 123 + 2 s].
//
// Blocking: one 256-thread block = 1024 outputs of one VFO.  Outputs of equal parity share their
// Q samples, so Q is staged in LDS as two parity planes and a thread computes 4 same-parity
// outputs from one contiguous run of 65 plane entries (17 ds_read_b128 for 248 MACs); the taps
// are wave-uniform scalar loads held in SGPRs.  The low-pass then takes 4 consecutive outputs per
// thread from the usb values parked in LDS, taps broadcast from LDS.  EXACT keeps one accumulator
// per output and the reference's summation order (4 independent chains per thread give the ILP).
constexpr int kDemodTile = 1024;

// ---- the non-exact arithmetics' MACs, two outputs per instruction ----------------------------------------------------------
// Four outputs r = 0..3 of a thread share a window: at window entry k output r takes tap h[k - r] (the Hilbert sum: outputs
// t0 + 2 r on one parity plane; the audio low-pass: four consecutive outputs).  As scalar FMAs that is four instructions per
// entry, and a v_fma_f32 pairs with another wave's instruction far less often than a two-operand v_mul / v_add does (37 % of
// k_usb_demod's instructions in the tolerance arithmetic against 80 % in the exact one: profiles/pmc_config3_tolerance.json).  As
// PACKED FMAs it is two: A = (out0, out1) += (h[k], h[k-1]) * v[k], B = (out2, out3) += (h[k-2], h[k-3]) * v[k].  The pair
// (h[k-1], h[k]) is an aligned register pair of one of two copies of the taps -- E: pairs (h[2j-1], h[2j]), O: pairs
// (h[2j], h[2j+1]) -- taken SWAPPED (op_sel / op_sel_hi on the tap operand), v[k] either half of an aligned pair for both
// lanes.  Every lane of every instruction is the same fma(h, v, acc) in the same order as the scalar form: bit-identical.
template <int H>
__device__ __forceinline__ void pk_fma2_s(v2f &A, v2f &B, v2f pa, v2f pb, v2f vv) // taps: scalar register pairs
{
    asm("v_pk_fma_f32 %0, %2, %4, %0 op_sel:[1,%5,0] op_sel_hi:[0,%5,1]\n\t"
        "v_pk_fma_f32 %1, %3, %4, %1 op_sel:[1,%5,0] op_sel_hi:[0,%5,1]"
        : "+v"(A), "+v"(B)
        : "s"(pa), "s"(pb), "v"(vv), "n"(H));
}
// the same in the exact arithmetic: product and sum rounded separately (v_pk_mul_f32, v_pk_add_f32), the two products first
template <int H>
__device__ __forceinline__ void pk_mac2_s(v2f &A, v2f &B, v2f pa, v2f pb, v2f vv)
{
    v2f ta, tb;
    asm("v_pk_mul_f32 %2, %4, %6 op_sel:[1,%7] op_sel_hi:[0,%7]\n\t"
        "v_pk_mul_f32 %3, %5, %6 op_sel:[1,%7] op_sel_hi:[0,%7]\n\t"
        "v_pk_add_f32 %0, %0, %2\n\t"
        "v_pk_add_f32 %1, %1, %3"
        : "+v"(A), "+v"(B), "=&v"(ta), "=&v"(tb)
        : "s"(pa), "s"(pb), "v"(vv), "n"(H));
}
// pair i (0..8) of the 18 floats (x16, x2) a pass has loaded
template <int I>
__device__ __forceinline__ v2f pair_of(v16f a, v2f b)
{
    if constexpr (I < 8)
        return __builtin_shufflevector(a, a, 2 * I, 2 * I + 1);
    else
        return b;
}
// The Hilbert sum of four same-parity outputs: plane[k], k = 0 .. 64 (17 aligned b128 reads), taps hE[m] = h[m - 3], hO[m] =
// h[m - 2] (zeros outside 0 .. 61; K2Vfo::hnz_e / hnz_o, 96 floats each): pair j' of hE = (h[2j'-3], h[2j'-2]), of hO =
// (h[2j'-2], h[2j'-1]).  Entry k takes P(k) = (h[k-1], h[k]) for A and P(k-2) for B: P(k) = pair k/2 + 1 of hE (k even) or
// of hO (k odd).  Sixteen entries per pass, the 2 x 18 floats of taps a pass needs requested in front of it.
template <bool EXACT>
__device__ __forceinline__ void hilbert4_packed(const float *plane, const float *hE, const float *hO, float (&acc)[4])
{
    v2f A = {0.f, 0.f}, B = {0.f, 0.f};
    static_for<5>([&](auto pass_ic) {
        constexpr int pass = decltype(pass_ic)::value, nk = pass < 4 ? 16 : 1; // (entry 64 feeds out3 alone: h[61])
        const float *pe = hE + 16 * pass, *po = hO + 16 * pass;
        asm volatile("" : "+s"(pe), "+s"(po)); // (a pass's taps are requested here, not five passes' worth up front)
        const v16f e16 = *(const SDRX_AS4 v16f *)pe, o16 = *(const SDRX_AS4 v16f *)po;
        const v2f e2 = *(const SDRX_AS4 v2f *)(pe + 16), o2 = *(const SDRX_AS4 v2f *)(po + 16);
        static_for<(nk + 3) / 4>([&](auto g_ic) {
            constexpr int g = decltype(g_ic)::value;
            const v4f v4 = *reinterpret_cast<const v4f *>(plane + 16 * pass + 4 * g);
            static_for<(nk < 4 ? nk : 4)>([&](auto e_ic) {
                constexpr int e = decltype(e_ic)::value, kk = 4 * g + e, iA = kk / 2 + 1, iB = iA - 1;
                const v2f vv = e < 2 ? lo2(v4) : hi2(v4);
                if constexpr (EXACT) {
                    if constexpr (kk % 2 == 0)
                        pk_mac2_s<0>(A, B, pair_of<iA>(e16, e2), pair_of<iB>(e16, e2), vv);
                    else
                        pk_mac2_s<1>(A, B, pair_of<iA>(o16, o2), pair_of<iB>(o16, o2), vv);
                } else {
                    if constexpr (kk % 2 == 0)
                        pk_fma2_s<0>(A, B, pair_of<iA>(e16, e2), pair_of<iB>(e16, e2), vv);
                    else
                        pk_fma2_s<1>(A, B, pair_of<iA>(o16, o2), pair_of<iB>(o16, o2), vv);
                }
            });
        });
        __builtin_amdgcn_sched_barrier(0);
    });
    acc[0] = A.x, acc[1] = A.y, acc[2] = B.x, acc[3] = B.y;
}

// The block's window is staged in 16-byte UNITS: unit j = the sample pair at offsets r = 2 j, 2 j + 1 from `lo`, one per thread
// and iteration, kStageUnits in all.  Every unit has a home in LDS whether the block wants it or not (no test per sample):
//   sP0[j + 3] = Q(2 j)   sP1[j] = Q(2 j + 1)   sI[2 j - 62], sI[2 j - 61] = I(2 j), I(2 j + 1)   (sI[t] = I of usb value t)
// which takes kDelay floats of slack in FRONT of sI for the units j < 31.
constexpr int kStageIters = 3, kStageUnits = 256 * kStageIters;
constexpr int kWindowUnits = (kDemodTile + kHilbert - 1) / 2; // units a block can want: nr <= 1148 (demod_block)
constexpr int kSiFront = 64;                                  // >= kDelay, a multiple of 4
static_assert(kWindowUnits > 256 * (kStageIters - 1) && kWindowUnits <= kStageUnits && kSiFront >= kDelay, "staging covers the window");
struct DemodLds { // LDS of one 256-thread demodulation block
    alignas(16) float sP0[kStageUnits + 4]; // even offsets from `lo`, stored shifted by +3
    alignas(16) float sP1[kStageUnits];     // odd offsets
    alignas(16) float sIf[kSiFront + 2 * kStageUnits - kDelay + 2]; // sI = sIf + kSiFront
    alignas(16) float sU[kDemodTile + kMaxFir + 16];
    alignas(16) float sH[kMaxFir + 16];  // sH[m] = hu[m - 3]
};
static_assert(sizeof(DemodLds) % 16 == 0, "DemodLds is a whole number of 16-byte units");
static_assert(7 * sizeof(DemodLds) <= 160 * 1024, "seven blocks of k_usb_demod per CU (its 7 waves per SIMD)");

// METER: the block's output meter goes to the leaf's record blk (K2Vfo::meter_rel; not for a leaf with a long low-pass:
// k_lpf_long meters that one).
template <bool EXACT, bool METER>
__device__ __forceinline__ void demod_block(const K2Vfo *__restrict__ vfos, const BlockWork bw, unsigned long long frame_no, DemodLds &S,
                                            int tid)
{
    float *sP0 = S.sP0, *sP1 = S.sP1, *sI = S.sIf + kSiFront, *sU = S.sU, *sH = S.sH;
    const K2Vfo *Dp = vfos + bw.vfo;
    const int blk = bw.blk;
    const int par = (int)(frame_no & 1ull);
    struct {
        const float *hnz, *lpf;
        short *pay;
        float *prequant;
        float gain;
        int H, n, nlpf, tile;
    } D = {ldc(&Dp->hnz), ldc(&Dp->lpf_pad), ldc(&Dp->pay[par]), ldc(&Dp->prequant), ldc(&Dp->gain),
           ldc(&Dp->H),   ldc(&Dp->n),       ldc(&Dp->nlpf),     ldc(&Dp->tile)};
    float *usb_out = ldc(&Dp->usb_out[par]); // non-null: a long low-pass follows in k_lpf_long
    const float2 *sbase = ldc(&Dp->s[par]);
    float2 *snext = ldc(&Dp->s_next[par]);
    const int m0 = blk * D.tile;
    if (m0 >= D.n && blk != 0) {
        if constexpr (METER) // (the whole block: no value, an empty record)
            if (!usb_out && tid == 0)
                meter_put(reinterpret_cast<unsigned char *>(D.pay) + ldc(&Dp->meter_rel) + 16 * blk, meter_zero());
        return;
    }
    // The 62 Hilbert taps, read before this kernel has stored anything so the compiler can use
    // wave-uniform scalar loads and keep them in SGPRs for the whole block.  (The non-exact arithmetics take them pass by
    // pass as register PAIRS instead: hilbert4_packed.  The exact arithmetic's sum packed -- v_pk_mul / v_pk_add -- was
    // 1-3 % slower on all three workloads.)
    constexpr bool kPackedHilbert = !EXACT;
    float hnz[kHilbertNz];
    if constexpr (!kPackedHilbert) {
#pragma unroll
        for (int s = 0; s < kHilbertNz; ++s)
            hnz[s] = ldc(D.hnz + s);
    }
    if (D.nlpf > 0)
        for (int j = tid; j < D.nlpf + 15; j += 256)
            sH[j] = gld(D.lpf + j);
    if (blk == 0) // history for the next frame: the last H entries of [hist | data]
        for (int j = tid; j < D.H; j += 256)
            gst2(snext + j, gld2(sbase + D.n + j));
    const int N = D.nlpf;
    const int E = N + (N & 1);                  // usb values m0-E .. m0+1023 are computed (t = 0 .. ntv-1)
    const int ntv = D.tile + E;                 // <= 1024: the host shortens the tile of a low-pass VFO by E (one usb pass)
    const int lo = m0 - E - (kHilbert - 1);     // first stream index touched (>= -H)
    // Offsets r = idx - lo in [0, nr), nr = ntv + 124 <= 1148, are what the block wants: kWindowUnits units at most.  H + lo is
    // even and the stream starts on a 16-byte boundary (sdrx_finalize checks both: demod_window_rule), so unit j -- samples
    // lo + 2 j and lo + 2 j + 1 -- is ONE aligned 16-byte load through a resource that ends at sample n: what lies beyond
    // reads 0, dword by dword.  All of this thread's loads are issued before the first LDS write (a rolled load -> wait ->
    // write loop would pay the memory latency once per iteration); the last iteration asks only for units the largest
    // window has (the others would be bytes fetched for nothing) and gets zeros for the rest.
    // Units past nr are written but feed no output that is kept: usb value t reads Q at r = t + 1 + 2 s <= t + 123 and I at
    // sI[t], and only t < ntv is stored to sU below (r <= ntv + 122 < nr, sI[t] from r = t + 62 < nr); the threads
    // whose t runs past ntv compute on them and drop the result.
    const __amdgpu_buffer_rsrc_t win = window_rsrc(sbase, D.H + D.n);
    const unsigned voff = 8u * (unsigned)(D.H + lo) + 16u * (unsigned)tid;
    v4f stage[kStageIters];
#pragma unroll
    for (int it = 0; it < kStageIters; ++it) {
        unsigned off = voff + 4096u * it;
        if (it == kStageIters - 1)
            off = tid < kWindowUnits - 256 * it ? off : kNoLoad;
        stage[it] = bld4(win, off);
    }
#pragma unroll
    for (int it = 0; it < kStageIters; ++it) {
        const int j = tid + 256 * it;
        sP0[j + 3] = stage[it].y;
        sP1[j] = stage[it].w;
        sI[2 * j - kDelay] = stage[it].x; // I[u-62] for u = m0 - E + t, t = 2 j - 62 and the next
        sI[2 * j - kDelay + 1] = stage[it].z;
    }
    __syncthreads();

    // ---- usb: Q index of tap s for value t is r = t + 1 + 2 s
    const int p = tid >> 7, q = tid & 127;      // waves 0-1 take even t, waves 2-3 odd t
    const int soff = (4 - (E - N)) & 3;         // sU shift that makes the low-pass reads 16-byte aligned
    for (int tb = 0; tb < ntv; tb += kDemodTile) {
        const int t0 = tb + p + 8 * q;          // this thread: t0, t0+2, t0+4, t0+6
        if (t0 >= ntv)
            continue;
        const float *plane = p == 0 ? sP1 + (t0 >> 1) : sP0 + 3 + ((t0 + 1) >> 1);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (!kPackedHilbert) {
#pragma unroll
            for (int g = 0; g < 17; ++g) {
                const float4 v4 = *reinterpret_cast<const float4 *>(plane + 4 * g);
                const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int s = 4 * g + e - rr;
                        if (s >= 0 && s < kHilbertNz)
                            acc[rr] = acc[rr] + hnz[s] * v[e];
                    }
            }
        } else {
            hilbert4_packed<EXACT>(plane, ldc(&Dp->hnz_e), ldc(&Dp->hnz_o), acc);
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int t = t0 + 2 * rr;
            if (t < ntv)
                sU[t + soff] = usb_difference(sI[t], acc[rr]);
        }
    }
    if (tid < 8) // read by the low-pass only under its zero padding taps: must be finite (0 * NaN = NaN)
        sU[ntv + soff + tid] = 0.f; // <= 1280 + 3 + 7, inside sU
    __syncthreads();

    // ---- audio low-pass (newest sample excluded) on 4 consecutive outputs, then int16
    asm volatile("" : "+v"(tid)); // (multiples of tid are formed again here, not carried through the Hilbert sum in registers of their own)
    const int j0 = 4 * tid;
    const int m = m0 + j0;
    const bool emits = j0 < D.tile && m < D.n;
    if (!emits && (!METER || usb_out)) // (usb_out: the same for the whole block -- none of its threads reaches the record)
        return;
    // (METER: every thread goes on to the block's record)
    MeterAcc macc = meter_zero();
    if (emits) {
    float u4[4];
    if (N > 0) {
        // output j0+rr, tap i reads usb t = j0 + rr + (E-N) + i; sH[i+3] = hu[i], zeros around
        const float *w = sU + soff + (E - N) + j0; // 16-byte aligned by the choice of soff
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const int groups = (N + 6) / 4;
        // (scalar in every arithmetic: packed like hilbert4_packed, the low-pass has two accumulator chains per thread instead
        // of four and cost config 4 2-3 %; profiles/README.md round 6)
        for (int g = 0; g < groups; ++g) {
            const float4 v4 = *reinterpret_cast<const float4 *>(w + 4 * g);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
            const float4 ha = *reinterpret_cast<const float4 *>(sH + 4 * g), hb4 = *reinterpret_cast<const float4 *>(sH + 4 * g + 4);
            const float h[8] = {ha.x, ha.y, ha.z, ha.w, hb4.x, hb4.y, hb4.z, hb4.w}; // h[k] = hu[4g + k - 3]
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    if (EXACT)
                        acc[rr] = acc[rr] + h[e - rr + 3] * v[e];
                    else
                        acc[rr] = fmaf(h[e - rr + 3], v[e], acc[rr]);
                }
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
            u4[rr] = acc[rr];
    } else {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
            u4[rr] = sU[soff + j0 + rr];
    }
    if (usb_out) { // hand the unfiltered usb values on (k_lpf_long quantises)
        for (int rr = 0; rr < 4 && m + rr < D.n; ++rr)
            *(SDRX_AS1 float *)(usb_out + m + rr) = u4[rr];
        return;
    }
    short o4[4];
    float pq[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        pq[rr] = quantise(u4[rr] * D.gain, o4[rr]);
    }
    if (m + 3 < D.n) {
        v4s o = {o4[0], o4[1], o4[2], o4[3]};
        *(SDRX_AS1 v4s *)(D.pay + m) = o;
        if (D.prequant)
            gst4(reinterpret_cast<float4 *>(D.prequant + m), make_float4(pq[0], pq[1], pq[2], pq[3]));
        if constexpr (METER)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                meter_usb(macc, pq[rr], o4[rr]);
    } else {
        for (int rr = 0; rr < 4 && m + rr < D.n; ++rr) {
            *(SDRX_AS1 short *)(D.pay + m + rr) = o4[rr];
            if (D.prequant)
                *(SDRX_AS1 float *)(D.prequant + m + rr) = pq[rr];
            if constexpr (METER)
                meter_usb(macc, pq[rr], o4[rr]);
        }
    }
    }
    if constexpr (METER)
        meter_block_store(macc, reinterpret_cast<unsigned char *>(D.pay) + ldc(&Dp->meter_rel) + 16 * blk, tid,
                          reinterpret_cast<MeterAcc *>(sP0)); // (the Hilbert planes are done with)
}

// (no occupancy demand: __launch_bounds__(256, 8) -- at most 64 VGPRs, eight 256-thread blocks per CU -- measured 92 us
// against 47 us; profiles/README.md)
template <bool EXACT, bool METER = false, bool PARK = false>
__global__ __launch_bounds__(256, 1) void k_usb_demod(const K2Vfo *__restrict__ vfos, const BlockWork *__restrict__ work,
                                                   unsigned long long frame_no, ParkArg<PARK> P)
{
    __shared__ __attribute__((aligned(16))) DemodLds S;
    if constexpr (PARK)
        if (ldc(P.act + ldc(&work[blockIdx.x].vfo)) == 0)
            return;
    demod_block<EXACT, METER>(vfos, work[blockIdx.x], frame_no, S, (int)threadIdx.x);
}

// ------------------------------------------------------------------------------------ k_lpf_long
// An audio low-pass of more than kMaxFir taps (the reference accepts any filter_bandwidth: 500 Hz at
// 48 kS/s is 925 taps, firfilter.cpp:108-119): usb'[m] = sum_{i<N} hu[i] usb[m-N+i], newest sample
// excluded (FIR::FIRUpdateAndProcess, dsp.cpp:59-71), one accumulator per output in tap order, then the
// same quantisation as k_usb_demod.  256 outputs per block; the block's window of N + 256 usb values sits
// in LDS, the taps are wave-uniform scalar loads.  A rare configuration: correctness first.
template <bool EXACT, bool METER = false, bool PARK = false>
__global__ __launch_bounds__(256) void k_lpf_long(const K4Vfo *__restrict__ vfos, const BlockWork *__restrict__ work, unsigned long long frame_no,
                                                  const int *__restrict__ mrel, ParkArg<PARK> P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *sw = reinterpret_cast<float *>(smem);
    if constexpr (PARK)
        if (ldc(P.act + ldc(&work[blockIdx.x].vfo)) == 0)
            return;
    const K4Vfo *Dp = vfos + ldc(&work[blockIdx.x].vfo);
    const int blk = ldc(&work[blockIdx.x].blk);
    const int par = (int)(frame_no & 1ull);
    const int tid = threadIdx.x;
    const float *taps = ldc(&Dp->taps);
    const int Hu = ldc(&Dp->Hu), n = ldc(&Dp->n), N = ldc(&Dp->nlpf);
    const float gain = ldc(&Dp->gain);
    const float *ubase = ldc(&Dp->u[par]);
    float *unext = ldc(&Dp->u_next[par]);
    short *pay = ldc(&Dp->pay[par]);
    float *prequant = ldc(&Dp->prequant);
    if (blk == 0) // history for the next frame: the last Hu entries of [hist | data]
        for (int j = tid; j < Hu; j += 256)
            *(SDRX_AS1 float *)(unext + j) = gld(ubase + n + j);
    const float *u = ubase + Hu; // sample 0 of this frame
    const int m0 = blk * 256;
    for (int t = tid; t < N + 256; t += 256) { // window: usb[m0 - N .. m0 + 255]
        const int idx = m0 - N + t;
        sw[t] = idx < n ? gld(u + idx) : 0.f;
    }
    __syncthreads();
    const int m = m0 + tid;
    if (!METER && m >= n)
        return;
    MeterAcc macc = meter_zero();
    if (m < n) { // (METER: every thread goes on to the block's record)
    const float *w = sw + tid; // w[i] = usb[m - N + i]
    float acc = 0.f;
    for (int i = 0; i < N; ++i) {
        const float h = ldc(taps + i);
        if (EXACT)
            acc = acc + h * w[i];
        else
            acc = fmaf(h, w[i], acc);
    }
    short q;
    const float pre = quantise(acc * gain, q);
    *(SDRX_AS1 short *)(pay + m) = q;
    if (prequant)
        *(SDRX_AS1 float *)(prequant + m) = pre;
    if constexpr (METER)
        meter_usb(macc, pre, q);
    }
    if constexpr (METER) {
        __shared__ MeterAcc red[4];
        meter_block_store(macc, reinterpret_cast<unsigned char *>(pay) + ldc(mrel + blockIdx.x), tid, red);
    }
}
