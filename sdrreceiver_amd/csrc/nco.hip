// nco.hip -- the oscillator: Oscillator::Oscillator's table recurrence (oscillator.cpp:4-32) replayed from checkpoints, in
// the exact arithmetic (nco_step, nco_step_pk) and as rotations of the checkpoints in the tolerance arithmetic
// (nco_mix_fast*, with the mixer of vfo.cpp:241), and the small kernels that write or patch a VFO's oscillator between
// frames: k_nco_init, k_vfo_retune, k_vfo_reset, k_nco_dump.  mix.hip (nco_mix) is where a chunk uses them.
// Relies on dev_helpers.hip (v2f, cmul, ldc) and on the descriptors of sdrx_dev.h.

// ------------------------------------------------------------------------------------ NCO
// One step of the reference's table recurrence (oscillator.cpp:20-28): v *= rot (complex
// product re = ac - bd, im = ad + bc), then v *= 1.95f - |v|^2.  Strict fp32, no FMA.
__device__ __forceinline__ float2 nco_step(float2 v, float rc, float rs)
{
    float nr = v.x * rc - v.y * rs;
    float ni = v.x * rs + v.y * rc;
    float norm = 1.95f - (nr * nr + ni * ni);
    return make_float2(nr * norm, ni * norm);
}

// The same step on a packed (re, im) pair: 7 instructions instead of 12.
__device__ __forceinline__ v2f nco_step_pk(v2f v, v2f rot)
{
    const v2f n = cmul(v, rot);          // nr = v.x rc - v.y rs, ni = v.x rs + v.y rc
    const v2f sq = n * n;
    const float norm = 1.95f - (sq.x + sq.y);
    return n * norm;
}

// NCO in the tolerance arithmetic (option exact = 0; north_star: "within 1e-5 relative float tolerance").  Once the table's
// amplitude has settled (the stabiliser 1.95f - |v|^2 pulls |v|^2 to 0.95 with the factor -0.9 per step: ~150 entries,
// oscillator.cpp:20-28) a step of the recurrence is a rotation by arg(rot) at constant modulus, plus its own rounding noise.
// So from the EXACT checkpoint c = table[16 j - 1] the 16 entries behind it are rotations of it:  with rk[q] = u^(q+1),
// q = 0..3, computed in double at finalize,  table[b + q] = base * rk[q]  for base = c, then table[b + 3] of the block
// before (four blocks of four; an entry is at most four products away from the checkpoint) -- two-instruction products
// with four wave-uniform constants instead of a 16-deep chain of seven instructions.  Measured against the reference's
// tables (the (Fs, f) pairs of the shipped profiles): max 1.0e-6, rms 2e-7 relative on entries >= 512; a checkpoint is
// never more than 16 entries away, so nothing accumulates over a frame or a run.  Chunks that touch the first kNcoSettle
// entries of the table (start-up ringing; the very first sample's table[L-1]) replay it exactly.
//
// Two samples per statement:  m_k = base * r_k  (the table entries; r_k wave-uniform, an SGPR pair),  x_k = m_k * x_k  (the
// mixer, vfo.cpp:241).  A complex product (a.x b.x - a.y b.y, a.x b.y + a.y b.x) is ONE packed multiply (a.x, a.x) * b and
// ONE packed FMA (a.y, a.y) * (-b.y, b.x) + that: the broadcast of a's halves, the swap of b's and the sign are source
// modifiers (op_sel, op_sel_hi, neg_lo) -- written out because the compiler finds them for one product in eight and
// builds (-b.y, b.x) with a v_xor and a v_mov for the others.  The two samples' instructions alternate, so none reads the
// result of the one before it (gfx950 wants one wait state behind a packed fp32 instruction; nobody inserts it inside an
// asm statement).  Returns m_1 (the later entry: the next block's base).
__device__ __forceinline__ v2f nco_mix_fast2(v2f base, v2f r0, v2f r1, v2f &x0, v2f &x1)
{
    v2f m0, m1, y0, y1; // (results in registers of their own: written in place, the compiler copies the inputs first)
    asm("v_pk_mul_f32 %2, %6, %7 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %3, %6, %8 op_sel_hi:[0,1]\n\t"
        "v_pk_fma_f32 %2, %6, %7, %2 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n\t"
        "v_pk_fma_f32 %3, %6, %8, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n\t"
        "v_pk_mul_f32 %0, %2, %4 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %1, %3, %5 op_sel_hi:[0,1]\n\t"
        "v_pk_fma_f32 %0, %2, %4, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n\t"
        "v_pk_fma_f32 %1, %3, %5, %1 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"
        : "=&v"(y0), "=&v"(y1), "=&v"(m0), "=&v"(m1)
        : "v"(x0), "v"(x1), "v"(base), "s"(r0), "s"(r1));
    x0 = y0, x1 = y1;
    return m1;
}
// The mixer alone in that form, two samples per statement:  x_k = m_k * x_k  (vfo.cpp:241) as one packed multiply and one packed
// FMA each, alternating (the ROBUST arithmetic: table entries m_k from the exact recurrence, everything after them as FMAs).
__device__ __forceinline__ void cmul_fast2(v2f m0, v2f m1, v2f &x0, v2f &x1)
{
    v2f y0, y1;
    asm("v_pk_mul_f32 %0, %2, %4 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %1, %3, %5 op_sel_hi:[0,1]\n\t"
        "v_pk_fma_f32 %0, %2, %4, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n\t"
        "v_pk_fma_f32 %1, %3, %5, %1 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"
        : "=&v"(y0), "=&v"(y1)
        : "v"(m0), "v"(m1), "v"(x0), "v"(x1));
    x0 = y0, x1 = y1;
}
// the 16 entries behind checkpoint `c` and the mixer on the lane's 16 samples
__device__ __forceinline__ void nco_mix_fast16(v2f c, const float2 *__restrict__ rk, v2f *x)
{
    const v2f r0 = {ldc(&rk[0].x), ldc(&rk[0].y)}, r1 = {ldc(&rk[1].x), ldc(&rk[1].y)};
    const v2f r2 = {ldc(&rk[2].x), ldc(&rk[2].y)}, r3 = {ldc(&rk[3].x), ldc(&rk[3].y)};
#pragma unroll
    for (int b = 0; b < kRun; b += 4) {
        nco_mix_fast2(c, r0, r1, x[b], x[b + 1]);
        c = nco_mix_fast2(c, r2, r3, x[b + 2], x[b + 3]);
    }
}

// Replays the whole table once per VFO and keeps every 16th entry: cp[j] = table[16j-1]
// (cp[0] = the initial (1,0)), so any aligned run of 16 entries can be regenerated in
// registers, bit-exact by construction.
__device__ __forceinline__ void nco_fill(float2 *__restrict__ cp, float rot_re, float rot_im, int L)
{
    float2 v = make_float2(1.0f, 0.0f);
    cp[0] = v;
    for (int k = 0; k < L; k += kRun) {
#pragma unroll
        for (int t = 0; t < kRun; ++t)
            v = nco_step(v, rot_re, rot_im);
        cp[(k >> 4) + 1] = v;
    }
}

// ---- kernels: one thread (k_vfo_reset: one workgroup) per job, between frames -----------------------------------------------
// One thread per VFO, at finalize.
__global__ void k_nco_init(const NcoInit *__restrict__ jobs, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const NcoInit J = jobs[i];
    nco_fill(J.cp, J.rot_re, J.rot_im, J.L);
}

// sdrx_set_mixer_freqs / sdrx_set_gains between two frames: one thread per job.  A retune is `delete osc_mix; osc_mix = new
// Oscillator(Fs, f)` (the checkpoints regenerated in place by the same recurrence as k_nco_init, exact in every arithmetic)
// plus the new rotation and the frame the oscillator starts at; a gain job patches one float of a demodulation descriptor.
// The host drained the context first: no launch reads these records while this one runs.
__global__ void k_vfo_retune(const RetuneJob *__restrict__ jobs, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const RetuneJob J = jobs[i];
    if (J.kind == kJobGain) {
        *J.gain = J.value;
        return;
    }
    K1Vfo *v = J.vfo;
    nco_fill(const_cast<float2 *>(v->cp), J.rot_re, J.rot_im, v->L);
    v->rot_re = J.rot_re;
    v->rot_im = J.rot_im;
    for (int t = 0; t < 4; ++t)
        v->rk[t] = J.rk[t];
    v->origin = J.origin;
}

// sdrx_set_active between two frames: one workgroup per job (FillJob, sdrx_dev.h).  The host drained the context first: no
// launch reads these words while this one runs.
__global__ __launch_bounds__(256) void k_vfo_reset(const FillJob *__restrict__ jobs)
{
    const FillJob J = jobs[blockIdx.x];
    for (unsigned i = threadIdx.x; i < J.words; i += 256)
        J.ptr[i] = J.value;
}

// Debug/parity helper: regenerate table[first .. first+count) from the checkpoints.
__global__ void k_nco_dump(const float2 *__restrict__ cp, float rc, float rs, long first, long count,
                           float2 *__restrict__ out)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count)
        return;
    long idx = first + i;
    long j = idx >> 4;
    float2 v = cp[j];
    for (long t = j << 4; t <= idx; ++t)
        v = nco_step(v, rc, rs);
    out[i] = v;
}
