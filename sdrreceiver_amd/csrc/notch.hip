// notch.hip -- the spur canceller in front of the frequency shift (include/sdrx.h "Spur canceller"): up to eight
// narrow steady carriers that are not signals, each tracked as a complex amplitude times the shift's table oscillator and
// subtracted from the tree's raw frame in place.  k_notch_corr correlates every block of 4096 samples with every tone's
// oscillator; k_notch_step, one thread per tone, runs the amplitude loop over the frame's blocks, re-estimates the tone's
// frequency from how the block estimates rotate, writes the record and advances the state; k_notch_apply subtracts every tone
// with the amplitude the loop held in front of each block; k_notch_load, one thread, changes the tone list between two frames.
// Every rule is sdrx_notch.h's, restated in sdrreceiver_amd/notch.py.
//
// k_notch_corr and k_notch_apply: k_shift's geometry -- a workgroup of 256 threads per block of 4096 samples, a wave per tile of
// 1024, a lane per 16 consecutive samples (8 coalesced float4 loads of the tile layout, once for all tones; k_notch_apply: 8
// stores to the same units).  The tables go into LDS as in k_shift.  The tones run in a loop over the registers.  A lane behind
// the frame's end loads and stores nothing and carries +0 into the sums.  -ffp-contract=off: every product and sum is its own
// instruction.
//   Sums of k_notch_corr: a lane adds its 16 terms in ascending order from +0; the wave combines by __shfl_down at distance 1, 2,
//   .., 32 in every lane -- lane 0's chain of partners is the fixed tree of sdrx_notch.h (notch_wave_sum) --; lane 0 of each wave
//   leaves its sum in LDS and thread k combines the four as fl(fl(w0 + w1) + fl(w2 + w3)).
// k_notch_step reads a tone's state, k_notch_apply what the step left as phase_used / inc_used: the step has moved the state on.
// Relies on dev_helpers.hip (gldv4, gstv4), tile_unit (sdrx_dev.h), sdrx_shift.h and sdrx_notch.h.

__device__ __forceinline__ void notch_tables_to_lds(ShiftC *sh_tab, const float2 *__restrict__ tab, int tid)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float2 t = tab[k * kShTab + tid];
        sh_tab[k * kShTab + tid] = ShiftC{t.x, t.y};
    }
}

__global__ __launch_bounds__(kNtThreads) void k_notch_corr(const float4 *__restrict__ buf, int n, int K, const NotchTone *__restrict__ S,
                                                           const float2 *__restrict__ tab, ShiftC *__restrict__ cc)
{
    __shared__ ShiftC sh_tab[3 * kShTab];
    __shared__ ShiftC sh_w[kNtThreads / 64][kNtMax];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    notch_tables_to_lds(sh_tab, tab, tid);
    __syncthreads();
    const int chunk = (int)blockIdx.x * (kNtThreads / 64) + wave;
    const int s0 = (int)blockIdx.x * kNtBlock + tid * kNtLane; // this lane's first sample
    const bool live = s0 < n;                                  // (frames are multiples of 16: all of a lane's samples or none)
    const ShiftC *A = sh_tab, *B = sh_tab + kShTab, *C = sh_tab + 2 * kShTab;
    v4f v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
        v[i] = live ? gldv4(buf + tile_unit(chunk, i, lane)) : v4f{0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < K; ++k) {
        const unsigned inc = S[k].inc;
        unsigned p = S[k].phase + (unsigned)s0 * inc;
        float sr = 0.0f, si = 0.0f;
        if (live) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const ShiftC t = notch_corr_term(ShiftC{v[i][2 * e], v[i][2 * e + 1]}, shift_rot(A, B, C, p));
                    sr = sr + t.re;
                    si = si + t.im;
                    p += inc;
                }
            }
        }
#pragma unroll
        for (int s = 1; s < 64; s *= 2) {
            sr = sr + __shfl_down(sr, s);
            si = si + __shfl_down(si, s);
        }
        if (lane == 0)
            sh_w[wave][k] = ShiftC{sr, si};
    }
    __syncthreads();
    if (tid < K)
        cc[(int)blockIdx.x * kNtMax + tid] = ShiftC{notch_wg_sum(sh_w[0][tid].re, sh_w[1][tid].re, sh_w[2][tid].re, sh_w[3][tid].re),
                                                   notch_wg_sum(sh_w[0][tid].im, sh_w[1][tid].im, sh_w[2][tid].im, sh_w[3][tid].im)};
}

// One workgroup behind k_notch_corr of the same frame: thread k < K runs its tone over the frame's blocks (sdrx_notch.h,
// notch_step_tone), writes used[b][k] and its part of the record and moves its slot's state on; the others clear theirs.
__global__ __launch_bounds__(64) void k_notch_step(NotchTone *__restrict__ S, const ShiftC *__restrict__ cc, ShiftC *__restrict__ used,
                                                   NotchRecord *__restrict__ rec, long long frame, int n, int K, float mu, float afc_gain,
                                                   float min_coherence, unsigned max_pull)
{
    const int k = threadIdx.x;
    if (blockIdx.x != 0 || k >= kNtMax)
        return;
    NotchToneRecord R;
    if (k < K) {
        NotchTone T = S[k];
        notch_step_tone(cc + k, used + k, n, T, mu, afc_gain, min_coherence, max_pull, R);
        S[k] = T;
    } else {
        R.inc = R.inc_next = R.a_re_bits = R.a_im_bits = R.coherent = R.adapted = R.clamped = R.rejected = 0u;
        R.s_re = R.s_im = R.p = R.e = 0.0;
    }
    rec->tone[k] = R;
    if (k == 0) {
        rec->frame = frame;
        rec->n_complex = (unsigned)n, rec->n_tones = (unsigned)K, rec->blocks = (unsigned)notch_blocks(n);
        rec->reserved[0] = rec->reserved[1] = rec->reserved[2] = 0u;
    }
}

__global__ __launch_bounds__(kNtThreads) void k_notch_apply(float4 *__restrict__ buf, int n, int K, const NotchTone *__restrict__ S,
                                                            const float2 *__restrict__ tab, const ShiftC *__restrict__ used)
{
    __shared__ ShiftC sh_tab[3 * kShTab];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    notch_tables_to_lds(sh_tab, tab, tid);
    __syncthreads();
    const int chunk = (int)blockIdx.x * (kNtThreads / 64) + wave;
    const int s0 = (int)blockIdx.x * kNtBlock + tid * kNtLane;
    if (s0 >= n)
        return;
    const ShiftC *A = sh_tab, *B = sh_tab + kShTab, *C = sh_tab + 2 * kShTab;
    v4f v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
        v[i] = gldv4(buf + tile_unit(chunk, i, lane));
    for (int k = 0; k < K; ++k) {
        const ShiftC u = used[(int)blockIdx.x * kNtMax + k];
        const unsigned inc = S[k].inc_used;
        unsigned p = S[k].phase_used + (unsigned)s0 * inc;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const ShiftC y = notch_subtract(ShiftC{v[i][2 * e], v[i][2 * e + 1]}, u, shift_rot(A, B, C, p));
                v[i][2 * e] = y.re, v[i][2 * e + 1] = y.im;
                p += inc;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const ShiftC y = notch_canonical(ShiftC{v[i][2 * e], v[i][2 * e + 1]});
            v[i][2 * e] = y.re, v[i][2 * e + 1] = y.im;
        }
        gstv4(buf + tile_unit(chunk, i, lane), v[i]);
    }
}

// sdrx_set_notch after sdrx_finalize: the tone list of the next frame, in stream order -- a slot named in `restart` starts at
// (0, inc0, 0), the others keep phase, increment and amplitude
__global__ void k_notch_load(NotchTone *__restrict__ S, NotchLoad a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    for (int k = 0; k < kNtMax; ++k)
        if ((a.restart >> k) & 1u) {
            NotchTone T;
            T.phase = 0u, T.inc = a.inc0[k], T.inc0 = a.inc0[k];
            T.a_re = 0.0f, T.a_im = 0.0f;
            T.phase_used = 0u, T.inc_used = a.inc0[k], T.pad = 0u;
            S[k] = T;
        }
}
