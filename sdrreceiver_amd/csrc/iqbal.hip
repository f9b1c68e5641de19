// iqbal.hip -- the IQ balance correction (include/sdrx.h "IQ balance"; no counterpart in the reference): k_iqbal
// applies the current pair (c, d) to a cf32 frame in place -- I' = I, Q' = fl(fl(c I) + fl(d Q)) -- where the ingest kernels left
// it, and sums what it produced; k_iqbal_step, one workgroup behind it, moves the pair for the next frame from those sums, clears
// them and writes the frame's record.  Every rule is sdrx_iqbal.h's, restated in sdrreceiver_amd/iqbal.py.
//
// k_iqbal: a workgroup of 256 threads per 4096 samples, a wave per tile of 1024, a lane per 16 consecutive samples (8 coalesced
// float4 loads of the tile layout, 8 stores to the same units).  A thread behind the frame's end loads and stores nothing and
// carries zeros, so tile padding is in no sum.  -ffp-contract=off: v_mul, v_mul, v_add.
//   Sums: q(I'), q(Q') are integers of at most 15 bits and a sign.  A thread's S_i, S_q stay below 2^19; its S_ii, S_qq, S_iq reach
//   16 * 32767^2 < 2^34 and are 64 bits wide from the first sample.  Wave: the DPP scans of adcmeter.hip (adc_wave_sum for the
//   plain sums, adc_wave_sum64 -- two scans of parts that fit 32 bits -- for the three of products).  Workgroup: the four waves'
//   totals meet in LDS; thread k < 5 adds total k, if it is not zero, to the state's accumulator k with one 64-bit integer
//   atomic.  Plain integer sums: exact in any order.
// Relies on dev_helpers.hip (gldv4, gstv4), adcmeter.hip (adc_wave_sum, adc_wave_sum64), tile_unit (sdrx_dev.h) and sdrx_iqbal.h.

struct IqState { // c = c0, d = d0 and zeros at sdrx_finalize
    float c, d;                 // the pair of the next frame
    unsigned pad[2];
    unsigned long long acc[5];  // of the frame in flight: S_i, S_q, S_iq (two's complement), S_ii, S_qq; zero again behind k_iqbal_step
    unsigned long long pad2;
};
struct IqRecord { // sdrx_iq_record of include/sdrx.h (the layout is asserted in sdrx.hip)
    long long frame;
    unsigned n_complex, measured;
    unsigned adapted, rejected;
    unsigned c_bits, d_bits;
    unsigned next_c_bits, next_d_bits;
    long long sum_i, sum_q, sum_iq;
    unsigned long long sum_ii, sum_qq;
    unsigned reserved[4];
};

__global__ __launch_bounds__(kIqThreads) void k_iqbal(float4 *__restrict__ buf, int n, IqState *__restrict__ S)
{
    __shared__ long long sh_sum[kIqThreads / 64][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = (int)blockIdx.x * (kIqThreads / 64) + wave;
    const int s0 = (int)blockIdx.x * kIqWg + tid * kIqThread; // this lane's first sample
    const bool valid = s0 < n;                                 // (frames are multiples of 16: all of a lane's samples or none)
    const float c = S->c, d = S->d;

    int si = 0, sq = 0;
    long long sii = 0, sqq = 0, siq = 0;
    if (valid) {
        v4f v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            v[i] = gldv4(buf + tile_unit(chunk, i, lane));
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v4f y = v[i];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float I = y[2 * e];
                const float a = c * I, b = d * y[2 * e + 1];
                const float s = a + b;
                const float Q = s == s ? s : iq_bits_float(kIqNanBits); // (one NaN whatever produced it: the model's bits)
                y[2 * e + 1] = Q;
                const int qi = iq_q(I), qq = iq_q(Q);
                si += qi, sq += qq;
                sii += (long long)(qi * qi); // |q| <= 32767: a product fits 32 bits, the sum of four does not
                sqq += (long long)(qq * qq);
                siq += (long long)(qi * qq);
            }
            gstv4(buf + tile_unit(chunk, i, lane), y);
        }
    }
    const long long w[5] = {(long long)adc_wave_sum(si), (long long)adc_wave_sum(sq), adc_wave_sum64(siq), adc_wave_sum64(sii), adc_wave_sum64(sqq)};
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            sh_sum[wave][k] = w[k];
    }
    __syncthreads();
    if (tid < 5) {
        long long t = 0;
#pragma unroll
        for (int k = 0; k < kIqThreads / 64; ++k)
            t += sh_sum[k][tid];
        if (t)
            atomicAdd(&S->acc[tid], (unsigned long long)t);
    }
}

// Bench calibration (sdrx_set_iq_balance with SDRX_IQ_LOAD after sdrx_finalize): the pair of the next frame, in stream order
__global__ void k_iqbal_load(IqState *__restrict__ S, float c, float d)
{
    if (threadIdx.x == 0 && blockIdx.x == 0)
        S->c = c, S->d = d;
}

// One workgroup behind k_iqbal of the same frame; one thread does rule 4, writes the record and the pair of the next frame and
// clears the accumulators for it.
__global__ __launch_bounds__(64) void k_iqbal_step(IqState *__restrict__ S, IqRecord *__restrict__ rec, long long frame, int n, float mu, float min_power)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    IqSums s;
    s.s_i = (long long)S->acc[0], s.s_q = (long long)S->acc[1], s.s_iq = (long long)S->acc[2];
    s.s_ii = S->acc[3], s.s_qq = S->acc[4];
    const float c = S->c, d = S->d;
    const IqStep st = iq_step(s, (unsigned)n, mu, min_power, c, d);
    IqRecord r;
    r.frame = frame;
    r.n_complex = (unsigned)n;
    r.measured = st.measured, r.adapted = st.adapted, r.rejected = st.rejected;
    r.c_bits = iq_float_bits(c), r.d_bits = iq_float_bits(d);
    r.next_c_bits = iq_float_bits(st.c_next), r.next_d_bits = iq_float_bits(st.d_next);
    r.sum_i = s.s_i, r.sum_q = s.s_q, r.sum_iq = s.s_iq;
    r.sum_ii = s.s_ii, r.sum_qq = s.s_qq;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        r.reserved[i] = 0u;
    *rec = r;
    S->c = st.c_next, S->d = st.d_next;
#pragma unroll
    for (int k = 0; k < 5; ++k)
        S->acc[k] = 0ull;
}
