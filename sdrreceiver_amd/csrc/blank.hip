// blank.hip -- the impulse blanker (include/sdrx.h "Impulse blanker"; no counterpart in the reference): k_blank zeroes
// the samples of a cf32 frame whose power exceeds a threshold, and G samples on either side of each, on the way from the ingest
// kernels' staging buffer to what they wrote before (the front stage's input, the resampler's, or the tree's raw frame);
// k_blank_step, one workgroup behind it, takes the next frame's reference bin from the frame's power histogram by rank, leaves the
// carry for the next frame and writes the frame's record.  Every rule is sdrx_blank.h's, restated in sdrreceiver_amd/blank.py.
//
// k_blank: a workgroup of 256 threads per 4096 samples, a wave per tile of 1024, a lane per 16 consecutive samples (8 coalesced
// float4 loads of the tile layout, 8 stores).  p = fl(fl(re re) + fl(im im)) (-ffp-contract=off: v_mul, v_mul, v_add), hit = p > thr.
//   Hit bitmap: 68 64-bit words in LDS for the samples [base - 128, base + 4096 + 128); a lane's 16-bit mask joins its three
//   neighbours' by two shuffles, the halo's 256 samples are read through tile_index (a lane each, one ballot per wave).  Halo
//   positions outside the frame hold no hit -- lookahead stops at the frame's end -- but for ONE virtual hit at -1 - tail_gap in
//   the first workgroup: |m - j| <= G for it is rule 5's second clause.
//   Dilation: thread w < 68 spreads word w with its neighbours by doubling shifts (at most 7 steps of 1 .. 32 for G <= 64): to the
//   right in (w, w + 1), to the left in (w - 1, w).  The bit of sample base - 1 says where a run that crosses the workgroup's
//   start began; at the frame's start it is the previous frame's last blank bit (state).
//   Histogram: a private one per wave in LDS, two 16-bit counters a word (a wave holds 1024 samples); a lane adds a run of equal
//   consecutive bins with one LDS atomic; the non-zero sums of the four go to the state's 2048 counters with integer atomics.
//   hits, blanked, runs: wave sums (DPP scan), one LDS atomic per wave, one global atomic per workgroup and non-zero figure; the
//   last hit: one atomicMax per wave that has one.  Integer atomics throughout: exact in any order.
// Relies on dev_helpers.hip (gldv4, gstv4), ingest.hip (wave_inclusive_scan), tile_unit / tile_index (sdrx_dev.h) and sdrx_blank.h.

struct BlankState { // zeroed but for ref_bin = -1, tail_gap = kBlankNoHit, last_hit = -1 at sdrx_finalize
    int ref_bin;             // the reference of the next frame
    int tail_gap;            // the carry of the next frame
    int last_blank;          // whether the last sample of the previous frame was blanked
    int last_hit;            // of the frame in flight: atomicMax of k_blank, -1 again behind k_blank_step
    unsigned hits, blanked, runs, pad; // of the frame in flight
    unsigned hist[kBlankBins];         // of the frame in flight
};
struct BlankRecord { // sdrx_blanker_record of include/sdrx.h (the layout is asserted in sdrx.hip)
    long long frame;
    unsigned n_complex, measured;
    unsigned thr_bits;
    int ref_bin, next_ref_bin;
    unsigned hits, blanked, runs, carry_in;
    unsigned reserved[5];
};

constexpr int kBlankWords = (kBlankWg + 2 * kBlankHalo) / 64; // 68
constexpr int kBlankHaloWords = kBlankHalo / 64;              // 2

__device__ __forceinline__ float blank_power(float re, float im) { return re * re + im * im; }

__global__ __launch_bounds__(kBlankThreads) void k_blank(const float4 *__restrict__ in, float4 *__restrict__ out, int n, float ratio, float floor,
                                                         int guard, BlankState *__restrict__ S)
{
    __shared__ unsigned long long sh_hit[kBlankWords], sh_blank[kBlankWords];
    __shared__ unsigned sh_hist[kBlankThreads / 64][kBlankBins / 2];
    __shared__ unsigned sh_cnt[2]; // hits | blanked << 16 (a workgroup: 4096 each at most), runs
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = (int)blockIdx.x * kBlankWg, chunk = (int)blockIdx.x * (kBlankThreads / 64) + wave;
    const int s0 = base + tid * kBlankThread; // this lane's first sample
    const bool valid = s0 < n;                // (frames are multiples of 16: all of a lane's samples or none)
    const float thr = blank_threshold(S->ref_bin, ratio, floor);
    const int tail_gap = S->tail_gap;

    for (int i = tid; i < kBlankThreads / 64 * (kBlankBins / 2); i += kBlankThreads)
        (&sh_hist[0][0])[i] = 0u;
    if (tid < 2)
        sh_cnt[tid] = 0u;
    v4f v[8];
    if (valid) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            v[i] = gldv4(in + tile_unit(chunk, i, lane));
    }
    __syncthreads();

    // ---- the lane's own 16 samples: hit mask, bins
    unsigned hit = 0u;
    if (valid) {
        unsigned *h = sh_hist[wave];
        int cur = -1;
        unsigned cnt = 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float p = blank_power(v[i][2 * e], v[i][2 * e + 1]);
                hit |= (p > thr ? 1u : 0u) << (2 * i + e);
                const int b = blank_bin(p);
                if (b == cur) {
                    ++cnt;
                } else {
                    if (cnt)
                        atomicAdd(&h[cur >> 1], cnt << (16 * (cur & 1)));
                    cur = b, cnt = 1u;
                }
            }
        }
        atomicAdd(&h[cur >> 1], cnt << (16 * (cur & 1)));
    }
    {
        const unsigned h32 = hit | ((unsigned)__shfl_down(hit, 1) << 16);                                   // (even lanes)
        const unsigned long long h64 = (unsigned long long)h32 | ((unsigned long long)__shfl_down(h32, 2) << 32); // (lanes 0, 4, ..)
        if ((lane & 3) == 0)
            sh_hit[kBlankHaloWords + (tid >> 2)] = h64;
    }
    {
        // the halo: waves 0, 1 the 128 samples in front of the workgroup, waves 2, 3 the 128 behind it
        const int g = (wave < 2 ? base - kBlankHalo + 64 * wave : base + kBlankWg + 64 * (wave - 2)) + lane;
        bool hh = false;
        if (g >= 0 && g < n) {
            const float2 x = reinterpret_cast<const float2 *>(in)[tile_index<size_t>(g)];
            hh = blank_power(x.x, x.y) > thr;
        }
        if (g < 0 && g == -1 - tail_gap) // (the first workgroup only)
            hh = true;
        const unsigned long long m = __ballot(hh);
        if (lane == 0)
            sh_hit[wave < 2 ? wave : kBlankWords - 4 + wave] = m;
    }
    __syncthreads();

    // ---- dilation by +-guard, a word per thread
    if (tid < kBlankWords) {
        const unsigned long long mid = sh_hit[tid];
        unsigned long long am = mid, ah = tid + 1 < kBlankWords ? sh_hit[tid + 1] : 0ull; // looks right: bit p |= bit p + k
        unsigned long long bm = mid, bl = tid > 0 ? sh_hit[tid - 1] : 0ull;               // looks left:  bit p |= bit p - k
        for (int c = 0; c < guard;) {
            const int s = min(c + 1, guard - c); // 1 .. 32
            am |= (am >> s) | (ah << (64 - s));
            ah |= ah >> s;
            bm |= (bm << s) | (bl >> (64 - s));
            bl |= bl << s;
            c += s;
        }
        sh_blank[tid] = am | bm;
    }
    // ---- the waves' histograms -> the state's, non-zero bins only (every LDS atomic is in front of the barrier above)
    for (int w = tid; w < kBlankBins / 2; w += kBlankThreads) {
        unsigned lo = 0u, hi = 0u;
#pragma unroll
        for (int k = 0; k < kBlankThreads / 64; ++k) {
            const unsigned x = sh_hist[k][w];
            lo += x & 0xffffu, hi += x >> 16;
        }
        if (lo)
            atomicAdd(&S->hist[2 * w], lo);
        if (hi)
            atomicAdd(&S->hist[2 * w + 1], hi);
    }
    __syncthreads();

    // ---- the lane's blank mask; write; count
    unsigned blank = 0u, prev = 0u;
    if (valid) {
        const unsigned long long w = sh_blank[kBlankHaloWords + (tid >> 2)];
        const int sh = 16 * (tid & 3);
        blank = (unsigned)(w >> sh) & 0xffffu;
        prev = sh ? (unsigned)(w >> (sh - 1)) & 1u : (unsigned)(sh_blank[kBlankHaloWords + (tid >> 2) - 1] >> 63);
        if (s0 == 0)
            prev = (unsigned)S->last_blank;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v4f y = v[i];
            if (blank & (1u << (2 * i)))
                y[0] = 0.0f, y[1] = 0.0f;
            if (blank & (2u << (2 * i)))
                y[2] = 0.0f, y[3] = 0.0f;
            gstv4(out + tile_unit(chunk, i, lane), y);
        }
    }
    const int n_run = __popc(blank & ~((blank << 1) | prev) & 0xffffu);
    const int hb = wave_inclusive_scan(__popc(hit) | (__popc(blank) << 16)), rr = wave_inclusive_scan(n_run);
    int last = hit ? s0 + 31 - __clz((int)hit) : -1;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
        last = max(last, __shfl_xor(last, d));
    if (lane == 63) {
        if (hb)
            atomicAdd(&sh_cnt[0], (unsigned)hb);
        if (rr)
            atomicAdd(&sh_cnt[1], (unsigned)rr);
        if (last >= 0)
            atomicMax(&S->last_hit, last);
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned c0 = sh_cnt[0], c1 = sh_cnt[1];
        if (c0 & 0xffffu)
            atomicAdd(&S->hits, c0 & 0xffffu);
        if (c0 >> 16)
            atomicAdd(&S->blanked, c0 >> 16);
        if (c1)
            atomicAdd(&S->runs, c1);
    }
}

// One workgroup behind k_blank of the same frame: the rank scan over the frame's histogram (8 bins a thread, a DPP scan per wave,
// the waves' totals through LDS), the record, the state of the next frame, and the histogram and the counters cleared for it.
__global__ __launch_bounds__(kBlankThreads) void k_blank_step(BlankState *__restrict__ S, BlankRecord *__restrict__ rec, long long frame, int n, int rank_q16,
                                                              int guard, float ratio, float floor)
{
    constexpr int kPer = kBlankBins / kBlankThreads; // 8
    __shared__ unsigned sh_tot[kBlankThreads / 64];
    __shared__ int sh_next;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned c[kPer], s = 0u;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        c[i] = S->hist[kPer * tid + i];
        s += c[i];
    }
    const unsigned incl = (unsigned)wave_inclusive_scan((int)s);
    if (lane == 63)
        sh_tot[wave] = incl;
    if (tid == 0)
        sh_next = kBlankMaxBin;
    __syncthreads();
    unsigned before = 0u;
    for (int k = 0; k < wave; ++k)
        before += sh_tot[k];
    unsigned long long cum = (unsigned long long)before + incl - s; // the bins in front of this thread's
    if (!blank_rank_reached(cum, (unsigned)n, (unsigned)rank_q16) && blank_rank_reached(cum + s, (unsigned)n, (unsigned)rank_q16)) {
        int b = kPer * tid;
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            cum += c[i];
            if (blank_rank_reached(cum, (unsigned)n, (unsigned)rank_q16))
                break;
            ++b;
        }
        sh_next = min(b, kBlankMaxBin); // (one thread: the cumulative count only grows)
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i)
        S->hist[kPer * tid + i] = 0u;
    __syncthreads();
    if (tid == 0) {
        const int ref = S->ref_bin, gap_in = S->tail_gap, gap_out = blank_tail_gap(n, S->last_hit);
        const int carry = blank_carry_in(n, guard, gap_in);
        BlankRecord r;
        r.frame = frame;
        r.n_complex = (unsigned)n;
        r.measured = 1u;
        r.thr_bits = blank_float_bits(blank_threshold(ref, ratio, floor));
        r.ref_bin = ref;
        r.next_ref_bin = sh_next;
        r.hits = S->hits, r.blanked = S->blanked, r.runs = S->runs;
        r.carry_in = (unsigned)carry;
#pragma unroll
        for (int i = 0; i < 5; ++i)
            r.reserved[i] = 0u;
        *rec = r;
        S->ref_bin = sh_next;
        S->tail_gap = gap_out;
        S->last_blank = gap_out <= guard || carry == n ? 1 : 0;
        S->last_hit = -1;
        S->hits = 0u, S->blanked = 0u, S->runs = 0u;
    }
}
