// shift.hip -- the frequency shift at the end of the ingest chain (include/sdrx.h "Frequency shift"; the reference's
// mix_offset, README "tune ALL VFO's up or down", done once on the wideband frame instead of once per VFO): k_shift multiplies the
// tree's raw frame in place by exp(+j 2 pi p / 2^32), p = phase + j inc, from three 256-entry tables; k_shift_step, one thread
// behind it, writes the frame's record and advances the phase; k_shift_load, one thread, changes inc (and phase) between two
// frames.  Every rule is sdrx_shift.h's, restated in sdrreceiver_amd/shift.py.
//
// k_shift: k_iqbal's geometry -- a workgroup of 256 threads per 4096 samples, a wave per tile of 1024, a lane per 16 consecutive
// samples (8 coalesced float4 loads of the tile layout, 8 stores to the same units).  A thread behind the frame's end loads and
// stores nothing.  -ffp-contract=off: every product and every sum is its own instruction.
//   Phase: a lane starts at phase + s0 inc (a wrapping 32-bit multiply) and adds inc per sample; the rotation of every sample is
//   looked up from its own phase, never carried from its neighbour's, so the result does not depend on the geometry.
//   Tables: A | B | C, 768 cf32 = 6 KiB, copied from the one device copy into LDS by every workgroup (3 coalesced float2 loads a
//   thread), entries interleaved (re, im): a gather is one ds_read_b64.  Its banks are (a / 4) mod 64 per 32-lane half, an entry
//   takes two, so 32 consecutive entries are conflict-free and equal addresses broadcast.  Lanes are 16 inc apart in phase: for a
//   correction of a few Hz to a few kHz all lanes of a half read one A entry and one or neighbouring B entries; C's index moves
//   with (16 inc) >> 8 per lane, which no fixed layout serves for every inc -- gcd(stride, 32) lanes share a bank at worst.
// Relies on dev_helpers.hip (gldv4, gstv4), tile_unit (sdrx_dev.h) and sdrx_shift.h.

struct ShiftState { // phase0, inc at sdrx_finalize
    unsigned phase, inc; // of the next frame
    unsigned pad[2];
};
struct ShiftRecord { // sdrx_shift_record of include/sdrx.h (the layout is asserted in sdrx.hip)
    long long frame;
    unsigned n_complex, applied;
    unsigned phase, inc;
    unsigned next_phase, next_inc;
    unsigned reserved[8];
};

__global__ __launch_bounds__(kShThreads) void k_shift(float4 *__restrict__ buf, int n, const ShiftState *__restrict__ S, const float2 *__restrict__ tab)
{
    __shared__ ShiftC sh_tab[3 * kShTab];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float2 t = tab[k * kShTab + tid];
        sh_tab[k * kShTab + tid] = ShiftC{t.x, t.y};
    }
    __syncthreads();
    const int chunk = (int)blockIdx.x * (kShThreads / 64) + wave;
    const int s0 = (int)blockIdx.x * kShWg + tid * kShThread; // this lane's first sample
    if (s0 >= n)                                               // (frames are multiples of 16: all of a lane's samples or none)
        return;
    const unsigned inc = S->inc;
    unsigned p = S->phase + (unsigned)s0 * inc;
    const ShiftC *A = sh_tab, *B = sh_tab + kShTab, *C = sh_tab + 2 * kShTab;
    v4f v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
        v[i] = gldv4(buf + tile_unit(chunk, i, lane));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v4f y = v[i];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const ShiftC r = shift_apply(ShiftC{y[2 * e], y[2 * e + 1]}, shift_rot(A, B, C, p));
            y[2 * e] = r.re, y[2 * e + 1] = r.im;
            p += inc;
        }
        gstv4(buf + tile_unit(chunk, i, lane), y);
    }
}

// sdrx_set_shift after sdrx_finalize: the increment of the next frame -- and with SDRX_SHIFT_LOAD_PHASE its phase -- in stream order
__global__ void k_shift_load(ShiftState *__restrict__ S, unsigned inc, unsigned phase0, int load_phase)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        S->inc = inc;
        if (load_phase)
            S->phase = phase0;
    }
}

// One thread behind k_shift of the same frame: the record, and the phase of the next frame.
__global__ __launch_bounds__(64) void k_shift_step(ShiftState *__restrict__ S, ShiftRecord *__restrict__ rec, long long frame, int n)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    const unsigned phase = S->phase, inc = S->inc;
    const unsigned next = shift_advance(phase, (unsigned)n, inc);
    ShiftRecord r;
    r.frame = frame;
    r.n_complex = (unsigned)n, r.applied = 1u;
    r.phase = phase, r.inc = inc;
    r.next_phase = next, r.next_inc = inc;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        r.reserved[i] = 0u;
    *rec = r;
    S->phase = next;
}
