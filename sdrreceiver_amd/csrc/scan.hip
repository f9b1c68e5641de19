// scan.hip -- band scan (include/sdrx.h "Band scan"): the carriers in a watched source's spectrum.  The PSD the
// channel watch has just computed for a source (watch.hip) is integrated over M frames, folded into cells of w bins in
// display order, and every run of cells above ratio x the floor -- the k-th smallest cell -- is reported as a hit: where a
// spare leaf can be tuned to (included from sdrx.hip behind drift.hip, launched behind k_watch_bands beside k_watch_drift).
//
//   ACC[i]  = count == 0 ? PSD[i] : ACC[i] + PSD[i]                       IEEE double, one addition per bin
//   cell[c] = ((a0 + a1) + a2) + ... over display bins c w .. c w + w - 1   the ONE prescribed order; display bin b = natural (b + N/2) mod N
//   floor   = the cell whose 64-bit pattern is the k-th smallest;  thr = fl(floor * (ratio_q8 / 256.0));  hot = cell > thr
// Everything behind the cell sums is a selection, a comparison or an integer/lexicographic scan: any order gives the same bits.
#pragma once

namespace sdrx {

constexpr int kScanMaxHits = 512;                     // SDRX_SCAN_MAX_HITS
constexpr int kScanMaxCellBins = 256;                 // widest cell: C = N / w = 32 cells
constexpr int kScanPerThread = kSpecN / kSpecThreads; // cells a thread owns at w = 1

struct ScanCfg { // = sdrx_scan_cfg (include/sdrx.h)
    int cell_bins, frames, floor_permille;
    unsigned ratio_q8;
    int min_cells;
    int reserved[3];
};
struct ScanHit { // = sdrx_scan_hit
    int first_cell, n_cells, peak_cell, reserved;
    double peak_pwr, reserved_d;
};
struct ScanRecord { // = sdrx_scan_level
    long long frame;
    double floor, thr;
    int n_hits, n_stored, n_hot, integrated, frames, cell_bins, measured, complete;
    int reserved[2];
};

struct ScanState { // what a source keeps on the device from its first sdrx_set_scan on: one allocation that never moves
    double acc[kSpecN];
    double cells[kSpecN];       // of the last completed evaluation: C of them
    ScanHit hits[kScanMaxHits]; // ... its first n_stored hits
    ScanRecord head;            // ... and its record
    unsigned count;             // frames integrated so far (sdrx_set_scan: back to 0)
    unsigned valid;             // 1: an evaluation has completed under the present setting (sdrx_set_scan: back to 0)
};
struct ScanSrc { // one workgroup of k_watch_scan
    const double *psd; // the watch's PSD of the source (WatchSrc::psd)
    ScanState *state;
    ScanCfg cfg;
    int level, slot; // tree level of the stream's VFO, -1: the raw frame; its record
};

// An element of the segmented scan over the cells.  A segment begins at every cell that does not continue a run (f = 1): a
// cold cell, or a hot one behind a cold one.  s: where the segment began; (v, i): its largest cell, the lowest index first.
struct ScanSeg {
    int f, s, i;
    double v;
};
// a then b, a to the left: associative (the segmented-scan operator over max by (value, lowest index))
__device__ __forceinline__ ScanSeg scan_combine(const ScanSeg &a, const ScanSeg &b)
{
    if (b.f)
        return b;
    ScanSeg r = a;
    if (b.v > a.v) { // (equal: a, which lies to the left)
        r.v = b.v;
        r.i = b.i;
    }
    return r;
}
__device__ __forceinline__ ScanSeg scan_shfl_up(const ScanSeg &x, int off)
{
    ScanSeg y;
    y.f = __shfl_up(x.f, off);
    y.s = __shfl_up(x.s, off);
    y.i = __shfl_up(x.i, off);
    y.v = __shfl_up(x.v, off);
    return y;
}

// the record of a measured frame, field by field to where it goes
__device__ __forceinline__ void scan_record(ScanRecord *r, unsigned long long frame, double flr, double thr, int n_hits, int n_hot, int integrated, int M,
                                            int w, int complete)
{
    r->frame = (long long)frame;
    r->floor = flr;
    r->thr = thr;
    r->n_hits = n_hits;
    r->n_stored = n_hits < kScanMaxHits ? n_hits : kScanMaxHits;
    r->n_hot = n_hot;
    r->integrated = integrated;
    r->frames = M;
    r->cell_bins = w;
    r->measured = 1;
    r->complete = complete;
    r->reserved[0] = r->reserved[1] = 0;
}

// One workgroup of kSpecThreads per source with the scan on.  Every frame: ACC += PSD in global memory.  On the M-th frame the
// integrated spectrum also goes into LDS in display order (64 KiB, what k_watch_drift keeps there), and
//   1. one thread per cell adds its w bins left to right; the cells replace the spectrum in LDS (and go to the state);
//   2. eight radix passes over the 64-bit patterns, most significant byte first, each a 256-bin LDS histogram of the cells that
//      still match the prefix and a workgroup scan of the bins, narrow the prefix down to the k-th smallest pattern;
//   3. thread t owns the cells t P .. t P + P - 1 (P = C / 512, at least 1): a segmented scan -- per thread, per wave (shuffles),
//      over the eight waves -- gives every run's end its first cell and its first largest cell; a prefix sum of the hits per
//      thread gives every hit its place in the list.  A thread walks its own P <= 16 cells, never a run.
__global__ __launch_bounds__(kSpecThreads) void k_watch_scan(const ScanSrc *__restrict__ srcs, WatchArgs A, ScanRecord *__restrict__ rec0,
                                                             ScanRecord *__restrict__ rec1)
{
    __shared__ double X[kSpecN];
    __shared__ unsigned hist[256];
    __shared__ unsigned wave_sum[kSpecThreads / 64];
    __shared__ int wave_f[kSpecThreads / 64], wave_s[kSpecThreads / 64], wave_i[kSpecThreads / 64]; // the waves' ScanSeg, field by field
    __shared__ double wave_v[kSpecThreads / 64];
    __shared__ unsigned long long sel_prefix;
    __shared__ unsigned sel_rank;
    const ScanSrc &D = srcs[blockIdx.x];
    ScanState *st = D.state;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = D.cfg.cell_bins, M = D.cfg.frames, C = kSpecN / w;
    const unsigned count = st->count; // (every thread reads it before thread 0 writes it: the barrier below)
    const bool complete = count + 1u >= (unsigned)M;
    const unsigned long long frame = D.level < 0 ? A.frame_raw : spec_level_frame(A.frame_level, D.level);
    ScanRecord *rec = (frame & 1ull ? rec1 : rec0) + D.slot;
    const double *psd = D.psd;
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k) {
        const int i = tid + k * kSpecThreads;
        const double a = count == 0u ? psd[i] : st->acc[i] + psd[i];
        st->acc[i] = a;
        if (complete)
            X[(i + kSpecN / 2) & (kSpecN - 1)] = a;
    }
    __syncthreads();
    if (!complete) {
        if (tid == 0) {
            scan_record(rec, frame, 0.0, 0.0, 0, 0, (int)(count + 1u), M, w, 0);
            st->count = count + 1u;
        }
        return;
    }
    // 1. the cells: cell c = tid + k * 512, left to right over its w bins; into registers first -- cell c's place in X is
    //    another cell's bin
    double cell[kScanPerThread];
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k) {
        const int c = tid + k * kSpecThreads;
        double sum = 0.0;
        if (c < C) {
            const double *x = X + (size_t)c * w;
            sum = x[0];
            for (int j = 1; j < w; ++j)
                sum += x[j];
        }
        cell[k] = sum;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k) {
        const int c = tid + k * kSpecThreads;
        if (c < C) {
            X[c] = cell[k];
            st->cells[c] = cell[k];
        }
    }
    if (tid == 0) {
        sel_prefix = 0ull;
        sel_rank = (unsigned)(((long long)D.cfg.floor_permille * (C - 1)) / 1000);
    }
    // 2. the k-th smallest pattern
    for (int pass = 0; pass < 8; ++pass) {
        if (tid < 256)
            hist[tid] = 0u;
        __syncthreads(); // (also: X and sel_* of the step before are written)
        const unsigned long long prefix = sel_prefix;
        const unsigned rank = sel_rank;
        const int shift = 56 - 8 * pass;
#pragma unroll
        for (int k = 0; k < kScanPerThread; ++k) {
            const int c = tid + k * kSpecThreads;
            if (c < C) {
                const unsigned long long p = (unsigned long long)__double_as_longlong(cell[k]);
                if (pass == 0 || (p >> (shift + 8)) == prefix)
                    atomicAdd(&hist[(unsigned)(p >> shift) & 255u], 1u);
            }
        }
        __syncthreads();
        // inclusive prefix sum of the 256 bins by the first four waves; the bin that holds rank `rank` extends the prefix
        const unsigned h = tid < 256 ? hist[tid] : 0u;
        unsigned incl = h;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned y = __shfl_up(incl, off);
            if (lane >= off)
                incl += y;
        }
        if (lane == 63)
            wave_sum[wave] = incl;
        __syncthreads();
        for (int v = 0; v < wave; ++v)
            incl += wave_sum[v];
        __syncthreads(); // (every thread has read sel_* and wave_sum)
        if (tid < 256 && incl - h <= rank && rank < incl) { // exactly one bin: the matching cells number more than rank
            sel_prefix = (prefix << 8) | (unsigned long long)tid;
            sel_rank = rank - (incl - h);
        }
    }
    __syncthreads();
    const double flr = __longlong_as_double((long long)sel_prefix);
    const double thr = flr * ((double)D.cfg.ratio_q8 / 256.0);
    // 3. the runs.  Thread t owns the cells t P .. t P + P - 1; a thread behind the last cell owns none.
    const int P = C >= kSpecThreads ? C / kSpecThreads : 1;
    const int c0 = tid * P, n_own = c0 < C ? P : 0;
    const int min_cells = D.cfg.min_cells;
    auto element = [&](int c) {
        ScanSeg e;
        const double v = X[c];
        const bool hot = v > thr;
        e.f = !(hot && c > 0 && X[c - 1] > thr);
        e.s = c;
        e.i = c;
        e.v = hot ? v : -__builtin_huge_val();
        return e;
    };
    ScanSeg own; // the identity: nothing to its left
    own.f = 0;
    own.s = -1;
    own.i = 0x7fffffff;
    own.v = -__builtin_huge_val();
    const ScanSeg identity = own;
    for (int j = 0; j < n_own; ++j)
        own = scan_combine(own, element(c0 + j));
    ScanSeg incl = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const ScanSeg y = scan_shfl_up(incl, off);
        if (lane >= off)
            incl = scan_combine(y, incl);
    }
    if (lane == 63) {
        wave_f[wave] = incl.f;
        wave_s[wave] = incl.s;
        wave_i[wave] = incl.i;
        wave_v[wave] = incl.v;
    }
    ScanSeg carry = scan_shfl_up(incl, 1); // what lies to the left of this thread's cells
    if (lane == 0)
        carry = identity;
    __syncthreads();
    {
        ScanSeg left = identity;
        for (int v = 0; v < wave; ++v) {
            ScanSeg ws;
            ws.f = wave_f[v];
            ws.s = wave_s[v];
            ws.i = wave_i[v];
            ws.v = wave_v[v];
            left = scan_combine(left, ws);
        }
        carry = scan_combine(left, carry);
    }
    // the hits that end in this thread's cells, and its hot cells: both counts in one word (hits <= 4096 in the low half)
    unsigned mine = 0u;
    {
        ScanSeg run = carry;
        for (int j = 0; j < n_own; ++j) {
            const int c = c0 + j;
            run = scan_combine(run, element(c));
            if (X[c] > thr) {
                mine += 1u << 16;
                if ((c == C - 1 || !(X[c + 1] > thr)) && c - run.s + 1 >= min_cells)
                    mine += 1u;
            }
        }
    }
    unsigned before = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned y = __shfl_up(before, off);
        if (lane >= off)
            before += y;
    }
    if (lane == 63)
        wave_sum[wave] = before; // (its readers of step 2 are behind a barrier)
    __syncthreads();
    unsigned total = 0u;
    for (int v = 0; v < kSpecThreads / 64; ++v) {
        if (v == wave)
            before += total;
        total += wave_sum[v];
    }
    before -= mine; // exclusive
    {
        int at = (int)(before & 0xffffu);
        ScanSeg run = carry;
        for (int j = 0; j < n_own; ++j) {
            const int c = c0 + j;
            run = scan_combine(run, element(c));
            if (X[c] > thr && (c == C - 1 || !(X[c + 1] > thr)) && c - run.s + 1 >= min_cells) {
                if (at < kScanMaxHits) { // (field by field: no copy of the struct on the stack)
                    ScanHit *hit = st->hits + at;
                    hit->first_cell = run.s;
                    hit->n_cells = c - run.s + 1;
                    hit->peak_cell = run.i;
                    hit->reserved = 0;
                    hit->peak_pwr = run.v;
                    hit->reserved_d = 0.0;
                }
                ++at;
            }
        }
    }
    if (tid == 0) {
        const int n_hits = (int)(total & 0xffffu), n_hot = (int)(total >> 16);
        scan_record(rec, frame, flr, thr, n_hits, n_hot, M, M, w, 1);
        scan_record(&st->head, frame, flr, thr, n_hits, n_hot, M, M, w, 1);
        st->count = 0u;
        st->valid = 1u;
    }
}

} // namespace sdrx
