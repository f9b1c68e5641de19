// agc.hip -- option "agc": the per-leaf gain step behind a frame's gate (included from sdrx.hip, launched by its frame sequence
// wherever squelch_gate is).  One launch on the stream that completed the frame's meter records:
//
//   k_agc_step   one thread per USB leaf.  Folds the leaf's meter records of frame f (what sdrx_get_meters folds on the host:
//                16-byte loads, integers, independent of any order), applies the rule of include/sdrx.h to the gain frame f ran
//                with -- the float the demodulation reads, K2Vfo::gain or K4Vfo::gain -- and stores the gain of frame f + 1 there
//                with a plain vector store: the demodulation reads it through the constant address space in a LATER launch
//                (what k_vfo_retune relies on).  One fp32 multiply and two min / max per step; everything else in integers.
//                Writes one record {gain_used, gain_next, action, quiet_run} per leaf into frame f's parity of d_pay, in the
//                fixed-size part behind the meter records.
//   k_agc_set    sdrx_set_agc's job kernel: settings of the named leaves, quiet_run = 0.
//
// No atomics, no LDS, no inter-workgroup protocol.  Everything a thread loads is its own leaf's (per-lane addresses: vector
// loads; only the array bases and n are wave-uniform, and they are kernel arguments -- SGPRs already).
//
// Option "park": the PARK form reads the leaf's K2Vfo flag word (ParkArg, sdrx_dev.h).  A parked frame is no observation: the
// leaf's records are stale (nothing wrote them) and are not read into the decision; gain and quiet_run stay.
#pragma once

namespace sdrx {

constexpr int kAgcThreads = 256;

struct AgcLeaf { // static, per USB leaf (slot order = node order); 32 bytes = two 16-byte loads (the last two words are padding
                 // that keeps the stride a multiple of 16: the second load fetches them and nobody reads them)
    float *gain;                 // the float frame f's demodulation read: K2Vfo::gain, or K4Vfo::gain behind a long low-pass.
                                 //   For such a leaf ONLY K4Vfo::gain is stepped: its K2Vfo::gain (which sdrx_set_gains also
                                 //   writes) goes stale, and nothing reads it -- k_usb_demod hands usb_out on before the gain
                                 //   is applied.  Whoever reads K2Vfo::gain of a long-low-pass leaf one day must step it here too.
    unsigned meter_off, meter_n; // its MeterAcc records: byte offset into d_pay[p] (a multiple of 16), count
    unsigned n_values;           // payload values per frame (n_out)
    unsigned act_word;           // option park: its flag word in Park::d_act
    unsigned pad[2];
};
struct AgcCfg { // sdrx_agc_cfg as the device keeps it
    unsigned lo_ms, hi_ms, silent_ms, hold_frames;
    float up, down, gain_min, gain_max;
};
struct AgcRecord { // per leaf and frame
    float gain_used, gain_next;
    int action;
    unsigned quiet_run;
};
struct AgcJob { // sdrx_set_agc: leaf `index` (slot) gets `cfg`, its quiet_run restarts at 0
    AgcCfg cfg;
    unsigned index, pad[3];
};
static_assert(sizeof(AgcLeaf) == 32 && sizeof(AgcCfg) == 32 && sizeof(AgcRecord) == 16 && sizeof(AgcJob) == 48, "agc: record sizes");

__global__ __launch_bounds__(64) void k_agc_set(const AgcJob *__restrict__ jobs, int n, AgcCfg *__restrict__ cfg, unsigned *__restrict__ quiet)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= n)
        return;
    const AgcJob J = jobs[j];
    cfg[J.index] = J.cfg;
    quiet[J.index] = 0;
}

// rec: AgcRecord[n] inside d_pay[p] (p = the frame's parity), pay = d_pay[p].  Both point into ONE allocation and both are
// __restrict__: the kernel reads only [meter_off, rec_off) through `pay` -- the meter records -- and writes only the records
// behind them through `rec` (sdrx_ctx::Agc::rec_off), so the regions never overlap.
template <bool PARK = false>
__global__ __launch_bounds__(kAgcThreads) void k_agc_step(const AgcLeaf *__restrict__ leaves, const AgcCfg *__restrict__ cfg, unsigned *__restrict__ quiet,
                                                          const unsigned char *__restrict__ pay, AgcRecord *__restrict__ rec, int n, ParkArg<PARK> K)
{
    const int i = blockIdx.x * kAgcThreads + threadIdx.x;
    if (i >= n)
        return;
    const uint4 *lp = reinterpret_cast<const uint4 *>(leaves + i), *cp = reinterpret_cast<const uint4 *>(cfg + i);
    const uint4 l0 = lp[0], l1 = lp[1], c0 = cp[0], c1 = cp[1]; // (asked for together: no dependent step between them)
    float *gp = reinterpret_cast<float *>(((unsigned long long)l0.y << 32) | l0.x);
    const unsigned meter_off = l0.z, meter_n = l0.w, nv = l1.x;
    bool parked = false;
    if constexpr (PARK)
        parked = K.act[l1.y] == 0;
    unsigned q = quiet[i];
    const float g = *gp;
    const unsigned lo_ms = c0.x, hi_ms = c0.y, silent_ms = c0.z, hold = c0.w;
    const float up = __uint_as_float(c1.x), down = __uint_as_float(c1.y), gmin = __uint_as_float(c1.z), gmax = __uint_as_float(c1.w);
    float g2 = g;
    int action = 0;
    if (!parked && nv != 0 && hi_ms != 0) {
        unsigned long long s = 0;
        unsigned clipped = 0;
        const uint4 *mr = reinterpret_cast<const uint4 *>(pay + meter_off);
        for (unsigned j = 0; j < meter_n; ++j) { // {sum_sq u64, clipped u32, peak u32}
            const uint4 r = mr[j];
            s += ((unsigned long long)r.y << 32) | r.x;
            clipped += r.z;
        }
        const unsigned long long nn = nv;
        const bool hot = clipped > 0 || s > (unsigned long long)hi_ms * nn;
        const bool silent = !hot && s < (unsigned long long)silent_ms * nn;
        const bool cold = !hot && !silent && s < (unsigned long long)lo_ms * nn;
        if (hot) {
            g2 = fminf(fmaxf(__fmul_rn(g, down), gmin), gmax);
            q = 0;
            action = -1;
        } else if (silent) {
        } else if (cold) {
            q = q == 0xffffffffu ? q : q + 1;
            if (q > hold) {
                g2 = fminf(fmaxf(__fmul_rn(g, up), gmin), gmax);
                action = 1;
            }
        } else {
            q = 0;
        }
        quiet[i] = q;
        if (action != 0)
            *gp = g2;
    }
    AgcRecord R;
    R.gain_used = g;
    R.gain_next = g2;
    R.action = action;
    R.quiet_run = q;
    *reinterpret_cast<uint4 *>(rec + i) = make_uint4(__float_as_uint(R.gain_used), __float_as_uint(R.gain_next), (unsigned)R.action, R.quiet_run);
}
} // namespace sdrx
