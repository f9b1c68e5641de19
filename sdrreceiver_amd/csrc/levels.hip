// levels.hip -- the launches that carry a whole step: k_mix_levels, the mix items of every tree level in one grid, and
// k_levels_tail, the same with the demodulation blocks of the frame that left the last level.  No arithmetic of their own:
// the reference functions are those of run_item (mix.hip) and demod_block (demod.hip).
// Relies on dev_helpers.hip (ldc), mix.hip (run_item, kK1MinWaves) and demod.hip (demod_block, DemodLds).

// ------------------------------------------------------------------------------------ k_mix_levels
// ONE launch for the mix/decimate items of EVERY tree level, each level working on the frame that has
// reached it: level l on frame k - l (a software pipeline over consecutive frames: the levels of one
// launch are independent of each other).  Why: on BASELINE config 3 the level-0 launch -- 2-3 main VFOs,
// ~770 one-chunk items -- leaves most of the chip idle for its whole duration (6-9 us of a ~110 us
// frame); as part of the same grid its short items run beside the sub VFOs' long ones, without the
// cross-stream events that cost more than they gain on this runtime (profiles/README.md).
// The list is [level 0 items | level 1 items | ...], every part starting at a multiple of 8 entries
// (workgroup i runs on XCD i mod 8: a part keeps its XCD mapping whichever range a launch covers);
// -1 = padding.  One wave per workgroup, exactly as k_mix_decimate.
struct LevelArgs {
    unsigned long long frame_level[kMaxLevels]; // frame each tree level works on in this launch
    const void *raw;                            // level 0's raw frame ...
    int raw_mode;                               // ... and its form (kRaw*)
    int pad_;
};
template <bool EXACT, bool ROT = !EXACT, bool METER = false, bool PARK = false>
__global__ __launch_bounds__(64, kK1MinWaves) void k_mix_levels(const K1Vfo *__restrict__ k1, const K1Work *__restrict__ items,
                                                   const int *__restrict__ item_level, const int *__restrict__ list, LevelArgs A,
                                                   ParkArg<PARK> P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int it = ldc(list + blockIdx.x);
    if (it < 0)
        return;
    const int lv = ldc(item_level + it);
    if constexpr (PARK) // (the item's own level word carries the flag: kParkBit, sdrx_dev.h)
        if (lv & kParkBit)
            return;
    run_item<EXACT, ROT, METER>(k1, K1Work{ldc(&items[it].vfo), ldc(&items[it].s_begin), ldc(&items[it].s_first_out), ldc(&items[it].s_end)},
                    A.frame_level[lv], A.raw, A.raw_mode, lv == 0, smem, (int)threadIdx.x);
}

// ------------------------------------------------------------------------------------ k_levels_tail
// k_mix_levels with the USB demodulation of the frame that left the last level in the PREVIOUS launch inside the same grid
// (option tail_in_levels): one launch per step where k_mix_levels + k_usb_demod were two, and the second launch's ramp and
// tail go.  Nothing in the grid depends on anything else in it: level l works on frame k - l, the demodulation
// on frame k - n_levels, whose leaf streams (parity (k - n_levels) & 1) no item of this launch writes -- the planner fuses only
// trees whose demodulated leaves all sit on the last level (sdrx.hip, build_level_plan).
// Workgroups of 256 threads, each one of two things (TailWg):
//   * four mix items, one per wave, every wave on LDS of its own (lds_wave bytes apart) -- exactly k_mix_levels' item body;
//   * one demodulation block (demod_block, unchanged: same taps, same order, one accumulator per output) on all four waves.
// Every part of the list starts at a multiple of 8 workgroups, and inside a part workgroup 8 b + x takes the items
// 32 b + 8 w + x (w = wave): item j still runs on XCD j mod 8, as it does in k_mix_levels.
struct TailWg {
    int item[4]; // mix items of the four waves (-1: none); item[0] <= -2: demodulation block -2 - item[0] of the BlockWork list
};
struct LevelTailArgs {
    LevelArgs L;
    unsigned long long frame_tail; // frame the demodulation blocks work on
    int active;                    // bit l: tree level l has a frame in this launch; bit kMaxLevels: the demodulation has one
    int lds_wave;                  // LDS bytes of one mix wave
};
template <bool EXACT, bool ROT = !EXACT, bool METER = false, bool PARK = false>
__global__ __launch_bounds__(256, kK1MinWaves) void k_levels_tail(const K1Vfo *__restrict__ k1, const K1Work *__restrict__ items,
                                                                  const int *__restrict__ item_level, const TailWg *__restrict__ wgs,
                                                                  const K2Vfo *__restrict__ k2, const BlockWork *__restrict__ dwork,
                                                                  LevelTailArgs A, ParkArg<PARK> P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int first = ldc(&wgs[blockIdx.x].item[0]);
    if (first <= -2) {
        if (A.active & (1 << kMaxLevels)) {
            const int b = -2 - first;
            if constexpr (PARK)
                if (ldc(P.act + ldc(&dwork[b].vfo)) == 0)
                    return;
            demod_block<EXACT, METER>(k2, BlockWork{ldc(&dwork[b].vfo), ldc(&dwork[b].blk)}, A.frame_tail, *reinterpret_cast<DemodLds *>(smem),
                                      (int)threadIdx.x);
        }
        return;
    }
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int it = ldc(&wgs[blockIdx.x].item[wave]);
    if (it < 0)
        return;
    const int lv = ldc(item_level + it);
    if constexpr (PARK)
        if (lv & kParkBit)
            return;
    if (!((A.active >> lv) & 1)) // (a level without a frame: only while the pipeline drains)
        return;
    // (METER && EXACT: the fused-demodulation items' meters would cost this kernel a spill -- 4 VGPRs of accumulators beside
    // the demodulation blocks' SGPRs; the planner keeps such trees in k_mix_levels + k_usb_demod instead: build_level_plan)
    run_item<EXACT, ROT, METER && !EXACT>(k1, K1Work{ldc(&items[it].vfo), ldc(&items[it].s_begin), ldc(&items[it].s_first_out), ldc(&items[it].s_end)},
                                A.L.frame_level[lv], A.L.raw, A.L.raw_mode, lv == 0, smem + wave * A.lds_wave, (int)threadIdx.x & 63);
}
