// kernels.hip -- hand-written HIP kernels of the per-VFO IQ chain for gfx950 (MI355X, CDNA4): the map of them, and the
// files they are in, included below in dependency order.
//
// Compiled with -ffp-contract=off: every a*b+c below is two roundings unless fmaf() is
// spelled out.  That is what makes the EXACT variants reproduce the reference's -O2 x86-64
// arithmetic bit for bit; the FAST variants use explicit fmaf() (option "exact" = 0: and the NCO table as
// rotations of its exact checkpoints, ROT; = 2, the robust arithmetic: FMAs, but the table replayed exactly).
//
// Kernel map: every __global__ of the chain, the file it is in, and the reference function (file:lines) it implements.
//   k_nco_init            nco.hip       Oscillator::Oscillator, oscillator.cpp:4-32: the table, kept as every 16th entry
//   k_vfo_retune          nco.hip       `delete osc_mix; osc_mix = new Oscillator(Fs, f)` on a running tree (the same recurrence), and gains
//   k_vfo_reset           nco.hip       (none: sdrx_set_active fills a leaf's state words between two frames, FillJob in sdrx_dev.h)
//   k_nco_dump            nco.hip       (none: table entries regenerated from the checkpoints, for the parity tests)
//   k_ingest_f32          ingest.hip    (none: a natural-order cf32 frame into the tile layout, sdrx_dev.h)
//   k_ingest_samples<FMT> ingest.hip    floats[b] = b - 127, jonti/sdr.cpp:43-49,122-129 and sdrj.cpp:155-160, into the tile layout (FMT =
//                                       SDRX_FMT_CU8; CS8 / CS16: none -- a wideband front end's int8 / int16 in the reference's units)
//   k_dc_products<FMT>    ingest.hip    \
//   k_dc_chain            ingest.hip     | sdrj::demodData's DC-bias removal, sdrj.cpp:271-286, bit for bit: k * curr of every sample; avept
//   k_dc_chain_spec       ingest.hip     | sample by sample, or a verified block of 1024 at a time; curr -= avept into the tile layout
//   k_dc_apply<FMT>       ingest.hip    /  (the kernels that read samples are templates on the format; the chain kernels serve every format)
//   k_dc_block_sums<FMT>  ingest.hip    \ the same in the tolerance arithmetic: a blocked scan of the linear recurrence
//   k_ingest_dc_fast<FMT> ingest.hip    /
//   k_adc_meter<FMT>      adcmeter.hip  (none: option adc_meter -- exact integer statistics of an integer frame as it arrived: sums, min / max,
//                                       rail counts, the longest rail run, a bit-length histogram; include/sdrx.h sdrx_adc_meter)
//   k_resample            resample.hip  (none: sdrx_set_resampler -- the polyphase rational resampler L/M between the ingest kernels and level 0, for
//                                       front ends whose rate no chain of half-bands reaches; include/sdrx.h "Resampler")
//   k_front_halfband<MODE> front.hip    (none: sdrx_set_front -- 1 .. 3 half-band decimations by 2 in front of k_resample or level 0; stage 1 may read
//                                       real int16 / 12-bit samples with the fs/4 translation built in; include/sdrx.h "Front stage")
//   k_blank, k_blank_step blank.hip     (none: sdrx_set_blanker -- the impulse blanker behind the format conversion and in front of the front stage, the
//                                       resampler or level 0: samples above ratio x a rank of the previous frame's power histogram, and a guard on
//                                       either side, become zero; include/sdrx.h "Impulse blanker")
//   k_iqbal, k_iqbal_step iqbal.hip     (none: sdrx_set_iq_balance -- the IQ balance correction behind the format conversion and the DC removal, in front
//                                       of the blanker: Q' = c I + d Q in place, and the pair (c, d) moved from exact integer statistics of each
//                                       frame's output; include/sdrx.h "IQ balance")
//   k_shift, k_shift_step shift.hip     mix_offset (README "tune ALL VFO's up or down"), as one stage: sdrx_set_shift -- the frequency shift at the end
//                                       of the ingest chain, in place on the tree's raw frame: y = x exp(+j 2 pi p / 2^32) from three 256-entry
//                                       tables, the 32-bit phase carried on the device from frame to frame; include/sdrx.h "Frequency shift")
//   k_notch_corr, k_notch_step, k_notch_apply notch.hip (none: sdrx_set_notch -- the spur canceller in front of the frequency shift, in place on the
//                                       tree's raw frame: up to eight tones, each a tracked complex amplitude times the shift's table oscillator,
//                                       estimated per block of 4096 samples and subtracted one block late; include/sdrx.h "Spur canceller")
//   k_mix_decimate        mix.hip       vfo::process mix loop, vfo.cpp:237-245; HalfBandDecimator::decimate, halfbanddecimator.cpp:43-72,
//                                       with FIR::...HalfBandQueue, dsp.cpp:96-173 (mix_item); option fuse_late: the FIR part of
//                                       vfo::usb_decimdemod, vfo.cpp:334-356, inside a d = 0 leaf's wave (late_item); option fuse_demod:
//                                       vfo::usb_demod inside a d = 2 leaf's wave (demod_chunk, demod.hip)
//   k_late_decimate       late.hip      vfo::usb_decimdemod (FIR part), vfo.cpp:334-387, with FIR::FIRUpdateAndProcess / FIRUpdate, dsp.cpp:59-71,150-154
//   k_late_decimate4      late.hip      the same for L in {5, 6} and at most 96 taps: one wave per 128 outputs
//   k_usb_demod           demod.hip     vfo::usb_demod / the demod tail of vfo::usb_decimdemod, vfo.cpp:300-332,350-364 (demod_block)
//   k_lpf_long            demod.hip     its audio low-pass when longer than kMaxFir taps: FIR::FIRUpdateAndProcess, dsp.cpp:59-71 (firfilter.cpp:108-119)
//   k_mix_levels          levels.hip    k_mix_decimate's items of every tree level in one launch (run_item, mix.hip)
//   k_levels_tail         levels.hip    the same plus k_usb_demod's blocks of the frame that left the last level (option tail_in_levels)
//   k_compress            compress.hip  vfo::compress, vfo.cpp:389-424
//   k_env_sum, k_detect<KIND> detect.hip (none: sdrx_set_detector -- the int16 payload of a non-USB leaf as an AM envelope (carrier = the frame's
//                                       own mean, summed in exact integers by k_env_sum) or an FM discriminator; include/sdrx.h "Detector leaves")
//   k_detect_post<KIND>   postdet.hip   (none: sdrx_set_postfilter -- the same leaf through a real FIR of the caller's taps over the detector's floats,
//                                       decimated by R, history carried per frame parity; include/sdrx.h "Post-detection filter")
// (The kernels beside the chain have files of their own, included by sdrx.hip: spectrum.hip, squelch.hip, agc.hip, watch.hip, wake.hip,
// drift.hip, scan.hip.)
//
// Execution model: 64-wide wavefronts.  k_mix_decimate runs ONE wave per workgroup and one
// workgroup per (VFO, time segment); a wave owns all the LDS it touches, so its
// __syncthreads() are wave-local (no cross-wave barrier traffic) and the segment walks the
// frame chunk by chunk with the filter state resident in LDS.
#include "sdrx_dev.h"
#include "sdrx_resample.h"
#include "sdrx_front.h"
#include "sdrx_blank.h"
#include "sdrx_iqbal.h"
#include "sdrx_shift.h"
#include "sdrx_notch.h"
#include "sdrx_detect.h"
#include "sdrx_postdet.h"

#include <type_traits>
#include <utility>

namespace sdrx {

#include "dev_helpers.hip"
#include "nco.hip"
#include "ingest.hip"
#include "adcmeter.hip"
#include "resample.hip"
#include "front.hip"
#include "blank.hip"
#include "iqbal.hip"
#include "shift.hip"
#include "notch.hip"
#include "meter.hip"
#include "demod.hip"
#include "mix.hip"
#include "late.hip"
#include "levels.hip"
#include "compress.hip"
#include "detect.hip"
#include "postdet.hip"

} // namespace sdrx
