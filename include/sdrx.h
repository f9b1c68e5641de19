/* include/sdrx.h -- C ABI of the MI355X-native per-VFO IQ chain (libsdrx.so).
 *
 * Drop-in boundary for ONE path of jeroenbeijer/SDRReceiver: the per-VFO chain
 *   table-NCO complex mix -> cascaded 11-tap half-band decimation -> USB demodulation
 *   (62-sample delay minus 125-tap Hilbert) -> optional Hamming low-pass -> int16
 * i.e. the arithmetic of vfo.cpp / oscillator.cpp / halfbanddecimator.cpp / jonti/dsp.cpp /
 * gnuradio/firfilter.cpp.  Everything around it (Qt GUI, RTL-SDR / rtl_tcp ingest, the ZeroMQ
 * socket) stays on the host side of this boundary; INTEGRATION.md shows the reference-side
 * binding.  All citations are file:line in the reference repository.
 *
 * Conventions: plain C types only, every function returns 0 on success and a negative
 * SDRX_E* code on failure (no exception crosses the ABI; sdrx_last_error() has the text).
 * A context is single-caller and not re-entrant -- like the reference, where all VFOs run on
 * one thread (sdrj.cpp:288-294).  There is no CPU fallback: without a usable HIP device
 * sdrx_create() fails.
 */
#ifndef SDRX_H
#define SDRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDRX_ABI_VERSION 5

enum {
    SDRX_OK = 0,
    SDRX_EINVAL = -1,   /* bad argument / bad descriptor                               */
    SDRX_ESTATE = -2,   /* call order violated (e.g. process before finalize)            */
    SDRX_EFILTER = -3,  /* tap design rejected: where the reference throws out_of_range  */
                        /* from firfilter::sanity_check_1f (firfilter.cpp:122-134)       */
    SDRX_EHIP = -4,     /* HIP runtime error                                             */
    SDRX_EUNSUPPORTED = -5, /* geometry outside what the kernels handle (see sdrx_finalize) */
    SDRX_ENOMEM = -6,
    SDRX_ENOSTREAM = -7 /* sdrx_get_stream: this VFO keeps no decimate[d] (a fused /5 | /6 leaf that is not a tap)  */
};

typedef struct sdrx_ctx sdrx_ctx;

/* One VFO node.  Each field replaces one reference setter; sdrx_add_vfo + sdrx_finalize
 * together replace `new vfo` + setters + vfo::init (vfo.cpp:60-176, called from
 * mainwindow.cpp:105-136 for main VFOs and 150-225 for sub VFOs). */
typedef struct sdrx_vfo_desc {
    int32_t fs;                 /* vfo::setFs                 vfo.cpp:189-193: input rate of THIS vfo */
    int32_t decimate_count;     /* vfo::setDecimationCount    vfo.cpp:194-197: half-band stages, 0..8 */
    double mixer_freq_hz;       /* vfo::setMixerFreq          vfo.cpp:199-204: integer Hz, may be < 0 */
    int32_t demod_usb;          /* vfo::setDemodUSB           vfo.cpp:468-472: 1 = USB audio leaf      */
    int32_t late_decimate;      /* vfo::init(..,lateDecimate) vfo.cpp:70-101: 0, 5 or 6               */
    int32_t filter_bw_hz;       /* vfo::setFilterBandwidth    vfo.cpp:223-227: 0 = no audio low-pass   */
    float gain;                 /* vfo::setGain               vfo.cpp:229-233                          */
    int32_t cstyle;             /* vfo::setCompressonStyle    vfo.cpp:455-460 (compress(), 389-424)    */
    int32_t scalecomp;          /* vfo::setScaleComp          vfo.cpp:462-467                          */
    int32_t parent_id;          /* vfo::setVFOs on the parent vfo.cpp:485-490; -1 = fed by the raw     */
                                /*   stream, i.e. a member of sdrj's main-VFO list (sdrj.cpp:288-294)  */
    int32_t samples_per_buffer; /* vfo::init(samplesPerBuffer) vfo.cpp:60: complex samples per frame   */
    char topic[8];              /* vfo::setZmqTopic: the first 5 bytes go on the wire                  */
                                /*   (zmqpublisher.cpp:91)                                              */
} sdrx_vfo_desc;

/* Replaces the call `ZmqPublisher::publish(buf, len, topic, sampleRate)` made by
 * vfo::transmitData (vfo.cpp:426-453, zmqpublisher.h:16).  Invoked once per publishing leaf per
 * frame, in the reference's order: main VFOs in list order, their sub VFOs in list order
 * (sdrj.cpp:288-294, vfo.cpp:257-263).  `buf` is owned by the library and valid until the next
 * sdrx_process*() / sdrx_wait() / sdrx_fetch() / sdrx_destroy() -- libzmq copies on zmq_send
 * (zmqpublisher.cpp:91-93), so the reference's publisher needs it no longer than the callback.
 * Not invoked for an empty payload (zmqpublisher.cpp:88).
 * With option "preroll" = 1, and only then, "once per leaf per frame" becomes "at most twice": a leaf that opens in the
 * delivered frame f after its squelch was closed in f-1 gets two invocations at its place in that order, its payload of frame
 * f-1 first, then that of f (same topic, same rate). */
typedef void (*sdrx_publish_fn)(void *user, const char topic[5], uint32_t sample_rate, const void *buf,
                                uint32_t len_bytes);

/* ---- lifetime ------------------------------------------------------------------------------ */
int sdrx_abi_version(void);
/* A short hash of the sources this library was compiled from (csrc/Makefile): what profiles and bench lines name as the
 * build they measured. */
const char *sdrx_build_id(void);
int sdrx_create(sdrx_ctx **ctx, int device_ordinal);
int sdrx_destroy(sdrx_ctx *ctx);
const char *sdrx_last_error(const sdrx_ctx *ctx); /* ctx may be NULL: error of a failed create */

/* ---- configuration ( = MainWindow building the VFO tree) ------------------------------------ */
int sdrx_add_vfo(sdrx_ctx *ctx, const sdrx_vfo_desc *desc, int *id_out);
/* Options, all before sdrx_finalize:
 *   "exact"  1 (default): every fp32 operation rounded like the reference's -O2 x86-64 build
 *            (no FMA contraction, reference summation order) -> results bit-identical to it.
 *            0: the TOLERANCE arithmetic -- what BASELINE.json's north_star grants ("within 1e-5 relative float
 *            tolerance"): every final complex stream and pre-quantisation float within 1e-5 of max|reference| per
 *            VFO-frame, int16 within 1 LSB (tests: every VFO of configs 3 / 4 and of the 10 240-VFO workload, 18 s runs
 *            without drift, the -Ofast build's fixtures).  The NCO table entries (oscillator.cpp:20-28) become rotations
 *            of the table's EXACT 16-entry checkpoints (<= 1e-6 from the table, never accumulating; the table's first 512
 *            entries and the first sample ever are still replayed exactly), the mixer (vfo.cpp:241) a packed multiply +
 *            FMA, the half-band / FIR dot products FMAs: ~230 instead of ~390 vector instructions per 1024 samples.
 *            Its NCO error (~1e-6 of |v|) multiplies the TOTAL input power while the bar is relative to the VFO's own
 *            output: a strong out-of-band carrier over a quiet channel eats the margin -- 100 LSB of carrier over +-1 LSB of
 *            noise: 6.4e-6 of max|stream|, 8.3e-6 on the pre-quantisation float
 *            (tests/test_gpu_parity.py::test_strong_carrier_over_quiet_channels).
 *            2: the ROBUST arithmetic -- the table entries from the exact recurrence (bit-identical to the reference's
 *            table: no NCO error at all), the mixer and every filter as FMAs as with 0 (~260 instructions per 1024 samples).
 *            What is left is FMA versus two roundings -- the kind of difference the reference's own -Ofast build (as shipped)
 *            has against its -O2 build, and on that adversarial input the same size: 4.3e-6 against their 4.0e-6.
 *   "keep_prequant" 1: also keep the pre-quantisation float `usb*gain*32768` per leaf
 *            (parity tests; sdrx_get_prequant).   default 0
 *   "segments" n: force n time-segments per VFO-frame in the decimation kernel (0 = auto).
 *   "pipeline" 0 (default) | 1: with 1 the leaf tail of a frame (late decimation, USB
 *            demodulation, compress) runs on a second HIP stream behind an event, so that it may
 *            overlap the mix/decimate launches of the NEXT frame when frames are queued back to
 *            back; results are bit-identical.  Measured on MI355X (profiles/README.md): the two
 *            kernels then share a VALU-bound machine and both stretch -- 0.119 vs 0.109 ms per
 *            frame on BASELINE config 3 -- so it is off by default and kept as an A/B switch.
 *   "fuse" 1 (default) | 0: frames queued on the device (sdrx_process_device) run the mix/decimate items
 *            of ALL tree levels in one launch (k_mix_levels); 0 = one launch per tree level (A/B switch).
 *   "frame_pipeline" 1 (default) | 0: with "fuse", level l of that one launch works on frame k - l (a
 *            software pipeline over the frames queued back to back), so a frame queued with
 *            sdrx_process_device is only COMPLETE after the next such call or after sdrx_sync /
 *            sdrx_fetch / sdrx_get_* (which run what is outstanding).  0 = every call runs its frame through
 *            all levels at once.  Results are bit-identical either way.
 *   "fuse_late" 1 (default) | 0: a USB leaf with decimate_count 0 and late_decimate 5 | 6 below a parent
 *            (vfo::usb_decimdemod, vfo.cpp:334-387: the reference mixes, low-passes and keeps every 5th / 6th
 *            sample in one pass) runs its decimating low-pass inside the mix wave and writes only the decimated
 *            stream to HBM; decimate[0] of such a leaf is kept only while it is the tap (sdrx_set_tap) or with
 *            "keep_streams".  0 = the two-kernel form (the mixed stream goes to HBM and comes back): A/B switch.
 *            Results are bit-identical either way.
 *   "fuse_demod" 0 (default) | 1: with 1 a USB leaf with decimate_count 2 below a parent and an audio low-pass of at most 64
 *            taps (the reference's 48 kS/s sub VFOs, vfo::usb_demod, vfo.cpp:300-332) demodulates inside its mix wave: 256
 *            stream samples per 1024-sample chunk go from registers through the wave's LDS to int16 and the leaf's cf32
 *            stream never reaches HBM (decimate[2] of such a leaf is kept only while it is the tap, sdrx_set_tap, or with
 *            "keep_streams").  Results are bit-identical with "exact" = 1 and 2; with "exact" = 0 they keep the same tolerance
 *            against the reference but are not bit-identical to the k_usb_demod form (the fused form cuts VFO-frames into
 *            other segments and chunks, which changes which chunks replay the NCO table exactly).  Measured on MI355X
 *            (round 6, profiles/README.md): it removes
 *            138 MB of HBM traffic per frame of BASELINE config 3 and is SLOWER -- 0.123 vs 0.112 ms per frame exact, 0.102 vs
 *            0.091 tolerance: the frame is bound by VALU issue, not by HBM, and the demodulation's plain fp32 MACs issue in
 *            pairs only beside other waves doing the same (k_usb_demod: 80 % paired at 7 waves per SIMD) -- inside the mix
 *            wave, five waves per SIMD most of which are in packed-fp32 phases, they do not.  Off by default; an A/B switch.
 *   "tail_in_levels" 1 (default) | 0: with "fuse" and "frame_pipeline", the USB demodulation of the frame that left the last
 *            tree level runs inside the NEXT k_mix_levels launch (k_levels_tail: one launch per step instead of two) -- where
 *            the planner finds it safe and faster: every demodulated leaf on the last tree level (frame parity of the leaf
 *            streams), four mix waves' LDS fitting as many waves on a CU as before, and at most 64 demodulation blocks per CU
 *            in the exact arithmetic, 16 in the others.  A frame is then complete one call later still;
 *            sdrx_sync / sdrx_fetch / sdrx_get_* run what is outstanding as before.  0 = the demodulation in a k_usb_demod
 *            launch behind the frame's last level (A/B switch).  Composes with "fuse_demod".  Results are bit-identical.
 *   "keep_streams" 0 (default) | 1: every such leaf also keeps decimate[d] of every frame (parity tests that
 *            compare every stream of the tree).
 *   "meter" 0 (default) | 1: with 1 every leaf also reports an output meter per frame (sdrx_get_meters).  0 changes
 *            nothing: same kernels, same launches, same device_bytes.  Payloads are bit-identical either way.
 *   "squelch" 0 (default) | 1: squelch-gated egress (sdrx_set_squelch below); 1 implies "meter".  0 changes nothing.  With 1
 *            and every threshold 0 (the start) every payload and callback is what it is with 0; sdrx_get_output of a leaf that
 *            was closed in the delivered frame gives SDRX_OK, *len_bytes = 0, *rate as always and a non-NULL *buf that is not to
 *            be read, and the publish callback is not invoked for it (the rule for an empty payload).
 *   "preroll" 0 (default) | 1: squelch pre-roll (sdrx_get_preroll below); 1 implies "squelch".  0 changes nothing.  With 1 a
 *            leaf that is open in frame f and was closed by the gate in frame f-1 is delivered with its payload of f-1 as
 *            well, ahead of that of f: one frame, which is what the device still holds.  With "fuse_demod" leaves the tree
 *            keeps k_mix_levels + k_usb_demod in every arithmetic ("tail_in_levels" is not used), and "pipeline" = 1 loses its
 *            overlap.
 *   "squelch_auto" 0 (default) | 1: the gate's threshold follows each leaf's own noise floor (sdrx_set_squelch_auto below); 1
 *            implies "squelch".  0 changes nothing.  With 1 and every ratio_q8 0 (the start) the gate is that of "squelch" = 1.
 *            Composes with "preroll", "fuse_demod", "tail_in_levels" and "pipeline" as "squelch" does: the gate keeps its
 *            place in the launch sequence.
 *   "park" 0 (default) | 1: leaves can be switched off and on between frames (sdrx_set_active below).  0 changes nothing:
 *            the same kernels, launches, device_bytes and payloads, and sdrx_set_active returns SDRX_ESTATE.  With 1 and
 *            nothing parked every payload, stream, meter, squelch decision and callback is bit for bit what it is with 0; the
 *            kernels are then the forms that read one flag word per work item first.
 *   "watch" 0 (default) | 1: channel watch (sdrx_set_watch below): the power inside any leaf's passband, measured on the stream
 *            the leaf is fed, whether the leaf is active or parked.  0 changes nothing: the same kernels, launches,
 *            device_bytes, payloads and callbacks, and the watch calls return SDRX_ESTATE.  1 is independent of "park", "meter"
 *            and "squelch"; until the first sdrx_set_watch switches a leaf on, device_bytes and the launches are those of 0
 *            (DESIGN.md section 4j).
 *   "catchup" 0 (default) | 1: a leaf unparked with sdrx_set_active starts one frame back, on the frame the device still holds
 *            (sdrx_get_catchup below); 1 implies "park" and "preroll", hence "squelch" and "meter".  0 changes nothing: the
 *            same kernels, launches, device_bytes, payloads and callbacks, and sdrx_get_catchup returns SDRX_ESTATE.  With 1
 *            and nothing caught up every frame is what "park" = 1 with "preroll" = 1 gives.  A
 *            sdrx_finalize that fails leaves the options as they were set, as with "preroll".
 *   "agc" 0 (default) | 1: the gain of every USB leaf follows its output meter between frames, on the device (sdrx_set_agc
 *            below); 1 implies "meter".  0 changes nothing: the same kernels, launches, device_bytes, payloads and callbacks,
 *            and the AGC calls return SDRX_ESTATE.  With 1 and every hi_ms 0 (the start) every frame is what "meter" = 1 gives;
 *            one more small launch per frame, and the planning rules of "preroll" on "fuse_demod" trees.
 *   "wake" 0 (default) | 1: the watch unparks and parks leaves itself, inside the frame, on the device (sdrx_set_wake below);
 *            1 implies "park" and "watch".  0 changes nothing: the same kernels, launches, device_bytes, payloads and
 *            callbacks, and the wake calls return SDRX_ESTATE.  With 1 and no leaf under control every frame and record is bit
 *            for bit what "park" = 1 with "watch" = 1 gives, and nothing is allocated and no launch added until the first
 *            sdrx_set_wake that switches a leaf on.  What 1 costs in the launch plan: with "pipeline" = 1 the levels of a frame
 *            wait for the tail of the frame before (the two-stream overlap is lost); "tail_in_levels" is not used; a tree with
 *            a leaf off its last level runs one launch per level instead of the software pipeline.
 *   "dc_blocked_scan" 0|1 (default 0): how sdrx_process_u8 removes the DC bias.  0 = the
 *                 reference's sequentially rounded fp32 recurrence, bit for bit (below).  1 = the same linear filter as a
 *                 blocked parallel scan (~15 us): the true IIR response.  The reference's recurrence
 *                 wanders around that by up to ~3e-3 of the DC offset (its rounding errors are
 *                 correlated from step to step), so 1 is NOT within the 1e-5 parity tolerance
 *                 of the reference unless the offset is well below 1 LSB.
 *   "dc_speculative" 1 (default) | 0: how the bit-exact recurrence is evaluated.  1 = blocks of 1024 samples as integer
 *                 prefix sums of the mantissa, several blocks side by side per step, each step VERIFIED (binade, sign
 *                 and the rounding of avept * (1 - 1e-6) unchanged through it, no exact ties), taken again block by
 *                 block where that fails and redone with the sequential operations where a single block fails: bit-exact
 *                 by construction, at worst the sequential time (sdrx_stats.dc_blocks / dc_retried_blocks /
 *                 dc_fallback_blocks).
 *   "dc_blocks_per_step" 1 | 2 | 4 | 8: how many 1024-sample blocks one step of that evaluation takes side by
 *                 side (= waves of the one workgroup per component).  Same results for every value; anything else is
 *                 SDRX_EINVAL.  (The sequential recurrence for every sample -- ~2.0 ms per frame: two waves, each alone
 *                 with its dependent chain -- is option "dc_speculative" = 0, not a value of this one.) */
int sdrx_set_option(sdrx_ctx *ctx, const char *name, int value);
/* All of vfo::init for every node: NCO tables (oscillator.cpp:4-32), low-pass designs
 * (firfilter.cpp:64-119), Hilbert taps (dsp.cpp:184-217), zeroed filter state, buffers.
 * SDRX_EFILTER where the reference would throw; SDRX_EUNSUPPORTED unless for every node
 * fs % 16 == 0, samples_per_buffer % 16 == 0 and samples_per_buffer % 2^decimate_count == 0
 * (true for every rate the reference accepts, mainwindow.h:29), and a child's
 * samples_per_buffer equals its parent's samples_per_buffer / 2^decimate_count. */
int sdrx_finalize(sdrx_ctx *ctx);
int sdrx_set_publish_callback(sdrx_ctx *ctx, sdrx_publish_fn fn, void *user);
/* What vfo::init would do with this descriptor, decided on the host without touching a device (so a
 * binding can fail at init() time exactly where the reference does): SDRX_OK; SDRX_EFILTER where
 * firfilter::sanity_check_1f throws std::out_of_range (firfilter.cpp:122-134) -- `msg` then holds the
 * reference's what() text, e.g. "firdes check failed: 0 < fa <= sampling_freq / 2"; SDRX_EINVAL /
 * SDRX_EUNSUPPORTED for descriptors sdrx_add_vfo / sdrx_finalize refuse (`msg` says why).  `msg` may
 * be NULL. */
int sdrx_check_vfo(const sdrx_vfo_desc *desc, char *msg, size_t msg_cap);

/* ---- per frame ( = sdrj::demodData, sdrj.cpp:266-305) ---------------------------------------- */
/* `iq`: n_complex interleaved (I,Q) float pairs on the HOST, as sdr::audio_signal_out /
 * sdrj::readyRead deliver them (values b-127, jonti/sdr.cpp:43-49).  n_complex must equal the
 * samples_per_buffer of the parent-less VFOs.  Synchronous: on return every payload is in host
 * memory and the publish callback has run for every leaf.  The DC-bias IIR of sdrj.cpp:271-286
 * stays on the caller's side of this entry point (or use sdrx_process_u8). */
int sdrx_process(sdrx_ctx *ctx, const float *iq, int n_complex);
/* Raw dongle bytes (2 per complex sample, unsigned, offset 127) with the byte->float LUT
 * (jonti/sdr.cpp:43-49,122-129; sdrj.cpp:155-160) and, if correct_dc != 0, the DC-bias IIR
 * (sdrj.cpp:271-286) done on the device.  Otherwise like sdrx_process. */
int sdrx_process_u8(sdrx_ctx *ctx, const uint8_t *iq_bytes, int n_complex, int correct_dc);

/* ---- integer sample formats: one front door for dongle bytes and wideband front ends ---------
 * `fmt` of the *_fmt calls.  Every format maps to the SAME units, the reference's "dongle LSB, |x| <= 128": the shipped INI
 * gains and every squelch, AGC and watch threshold live in those units, and the device's DC-bias removal is proved bit-exact
 * for exactly that bound.  The scale is therefore FIXED: there is no per-call scale or shift, and cf32 frames are not offered
 * with DC removal on the device (unbounded floats break the bound).
 *
 *   constant           memory                      sample value x (fp32, exact)       range
 *   SDRX_FMT_CU8  = 0  uint8 I,Q                   b - 127                            [-127, 128]   (RTL dongles; = sdrx_*_u8)
 *   SDRX_FMT_CS8  = 1  int8 I,Q                    (float)v                           [-128, 127]   (HackRF)
 *   SDRX_FMT_CS16 = 2  native-endian int16 I,Q     (float)v * 2^-8                    [-128, 128)   (Airspy, SDRplay, USRP sc16, LimeSDR)
 *
 * correct_dc != 0: avept = fl(fl(avept * (1 - 1e-6f)) + fl(1e-6f * x)), x - avept (sdrj.cpp:277-283) on x as defined above, with
 * the context's ONE accumulator -- the format may change from frame to frame.  Options "dc_blocked_scan", "dc_speculative" and
 * "dc_blocks_per_step" apply as for bytes.  SDRX_FMT_CU8 is the sdrx_*_u8 path itself: the same launches, the same bits.  The
 * signed formats always enter through one conversion pass into the tile layout (2-4 bytes read, 8 written per sample).
 * An unknown fmt is SDRX_EINVAL; pointer, n_complex and in-flight rules as for the calls they are named after.
 * Afterwards sdrx_get_raw serves the float frame (DC-corrected if it was); sdrx_submit_shared and its siblings refuse a source
 * whose last frame was SDRX_FMT_CS8 / SDRX_FMT_CS16 (SDRX_ESTATE, as after a DC-corrected frame). */
#define SDRX_FMT_CU8 0
#define SDRX_FMT_CS8 1
#define SDRX_FMT_CS16 2
int sdrx_process_fmt(sdrx_ctx *ctx, const void *iq, int n_complex, int fmt, int correct_dc);

/* Device-resident variant for pipelines that already hold the frame in HBM (bench.py, the
 * multi-GPU path where the frame arrives by RCCL broadcast): `dev_iq` is a DEVICE pointer to
 * n_complex cf32.  Asynchronous on the context's stream; sdrx_fetch() waits, copies the payloads
 * to the host and runs the callbacks; sdrx_sync() only waits. */
int sdrx_process_device(sdrx_ctx *ctx, const void *dev_iq, int n_complex);
int sdrx_fetch(sdrx_ctx *ctx);
int sdrx_sync(sdrx_ctx *ctx);
/* Run on a caller-provided hipStream_t (e.g. torch's current stream) instead of the context's
 * own; NULL restores the default.  The frame is consumed on that stream (work the caller queues on
 * it after sdrx_process_device may overwrite the frame); with option "pipeline" the leaf tail runs
 * on a stream of the library's own, which sdrx_sync / sdrx_fetch / sdrx_wait also wait for. */
int sdrx_set_stream(sdrx_ctx *ctx, void *hip_stream);

/* ---- pipelined per-frame interface ("optional async submit/wait pair") ---------------
 * sdrx_submit* enqueue one frame and return at once: host -> device copy of the frame (staged through
 * pinned memory of the library's own: `iq` is borrowed for the duration of the call only, like the
 * argument of sdrj::demodData), kernels, and the device -> host copy of that frame's payloads on a
 * copy stream -- which therefore overlaps the kernels of the next frame.  (Frames of sdrx_submit_u8 with correct_dc: that
 * copy is issued by sdrx_wait instead, once the frame's kernels have ended -- measured, it is the order in which the next
 * frame's DC recurrence and the copy do run side by side)  sdrx_wait delivers the
 * OLDEST frame not yet delivered: it blocks until that frame's payloads are in host memory, then
 * runs the publish callback for every leaf in the reference's order (= ZmqPublisher::publish per
 * leaf, vfo.cpp:426-453); afterwards sdrx_get_output serves that frame.  At most
 * SDRX_MAX_IN_FLIGHT frames may be submitted and not yet delivered (SDRX_ESTATE otherwise).
 * The steady state of a streaming host is  submit(f+1); wait() -> f;  i.e. one frame of latency in
 * exchange for PCIe and kernels running concurrently.  sdrx_process* are submit + wait of one frame.
 * While frames are in flight sdrx_get_output keeps serving the last DELIVERED frame (its payloads sit in
 * host memory); the synchronous calls (sdrx_process*, sdrx_fetch) and the device read-backs
 * (sdrx_get_stream, sdrx_get_raw, sdrx_get_prequant) return SDRX_ESTATE -- the device buffers behind them
 * already belong to a newer frame.  sdrx_get_kernel_times waits for everything queued. */
#define SDRX_MAX_IN_FLIGHT 2
int sdrx_submit(sdrx_ctx *ctx, const float *iq, int n_complex);
int sdrx_submit_u8(sdrx_ctx *ctx, const uint8_t *iq_bytes, int n_complex, int correct_dc);
/* sdrx_submit_device: `dev_iq` is a DEVICE pointer to n_complex cf32 on this context's device.  No host staging: the frame
 * is read where it lies, so it must be complete in the order of the context's stream (sdrx_set_stream; the context's own
 * stream by default: then complete already at the time of the call) and stay untouched until sdrx_wait has delivered
 * this frame.  sdrx_get_raw returns SDRX_ESTATE after such a frame (caller-owned device memory). */
int sdrx_submit_device(sdrx_ctx *ctx, const void *dev_iq, int n_complex);
/* The *_fmt forms (formats above).  sdrx_submit_fmt: like sdrx_submit_u8.  The two device forms take integer samples that
 * already lie in this context's device memory -- rtl_tcp or front-end samples landed by another kernel or a peer copy --
 * 16-byte aligned (SDRX_EINVAL otherwise, nothing queued) and complete in the order of the context's stream:
 * sdrx_process_device_fmt queues the frame like sdrx_process_device (sdrx_fetch / sdrx_sync afterwards), sdrx_submit_device_fmt
 * like sdrx_submit_device (sdrx_wait afterwards).  The samples must stay untouched until the frame's conversion has run:
 * until sdrx_sync, sdrx_fetch or sdrx_wait returns. */
int sdrx_submit_fmt(sdrx_ctx *ctx, const void *iq, int n_complex, int fmt, int correct_dc);
int sdrx_process_device_fmt(sdrx_ctx *ctx, const void *dev_iq, int n_complex, int fmt, int correct_dc);
int sdrx_submit_device_fmt(sdrx_ctx *ctx, const void *dev_iq, int n_complex, int fmt, int correct_dc);
/* Two contexts on ONE device fed the same raw frame -- sdrj::demodData hands every main VFO the same `samples`
 * (sdrj.cpp:288-294), and a binding that keeps one context per main VFO (host/qt/vfo_adapter.cpp) would otherwise
 * upload the frame once per main: run through `ctx` the frame `src` staged LAST (host floats or dongle bytes given
 * to sdrx_process* / sdrx_submit* of `src`; not after a DC-bias removal on the device) without another
 * host-to-device copy.  `ctx` waits for src's upload on the device.  src's frame buffers are per frame parity: the
 * shared frame stays valid until `src` stages the frame after next -- wait for it on `ctx` before that.  `ctx` and `src`
 * must be driven from one thread (the call touches both; contexts carry no locks -- like the reference, where every VFO
 * runs on the one thread of sdrj::demodData). */
int sdrx_submit_shared(sdrx_ctx *ctx, sdrx_ctx *src);
int sdrx_process_shared(sdrx_ctx *ctx, sdrx_ctx *src); /* = sdrx_submit_shared + sdrx_wait */
/* The same for a binding that cannot KNOW that two main VFOs were handed the same samples (host/qt/vfo_adapter.cpp: `class
 * vfo` only sees process(samples) calls): `iq` is compared byte for byte with the pinned staging copy of the frame `src`
 * staged last (a memcmp of the frame instead of its upload).  Equal: exactly sdrx_submit_shared / sdrx_process_shared.  Not
 * equal (or src staged bytes, not floats): SDRX_DIFFERENT (> 0), nothing queued -- submit the frame normally. */
#define SDRX_DIFFERENT 1
int sdrx_submit_if_same(sdrx_ctx *ctx, sdrx_ctx *src, const float *iq, int n_complex);
int sdrx_process_if_same(sdrx_ctx *ctx, sdrx_ctx *src, const float *iq, int n_complex);
int sdrx_wait(sdrx_ctx *ctx);
int sdrx_in_flight(sdrx_ctx *ctx); /* >= 0: frames submitted and not yet delivered; < 0: error */

/* ---- results -------------------------------------------------------------------------------- */
/* Payload of leaf `id` after the last frame: int16 audio (USB leaf) or packed int8 IQ
 * (compress(), vfo.cpp:389-424).  *rate = outputRate (vfo.cpp:102). */
int sdrx_get_output(sdrx_ctx *ctx, int id, const void **buf, uint32_t *len_bytes, uint32_t *rate);
/* Output meters (option "meter" = 1): what leaf ids[k]'s payload of the last DELIVERED frame -- the one sdrx_get_output
 * serves -- holds, computed on the device where the payload is produced and copied out with it (readable while the next
 * frame is in flight; for sdrx_process_device frames this runs what is outstanding first, as sdrx_get_output does).
 *   USB leaf (int16):      pre = usb' * gain * 32768.0 as the reference computes it (vfo.cpp:328,364), v = the int16 sent;
 *                          n_values = n_out; a sample wrapped when !(pre > -32769.0 && pre < 32768.0) (NaN included):
 *                          exactly where the truncating conversion to short differs from trunc(pre).
 *   compress() leaf (int8): per component pre = re * 128 (cstyle 0) or (re / scalecomp) * 128 (cstyle 1), v = its int8
 *                          value before cstyle 1's nibble masking; n_values = 2 n; a sample wrapped when either component
 *                          has !(pre > -129 && pre < 128).
 * sum_sq = sum of v * v (exact), peak = max |pre| in LSB of the payload type (NaN if any pre was NaN).
 * SDRX_ESTATE with the option off, before sdrx_finalize or before any frame was delivered; SDRX_EINVAL for a bad id, a
 * VFO with children (it publishes nothing) or n < 0; n == 0 does nothing.
 * This and every per-leaf list call below checks in one order, and the first thing wrong decides the code: handle, finalized,
 * option, list shape, ids (range, leaf, listed once in a setter), values, broken (group), frames in flight or delivered. */
typedef struct sdrx_meter {
    int64_t frame;     /* index of the frame these figures belong to (0 = first frame after finalize) */
    uint64_t sum_sq;   /* sum of v*v over the payload values v of that frame (exact integer) */
    uint32_t n_values; /* how many values were summed */
    uint32_t clipped;  /* samples whose conversion left the payload type's range (i.e. wrapped) */
    float peak;        /* max |pre-quantisation value|, in LSB of the payload type; NaN if any was NaN */
    uint32_t reserved;
} sdrx_meter;
int sdrx_get_meters(sdrx_ctx *ctx, const int *ids, int n, sdrx_meter *out);
/* Squelch-gated egress (option "squelch" = 1): every leaf has a threshold thr_sum_sq in units of its meter's sum_sq (0 = always
 * open: the default), a hang time in frames and a state hang_left (0 after sdrx_finalize).  For every frame the context
 * processes, on whichever path, with s = the leaf's meter sum_sq of that frame, decided on the device in integers:
 *     if s >= thr: open, hang_left = hang_frames;  else if hang_left > 0: open, hang_left -= 1;  else closed.
 * The open leaves' payloads are packed into one dense device buffer, and only those bytes are copied to the host (plus a part
 * of fixed size: the meter records of EVERY leaf -- sdrx_get_meters answers for closed leaves too, which is how a threshold is
 * chosen -- and the gate's directory).  The reference has no squelch (vfo.cpp:426-453 publishes every leaf every frame).
 * sdrx_set_squelch: batched and atomic like sdrx_set_gains -- the whole list is checked first; a bad, duplicate or non-leaf id
 * or n < 0 is SDRX_EINVAL with nothing changed; n == 0 does nothing; SDRX_ESTATE before sdrx_finalize, with the option off and
 * while submitted frames are undelivered; frames the software pipeline of sdrx_process_device still holds run to their end with
 * the old values first.  It resets hang_left of the named leaves to 0.  One small upload and one small launch per call.
 * sdrx_get_squelch: the state after the last DELIVERED frame (the one sdrx_get_output serves); calling rules of
 * sdrx_get_meters.
 * sdrx_get_egress: what the payload copy of the last delivered frame moved -- payload bytes only; the part of fixed size is
 * not counted.  Host bookkeeping (with the option off: every leaf, the whole payload region).  Each pointer may be NULL. */
typedef struct sdrx_squelch_state {
    int64_t frame;       /* the frame this state follows */
    uint64_t thr_sum_sq; /* as set */
    uint32_t hang_frames, hang_left;
    int32_t open;        /* 1: the leaf's payload of that frame was copied out and published */
    uint32_t reserved;
} sdrx_squelch_state;
int sdrx_set_squelch(sdrx_ctx *ctx, const int *ids, const uint64_t *thr_sum_sq, const uint32_t *hang_frames, int n);
int sdrx_get_squelch(sdrx_ctx *ctx, const int *ids, int n, sdrx_squelch_state *out);
int sdrx_get_egress(sdrx_ctx *ctx, int64_t *frame, uint32_t *n_open, uint32_t *n_leaves, uint64_t *payload_bytes_copied);
/* Squelch pre-roll (option "preroll" = 1).  Per leaf one more bit of device state, prev_open: 1 after sdrx_finalize (frame 0 has
 * no predecessor), and after every gate that gate's `open`; sdrx_set_squelch does not touch it.  With open(f) as above:
 *     pre(f) = open(f) && !prev_open;   prev_open = open(f)
 * A frame delivered with pre(f) = 1 for a leaf carries that leaf's payload of frame f-1 too; the callback sees it first
 * (sdrx_publish_fn).  The rule follows the gate, not the host: after several sdrx_process_device calls sdrx_fetch delivers the
 * last frame and, where due, the pre-roll of the one before it, which was never delivered itself.
 * sdrx_get_output is unchanged (frame f's payload).  sdrx_get_preroll: the leaf's pre-rolled payload in the delivered frame and
 * *frame = f-1, or SDRX_OK with *len_bytes = 0 (and a non-NULL *buf that is not to be read); calling rules and buffer lifetime
 * of sdrx_get_output; SDRX_ESTATE with the option off.  Each pointer may be NULL.
 * sdrx_get_preroll_count: for the delivered frame, how many leaves are pre-rolled and how many bytes (payloads padded to 64)
 * that added to the copy; calling rules of sdrx_get_egress, whose payload_bytes_copied includes them (it reports what the copy
 * moved) and whose n_open stays the number of open leaves.
 * The two calls differ after sdrx_process_device, as sdrx_get_squelch and sdrx_get_egress do: sdrx_get_preroll brings the last
 * queued frame over itself (an implicit sdrx_fetch, callbacks included), sdrx_get_preroll_count refuses with SDRX_ESTATE until
 * sdrx_fetch or another sdrx_get_* has delivered it.
 * A sdrx_finalize that fails (memory: the packed buffers double) leaves the options as they were set, so "preroll" can be
 * switched off and sdrx_finalize called again. */
int sdrx_get_preroll(sdrx_ctx *ctx, int id, const void **buf, uint32_t *len_bytes, int64_t *frame);
int sdrx_get_preroll_count(sdrx_ctx *ctx, uint32_t *n_preroll, uint64_t *preroll_bytes);
/* Auto-squelch (option "squelch_auto" = 1): the gate's threshold as a RATIO over the leaf's own noise floor, the floor tracked
 * on the device by minimum statistics over a sliding window of frames.  Per leaf two more settings -- ratio_q8 (a power ratio
 * times 256; 0 = off for this leaf: the default) and window_frames (>= 1 wherever ratio_q8 > 0) -- and three more words of
 * device state: cur_min, prev_min (uint64) and age (uint32); NONE = 2^64 - 1 is "no observation".  After sdrx_finalize, and
 * after every sdrx_set_squelch_auto that names the leaf: cur_min = prev_min = NONE, age = 0.  For every frame the context
 * processes, on whichever path, with s = the leaf's meter sum_sq of that frame, in integers:
 *     floor   = min(cur_min, prev_min)                               (from the frames BEFORE this one)
 *     auto    = 0 if ratio_q8 == 0 or floor == NONE, else min(2^64 - 1, (floor * ratio_q8) >> 8)     (the product in 128 bits)
 *     thr_eff = max(thr_sum_sq, auto);   open / hang_left: the rule of sdrx_set_squelch with thr_eff in place of thr_sum_sq
 *     cur_min = min(cur_min, s);  age += 1;  if age == window_frames: prev_min = cur_min, cur_min = NONE, age = 0
 * What follows from it: the first frame after sdrx_finalize or a restart decides with thr_sum_sq alone (open, with the
 * defaults); a frame of zeros makes the floor 0, so the gate fails open (thr_eff = thr_sum_sq) for at most 2 * window_frames
 * - 1 frames; a burst never lifts its own threshold (the floor excludes the current frame), but a transmission longer than
 * 2 * window_frames - 1 frames becomes the floor and, with ratio_q8 > 256, closes: choose window_frames above the longest
 * transmission and keep ratio_q8 = 0 on continuous channels.  thr_sum_sq stays a lower bound.  sdrx_set_squelch does not touch
 * the floor state; sdrx_set_squelch_auto does not touch thr_sum_sq, hang_frames, hang_left or prev_open; pre-roll follows
 * `open` as before.  There is no default ratio or window: what a real front end needs has not been measured.
 * sdrx_set_squelch_auto: batched and atomic, with the calling rules of sdrx_set_squelch; besides, window_frames[k] == 0 with
 * ratio_q8[k] > 0 is SDRX_EINVAL with nothing changed.  One small upload and one small launch per call.
 * sdrx_get_squelch_auto: for the last DELIVERED frame, the floor and the threshold that decided it; calling rules of
 * sdrx_get_squelch.  ratio_q8 and window_frames are as set. */
typedef struct sdrx_squelch_auto_state {
    int64_t frame;           /* the frame these values decided */
    uint64_t floor_sum_sq;   /* min(cur_min, prev_min) in front of that frame; 0 while floor_valid is 0 */
    uint64_t thr_eff_sum_sq; /* max(thr_sum_sq, auto) */
    uint32_t ratio_q8, window_frames;
    uint32_t floor_valid;    /* 0: the leaf had no observation yet */
    uint32_t reserved;
} sdrx_squelch_auto_state;
int sdrx_set_squelch_auto(sdrx_ctx *ctx, const int *ids, const uint32_t *ratio_q8, const uint32_t *window_frames, int n);
int sdrx_get_squelch_auto(sdrx_ctx *ctx, const int *ids, int n, sdrx_squelch_auto_state *out);

/* Parking (option "park" = 1): a leaf VFO switched off costs no arithmetic on the device, and a leaf switched on again starts
 * as a NEW vfo does -- together with sdrx_set_mixer_freqs the reference's `new vfo` + setters + vfo::init + setVFOs between two
 * sdrj::demodData calls: finalize with spare leaves, park them, and retune and unpark one when a channel is assigned.
 * Only leaves can be parked.  A VFO with children keeps running even when all its children are parked.
 *
 * A leaf that is PARKED in a frame does no mix, decimation, demodulation, compress, long low-pass or spectrum work in it, and
 * is delivered as a leaf that option "squelch" closed: no publish callback; sdrx_get_output gives SDRX_OK, *len_bytes = 0,
 * *rate as always and a non-NULL *buf that is not to be read; sdrx_get_preroll gives *len_bytes = 0; the other leaves'
 * callbacks keep their order.  sdrx_get_stream and sdrx_get_prequant return SDRX_ENOSTREAM; an enabled spectrum's `updates`
 * does not move (its display state is kept); a tap selection is kept and writes nothing; sdrx_get_meters gives the delivered
 * `frame` and n_values = sum_sq = clipped = 0, peak = 0.  Under "squelch" / "preroll" / "squelch_auto" the gate gives open = 0
 * and no pre-roll whatever the threshold is (threshold 0 = "always open" holds for active leaves only) and leaves hang_left,
 * prev_open and the floor state untouched -- a parked frame is not an observation; sdrx_get_squelch and sdrx_get_squelch_auto
 * report that frozen state with open = 0; sdrx_get_egress: n_leaves unchanged, n_open counts open active leaves, a parked leaf
 * adds no packed bytes.  Without "squelch" the payload region is still copied whole and n_open is the number of active leaves.
 * sdrx_set_mixer_freqs, sdrx_set_gains, sdrx_set_squelch and sdrx_set_squelch_auto accept a parked leaf and store the values.
 *
 * A leaf UNPARKED before frame K is, from K on, a new vfo with the leaf's descriptor as it stands (the mixer frequency and gain
 * last set): its oscillator starts fresh (sample 0 of frame K takes the table's last entry, as after sdrx_set_mixer_freqs), every
 * filter state is zero (half-band histories, late decimation, delay and Hilbert, audio low-pass), and its gate state is that of
 * sdrx_finalize (hang_left = 0, prev_open = 1: no pre-roll of a stale payload; no floor observation) -- thresholds, hang time,
 * ratio and window are kept, and so is the display state of an enabled spectrum.  Park followed by unpark with no frame
 * between is allowed: it restarts the leaf.
 *
 * sdrx_set_active: batched and atomic, with the calling rules of sdrx_set_gains / sdrx_set_squelch -- the whole list is checked
 * first: a bad or duplicate id, the id of a VFO with children, active[k] not 0 or 1 or n < 0 is SDRX_EINVAL with nothing
 * changed; n == 0 does nothing; SDRX_ESTATE before sdrx_finalize, with the option off, and while submitted frames are
 * undelivered.  Frames the software pipeline of sdrx_process_device still holds run to their end with the old values first.
 * An entry that names the state the leaf is already in is ignored (no reset).  One upload and two small launches; the call
 * returns when the device has applied it.  (A changed leaf with an enabled spectrum costs one more small upload.)
 * sdrx_get_active: host bookkeeping, good from sdrx_finalize on and with the option off (every leaf active since frame 0). */
typedef struct sdrx_active_state {
    int64_t since_frame;  /* first frame index in the present state (0 after sdrx_finalize) */
    int32_t active;       /* 1 after sdrx_finalize */
    uint32_t reserved;
} sdrx_active_state;
int sdrx_set_active(sdrx_ctx *ctx, const int *ids, const int32_t *active, int n);
int sdrx_get_active(sdrx_ctx *ctx, const int *ids, int n, sdrx_active_state *out);
/* Unpark with catch-up (option "catchup" = 1): a woken leaf starts one frame back.  A parent writes decimate[d] of every frame
 * into the buffer of that frame's parity whether or not a child is active, and after frame K-1 that stream stays untouched until
 * frame K+1: what an unparked leaf needs for K-1 is still on the device.  The reference has no counterpart: this text is the
 * definition.
 *
 * Let K be the index of the next frame.  A leaf named by sdrx_set_active with active = 1 (and parked until then) is CAUGHT UP
 * when it has a parent (parent_id >= 0), K >= 1, and it was parked in frame K-1.  A caught-up leaf
 *   - is a new vfo, with the descriptor as it stands (mixer frequency and gain last set), from frame K-1 on: its oscillator
 *     starts fresh at sample 0 of frame K-1, and every state region is zero, as for any unparked leaf;
 *   - runs frame K-1 before sdrx_set_active returns: mix, half-bands, late decimation, demodulation, long low-pass or compress on
 *     its parent's decimate[d] of K-1, read where it lies, into the leaf's own buffers of that frame's parity (stream, filter
 *     state, meter records, payload); frame K then continues from that state like any second frame;
 *   - has the gate state of sdrx_finalize EXCEPT prev_open = 0.  No gate runs on K-1, so in frame K pre(K) = open(K): if the
 *     leaf is open in K (always, with threshold 0) the delivered frame K carries its payload of K-1 first -- the callback is
 *     invoked twice, sdrx_get_preroll gives it with *frame = K-1, sdrx_get_preroll_count and sdrx_get_egress count it.  With
 *     a threshold > 0 and the leaf closed in K the caught-up payload is dropped; hang_frames does not help, because no gate has
 *     run on it.  Read sdrx_get_catchup to know what it held.
 * Leaves that are not caught up start at K exactly as without the option, with prev_open = 1: a leaf without a parent (the raw
 * frame of K-1 may be the caller's memory), a leaf unparked at K = 0, and a leaf parked and unparked with no frame between (it
 * was active in K-1 and delivered then: the restart).  Parking a caught-up leaf again before frame K discards the catch-up.
 *
 * Everything the host reports for frame K-1 stays "parked" for that leaf: sdrx_get_output and sdrx_get_meters of a K-1 still to
 * be fetched (frames queued with sdrx_process_device), n_open, and sdrx_get_active's since_frame = K.  A spectrum or a watch is
 * not updated by the catch-up; sdrx_get_stream keeps its rules (SDRX_ENOSTREAM until frame K has run).
 * The catch-up is this form whatever "fuse", "frame_pipeline", "tail_in_levels" or "pipeline" are: sub-lists of the leaf's own
 * work items through one k_mix_decimate launch per tree level and one launch per block kernel, uploaded with the call's jobs.
 * The call still returns when the device has applied it: it costs about one frame's work of the woken leaves more.
 *
 * One frame, no more: a host that pipelines `submit(f+1); wait() -> f` reads the figures of f only after f+1 is submitted, must
 * wait for f+1 before it may call sdrx_set_active, and so catches up f+1, not f.  The synchronous loop
 * process(f) -> sdrx_get_watch -> sdrx_set_mixer_freqs / sdrx_set_active -> process(f+1) loses nothing of f.
 *
 * sdrx_get_catchup: per leaf the meter of the caught-up frame -- frame = K-1 and sum_sq, n_values, clipped, peak by the
 * definition of sdrx_get_meters -- or frame = -1 and zeros if the leaf's present active state did not begin with a catch-up.
 * sdrx_set_active copies the few records back itself, so this is host bookkeeping that can be read as soon as that call has
 * returned: the host knows whether the burst was there before it spends frame K.  Calling rules of sdrx_get_active, except
 * SDRX_ESTATE with the option off: a bad id, the id of a VFO with children or n < 0 is SDRX_EINVAL; n == 0 does nothing. */
int sdrx_get_catchup(sdrx_ctx *ctx, const int *ids, int n, sdrx_meter *out);

/* Channel watch (option "watch" = 1): what tells a host WHEN to unpark.  A parked leaf does no work and so has no meter, no
 * squelch observation and no spectrum; the watch measures the stream the leaf CONSUMES instead -- one power spectrum per source
 * stream, shared by all the leaves it feeds -- and gives each watched leaf one number: the power inside the band that would
 * reach its output.  A leaf can be watched whether active or parked, and its figures do not depend on which.  The reference
 * has no counterpart (it runs every VFO always): this text is the definition.
 *
 * Source of a leaf: decimate[decimate_count] of its parent; for parent_id == -1 the raw frame exactly as sdrx_get_raw /
 * SDRX_SPECTRUM_RAW define it (after the byte LUT and the DC-bias removal on the device; for sdrx_process_device /
 * sdrx_submit_device the caller's device frame, read inside that frame's own launch sequence).  A source is measured in a frame
 * only while at least one of its leaves is watched.
 *
 * Per measured source and frame, n = the source's samples per frame, N = SDRX_SPECTRUM_BINS = 8192:
 *   S = min(max(n / N, 1), SDRX_WATCH_MAX_SEGMENTS) segments (integer division); segment s starts at sample s * (n / S) and
 *   takes min(N, n) samples, a stream shorter than N zero-padded as the spectrum display does;
 *   each segment: Hann window (the display's table) -> kiss_fft of N points, bit-identical to the display's ->
 *   P_s[i] = fl(fl(im*im) + fl(re*re)) in fp32, no contraction (the expression under the display's sqrtf);
 *   PSD[i] = sum over s, ascending, of (double)P_s[i];  i in kiss_fft's natural output order (i >= N/2: negative frequencies).
 * PSD is therefore bit-exact in every arithmetic, given the stream the device holds.
 *
 * Band of a leaf, computed on the host in IEEE double, recomputed when sdrx_set_mixer_freqs names the leaf.  The mixer
 * multiplies by exp(+j 2 pi f t) (oscillator.cpp:9-11, vfo.cpp:241): a component at g in the source lands at g + f in the leaf.
 * With f = mixer_freq_hz, fs = the leaf's fs, R = fs / 2^decimate_count:
 *   USB leaf:      R_out = R / late_decimate when late_decimate is 5 or 6, else R;  B = filter_bw_hz if > 0, else R_out / 2,
 *                  capped at R_out / 2;  [lo, hi] = [-f, -f + B]
 *   compress leaf: [lo, hi] = [-f - R/2, -f + R/2]
 *   k_lo = ceil(lo * 8192.0 / fs), k_hi = floor(hi * 8192.0 / fs), n_bins = clamp(k_hi - k_lo + 1, 1, 8192),
 *   first_bin = k_lo mod 8192 in [0, 8192)  (a mixer beyond +-fs/2 aliases, as the oscillator table does).
 *
 * Per watched leaf and frame: band_pwr = sum over j < n_bins of PSD[(first_bin + j) mod 8192], total_pwr = sum of PSD: doubles,
 * reduced in parallel -- every term is non-negative, so any order lies within n_terms * 2^-53 relative of the exact sum.
 *
 * sdrx_set_watch: batched and atomic, with the calling rules of sdrx_set_active -- the whole list is checked first: a bad or
 * duplicate id, the id of a VFO with children, on[k] not 0 or 1 or n < 0 is SDRX_EINVAL with nothing changed; n == 0 does
 * nothing; SDRX_ESTATE before sdrx_finalize, with the option off, and while submitted frames are undelivered.  Frames the
 * software pipeline of sdrx_process_device still holds finish with the old selection first.  The buffers are allocated by the
 * first call that switches a leaf on (as the spectrum's are); a leaf switched on is measured from the next frame on.
 * sdrx_get_watch: the figures of the last DELIVERED frame, with the calling rules of sdrx_get_meters; the records travel with
 * the frame's fixed-size part, so they can be read while the next frame is in flight.
 * sdrx_get_watch_psd: PSD of the source of watched leaf `leaf_id` after the last frame, with sdrx_get_spectrum's rules:
 * SDRX_ESTATE while frames are in flight (and before the first frame measured under the present selection of sources),
 * SDRX_EINVAL if the leaf is not watched.
 *
 * Latency: a carrier first seen in the figures of frame f can be heard from frame f + 1 at the earliest -- sdrx_set_active
 * needs every submitted frame delivered first, and the unparked leaf starts with empty filters.  With option "catchup" = 1 a
 * leaf with a parent, unparked before frame f + 1, starts on frame f itself: the stream the watch measured is still on the
 * device, and its payload of f is delivered in front of that of f + 1 (sdrx_get_catchup above). */
#define SDRX_WATCH_MAX_SEGMENTS 16
typedef struct sdrx_watch_level {
    int64_t frame;        /* frame of the source stream these figures were taken from */
    double band_pwr, total_pwr;
    int32_t first_bin, n_bins;
    int32_t segments;     /* S */
    int32_t watched;      /* 0: not watched in that frame -> the other fields but `frame`, first_bin, n_bins are 0 */
    int32_t reserved[2];  /* 0 (the record is 48 bytes) */
} sdrx_watch_level;
int sdrx_set_watch(sdrx_ctx *ctx, const int *ids, const int32_t *on, int n);
int sdrx_get_watch(sdrx_ctx *ctx, const int *ids, int n, sdrx_watch_level *out);
int sdrx_get_watch_psd(sdrx_ctx *ctx, int leaf_id, double *psd /* 8192, natural order */, int64_t *frame);

/* Drift estimate (part of option "watch" = 1; no option of its own): by how many Hz has the band moved?  The reference leaves
 * this loop to its user ("When changing dongles there may be a slight frequency difference ... mix_offset"); the actuator is
 * sdrx_set_mixer_freqs above, this is the sensor.  Per measured source and frame the PSD the watch has computed is registered
 * against a template of that source on the device, and the answer travels with the frame.  The reference has no counterpart:
 * this text is the definition.
 *
 * N = SDRX_SPECTRUM_BINS = 8192; PSD = the watch's PSD of the source for that frame; T = the source's template, N doubles, each
 * finite and >= 0; K = max_shift, 1 <= K <= SDRX_DRIFT_MAX_SHIFT.
 *   profile[s] = sum over i < N of T[i] * PSD[(i + s) mod N]      for s = -K .. K, in IEEE double
 *   shift      = the first maximum of the device's own profile, the shifts taken in the order 0, -1, +1, -2, +2, ...
 * Any summation order is allowed, with or without FMA.  The bound: every term is non-negative, so the exact sum E is the sum
 * of the terms' magnitudes, and N - 1 additions of rounded products (or N fused steps) in any order give a value within
 * ((1 + u)^N - 1) E <= (N + 1) u E of it, u = 2^-53 (Higham, Accuracy and Stability, 4.2, with the products' own rounding as
 * the N-th factor; (1 + u)^N - 1 < (N + 1) u for N u < 2^-39).  A model that rounds each product once and adds them exactly
 * (math.fsum) lies within 2 u E.  Device and model therefore differ by at most (N + 3) u E <= (N + 4) u * model, which is what
 * the tests allow.  An all-zero T gives profile = 0 and shift = 0.
 *
 * The record, 64 bytes, per source and frame -- written by the device to the fixed-size part of the frame the source stream
 * held, beside the watch records:
 *   frame     the frame the source stream held
 *   peak, left, right, zero      profile at shift, shift - 1, shift + 1 and 0; a neighbour outside [-K, K] is reported as 0
 *   shift, max_shift, measured, captured
 * A frame in which the source is not measured -- no leaf of it watched, or max_shift 0 -- has measured = 0, every other field
 * but `frame` 0, and costs no launch.
 *
 * What a host does with it (sdrx_host.hpp drift_bins / drift_hz, sdrreceiver_amd/drift.py; not the device):
 *   d_bins = shift + 0.5 * (left - right) / (left - 2 peak + right); plain shift when shift = +-K or the denominator is 0
 *   d_Hz   = d_bins * fs_source / N      (fs_source: the leaf's fs)
 * Sign: the mixer multiplies by exp(+j 2 pi f t); a band that appears D Hz higher in the source peaks at s = +D / binwidth, and
 * the correction moves every sub's mixer by -D -- what a mix_offset raised by D does.  The estimate is absolute since the
 * template was taken (a retune of the subs does not change the source's PSD): mix_offset = the offset at capture + D; there
 * is no loop gain to choose.
 *
 * sdrx_set_drift: `leaf_id` names the source the way sdrx_get_watch_psd does -- the source of that watched leaf; calling rules
 * and check order of sdrx_set_watch for a list of one.  SDRX_EINVAL with nothing changed for a leaf that is not watched, for
 * max_shift outside 0 .. SDRX_DRIFT_MAX_SHIFT, and for a template entry that is negative, NaN or Inf.
 *   max_shift == 0                  switches the source's drift off (templ is not read; the template stays)
 *   templ != NULL, max_shift > 0    uploads N doubles
 *   templ == NULL, max_shift > 0    capture: the PSD of the next frame in which the source is measured becomes the template,
 *                                   copied on the device.  That frame's record has captured = 1 and the correlation runs as
 *                                   always: shift = 0 and peak = sum of T^2
 * The template belongs to the source, not to the leaf: it survives retunes, parking, changes of the watched set and the moves
 * of the watch's buffers.  Nothing is allocated or launched until the first sdrx_set_drift that switches a source on: until
 * then device_bytes, the launches and every payload are those of the watch alone.
 * sdrx_get_drift: the record of the last DELIVERED frame for the source of leaf `leaf_id` (any leaf, watched or not), with the
 * calling rules of sdrx_get_watch for a list of one: readable while the next frame is in flight.
 * sdrx_get_drift_profile: the 2K + 1 values profile[-K .. K] after the last frame, with sdrx_get_watch_psd's rules: SDRX_ESTATE
 * while frames are in flight and before the first frame measured under the present setting, SDRX_EINVAL if the leaf is not
 * watched or its source's drift is off. */
#define SDRX_DRIFT_MAX_SHIFT 1024
typedef struct sdrx_drift_level {
    int64_t frame;
    double peak, left, right, zero;
    int32_t shift, max_shift;
    int32_t measured;     /* 0: not measured in that frame -> the other fields but `frame` are 0 */
    int32_t captured;     /* 1: this frame's PSD became the template */
    int32_t reserved[2];  /* 0 (the record is 64 bytes) */
} sdrx_drift_level;
int sdrx_set_drift(sdrx_ctx *ctx, int leaf_id, const double *templ /* 8192 or NULL */, int max_shift);
int sdrx_get_drift(sdrx_ctx *ctx, int leaf_id, sdrx_drift_level *out);
int sdrx_get_drift_profile(sdrx_ctx *ctx, int leaf_id, double *profile /* 2 max_shift + 1 */, int64_t *frame);

/* Band scan (part of option "watch" = 1; no option of its own, as the drift estimate): where are the carriers?  A watch band
 * is derived from a leaf's mixer frequency, so a carrier no leaf is tuned to is invisible to the watch, and a tree finalized
 * with spare parked leaves has nothing that tells it which frequency to assign.  (The reference leaves this to its user too:
 * "the FFT is quite slow so it is probably a good idea to determine the exact frequencies to use via other means".)  The scan
 * integrates a source's PSD over a few frames, folds it into cells, takes a noise floor as a rank statistic of the cells and
 * reports every run of cells above a ratio over that floor.  The reference has no counterpart: this text is the definition,
 * and the device's answer is bit for bit what it says on the PSD sdrx_get_watch_psd returns.
 *
 * N = SDRX_SPECTRUM_BINS = 8192; PSD = the watch's PSD of the source for that frame, natural order.
 * Settings per source, sdrx_scan_cfg, 32 bytes:
 *   cell_bins w       0 = scan off for this source; else a power of two 1 .. 256.  C = N / w cells, 32 .. 8192
 *   frames M          frames integrated per evaluation, 1 .. 65 536
 *   floor_permille q  0 .. 1000; the floor's rank is k = (q * (C - 1)) / 1000 (integer division)
 *   ratio_q8          power ratio x 256, 1 .. 2^32 - 1
 *   min_cells         shortest run reported, 1 .. C
 *   reserved[3]       must be 0
 * No default ratio_q8, floor_permille or cell width is offered: what a real front end needs has not been measured (as for
 * the squelch and AGC windows).
 *
 * Device state per source, kept from the first sdrx_set_scan that switches the source on, in one allocation that never moves:
 * ACC[N] doubles, count, and the cells, the hits and the record of the last completed evaluation.
 *
 * Per frame in which the source is measured and w > 0:
 *   1. Integration, IEEE double, one addition per bin: ACC[i] = count == 0 ? PSD[i] : ACC[i] + PSD[i]; then count += 1.
 *   2. count < M: the frame's record has complete = 0.  count == M: steps 3-7, then count = 0.
 *   3. Cells in display order: display bin b is natural bin (b + N/2) mod N, so cell 0 begins at -fs/2.  Cell c covers display
 *      bins c w .. c w + w - 1 (no cell straddles the wrap: w divides N/2).  cell[c] = the sum of its ACC values from left to
 *      right, ((a0 + a1) + a2) + ...  -- only additions, so contraction cannot matter.
 *   4. floor = the cell whose 64-bit pattern, read as an unsigned integer, is the k-th smallest of the C patterns (k 0-based,
 *      equal values each count).  For finite non-negative doubles this is the k-th smallest value; the pattern order makes the
 *      rule total for anything else.
 *   5. thr = fl(floor * (ratio_q8 / 256.0)) -- the quotient is exact: one rounding.  hot[c] = cell[c] > thr by the IEEE
 *      comparison: a NaN is not hot.
 *   6. A run is a maximal sequence of consecutive hot cells inside 0 .. C - 1.  There is NO wrap: a run touching cell C - 1 and
 *      one touching cell 0 are two runs.  A run of at least min_cells cells is a hit; hits are ordered by ascending first_cell.
 *      n_hits counts all of them; the first n_stored = min(n_hits, SDRX_SCAN_MAX_HITS) are stored.
 *   7. A hit, sdrx_scan_hit, 32 bytes: peak_cell = the lowest cell index among the run's largest cells, peak_pwr =
 *      cell[peak_cell]; both reserved fields 0.
 *
 * The record, sdrx_scan_level, 64 bytes, per source and frame -- written by the device to the fixed-size part of the frame the
 * source stream held, beside the watch and drift records.  `integrated` is the count behind step 1, `frames` is M, `n_hot` the
 * number of hot cells.  A frame with complete = 0 has floor = thr = 0 and n_hits = n_stored = n_hot = 0.  A frame in which the
 * source is not measured -- no leaf of it watched, or w = 0 -- has measured = 0 and every other field but `frame` 0; it costs
 * no launch and is NO observation: count and ACC stay as they are.
 *
 * What a host does with a hit (sdrx_host.hpp scan_hit_hz / scan_mixer_for / scan_unassigned, sdrreceiver_amd/scan.py; not the
 * device), fs = the source's rate (a leaf's fs), in IEEE double:
 *   lo   = (first_cell * w - N/2) * fs / N
 *   hi   = ((first_cell + n_cells) * w - 1 - N/2) * fs / N
 *   peak = (peak_cell * w + (w - 1) / 2.0 - N/2) * fs / N
 *   the integer mixer frequency that puts `hz` in the middle of a leaf's watch band: USB leaf rint(B/2 - hz), B as the watch
 *   defines it; compress() leaf rint(-hz)
 *   a hit is unassigned when [lo, hi] overlaps none of the given leaf bands [band_lo, band_hi] (closed intervals, Hz)
 * The loop: scan -> unassigned -> mixer_for -> sdrx_set_mixer_freqs -> sdrx_set_active (with "catchup": the woken leaf hears
 * the frame the scan completed on).
 *
 * sdrx_set_scan: `leaf_id` names the source the way sdrx_set_drift does; its calling rules and check order.  cfg == NULL or
 * cell_bins == 0 switches the source's scan off (the state stays allocated).  SDRX_EINVAL with nothing changed for a leaf that
 * is not watched, a field outside the table above, or a non-zero reserved field.  Every accepted call with w > 0 restarts the
 * integration (count = 0).  A retune of the source's own VFO does not: the host calls sdrx_set_scan again if it wants that.
 * Nothing is allocated or launched until the first sdrx_set_scan that switches a source on: until then device_bytes, the
 * launches and every payload are those of the watch alone, or of the watch with drift.  A spectrum, a catch-up or the drift
 * estimate neither reads nor changes the scan's state; scan and drift on one source each give what they give alone.
 * sdrx_get_scan: the record of the last DELIVERED frame, with the rules of sdrx_get_drift: any leaf of the source, watched or
 * not, readable while the next frame is in flight.
 * sdrx_get_scan_hits: the stored hits of the last COMPLETED evaluation and the frame it completed on, with the rules of
 * sdrx_get_drift_profile: SDRX_ESTATE while frames are in flight and before the first evaluation completed under the present
 * setting, SDRX_EINVAL if the leaf is not watched or its source's scan is off.  *n = min(n_stored, max_hits).
 * sdrx_get_scan_cells: cell[0 .. C - 1] of that evaluation, with the same rules. */
#define SDRX_SCAN_MAX_HITS 512
typedef struct sdrx_scan_cfg {
    int32_t cell_bins;       /* w: 0 off, else a power of two 1 .. 256 */
    int32_t frames;          /* M: 1 .. 65 536 */
    int32_t floor_permille;  /* q: 0 .. 1000 */
    uint32_t ratio_q8;       /* >= 1 */
    int32_t min_cells;       /* 1 .. C */
    int32_t reserved[3];     /* 0 */
} sdrx_scan_cfg;
typedef struct sdrx_scan_hit {
    int32_t first_cell, n_cells, peak_cell, reserved;
    double peak_pwr;
    double reserved_d;
} sdrx_scan_hit;
typedef struct sdrx_scan_level {
    int64_t frame;
    double floor, thr;
    int32_t n_hits, n_stored, n_hot;
    int32_t integrated;      /* count behind step 1 */
    int32_t frames;          /* M */
    int32_t cell_bins;
    int32_t measured;        /* 0: not measured in that frame -> the other fields but `frame` are 0 */
    int32_t complete;        /* 1: this frame completed an evaluation */
    int32_t reserved[2];     /* 0 (the record is 64 bytes) */
} sdrx_scan_level;
int sdrx_set_scan(sdrx_ctx *ctx, int leaf_id, const sdrx_scan_cfg *cfg);
int sdrx_get_scan(sdrx_ctx *ctx, int leaf_id, sdrx_scan_level *out);
int sdrx_get_scan_hits(sdrx_ctx *ctx, int leaf_id, sdrx_scan_hit *hits, int max_hits, int *n, int64_t *frame);
int sdrx_get_scan_cells(sdrx_ctx *ctx, int leaf_id, double *cells /* C */, int64_t *frame);

/* Device-side wake (option "wake" = 1): the watch decides on the device, for frame f from the source's spectrum of frame f,
 * whether a leaf runs in frame f -- no host between two frames, in every launch form (sdrx_process*, frames in flight through
 * sdrx_submit*, frames queued with sdrx_process_device), parent-less leaves included.  The reference has no counterpart: this
 * text is the definition.  No default threshold, contrast or hold time is offered (the stance of the squelch, the AGC and the
 * scan).
 *
 * Per controlled leaf the device keeps hold_left, 0 after every sdrx_set_wake that names the leaf.  THE RULE runs for every frame
 * f the context processes, for every controlled leaf, on the leaf's own watch record of frame f -- b = band_pwr, t = total_pwr,
 * n = n_bins, N = 8192 -- in IEEE double, one rounding per operation, no contraction:
 *     c_ok = contrast_q8 == 0
 *            || (n < N && fl(b * (double)(256 * (N - n))) >= fl(fl(t - b) * (double)((uint64)contrast_q8 * n)))
 *     hot  = b >= min_band_pwr && c_ok               (a NaN is not hot; both integer factors are exact in double)
 *     hot:                 hold_left = hold_frames;  active(f) = 1
 *     else if hold_left>0: hold_left -= 1;           active(f) = 1
 *     else:                                          active(f) = 0
 * c_ok is `contrast >= contrast_q8 / 256` (contrast: the band's power density over the density outside it) without the
 * division.  The decision is bit for bit this rule applied to the figures sdrx_get_watch reports for that leaf and frame;
 * band_pwr itself keeps its summation bound ("Channel watch" above).
 *
 * A leaf with active(f) = 1 that was parked in f-1 is a new vfo from frame f on, as an unparked leaf in "Parking" without
 * catch-up: the oscillator starts fresh at sample 0 of frame f, every state region is zero, the gate state is that of
 * sdrx_finalize (hang_left 0, prev_open 1, no floor observation), the AGC's quiet_run is 0; the gain and the mixer are what the
 * device holds.  No oscillator replay: a wake does not change the frequency, the checkpoints stand.  A leaf with active(f) = 0
 * is parked in f exactly as "Parking" defines a parked frame; a leaf that stays active continues.  Control starts with the
 * next frame: an active leaf with a cold band is parked by it.
 *
 * Whether a controlled leaf ran in a frame is a device result: sdrx_get_output / sdrx_get_preroll length 0 and no callback,
 * SDRX_ENOSTREAM from sdrx_get_stream / sdrx_get_prequant, the zero meter, n_open without "squelch" and sdrx_get_active answer
 * from the wake record of that frame.  The record travels with the fixed-size part of the frame, beside the watch records.
 *
 * sdrx_set_wake is batched and atomic, with the calling rules and check order of sdrx_set_agc (between frames; the software
 * pipeline drains first).  SDRX_EINVAL with nothing changed: a leaf that is not watched; a leaf with an enabled spectrum; `on`
 * not 0 or 1; a non-finite or negative min_band_pwr; a non-zero reserved word.  on = 0 releases the leaf: it stays in the state
 * its last frame ran in, and sdrx_set_active works on it again.  While a leaf is controlled, sdrx_set_active,
 * sdrx_set_watch(.., 0) and sdrx_set_spectrum(id, 1) on it are SDRX_EINVAL with nothing changed; sdrx_set_mixer_freqs (the watch
 * band follows), sdrx_set_gains, sdrx_set_squelch*, sdrx_set_agc and the taps keep working.  "catchup" composes: it concerns
 * only leaves the host unparks.  sdrx_get_wake has the calling rules of sdrx_get_watch. */
typedef struct sdrx_wake_cfg {   /* 32 bytes */
    double   min_band_pwr;       /* finite, >= 0: units of sdrx_watch_level.band_pwr */
    uint32_t contrast_q8;        /* 0: no contrast condition; else density ratio x 256 */
    uint32_t hold_frames;        /* frames a leaf stays active after the last hot one */
    uint32_t on;                 /* 0 | 1: 1 puts the leaf under the device's control */
    uint32_t reserved[3];        /* must be 0 */
} sdrx_wake_cfg;
typedef struct sdrx_wake_state { /* 32 bytes */
    int64_t  frame;
    int64_t  since_frame;        /* first frame of the present state */
    int32_t  active;             /* the state frame `frame` ran in */
    int32_t  hot;
    uint32_t hold_left;          /* behind the rule */
    int32_t  controlled;         /* 0: not under control in that frame -> active / since_frame from the host's bookkeeping, the rest 0 */
} sdrx_wake_state;
int sdrx_set_wake(sdrx_ctx *ctx, const int *ids, const sdrx_wake_cfg *cfgs, int n);
int sdrx_get_wake(sdrx_ctx *ctx, const int *ids, int n, sdrx_wake_state *out);

/* ---- ADC meter (option "adc_meter" = 1, set before sdrx_finalize) ---------------------------------------------
 * Every meter above sits behind the chain, on leaf payloads.  This one looks at what the front end delivers: with the option on,
 * every frame that reaches the context AS INTEGER SAMPLES -- sdrx_process_u8 / sdrx_submit_u8, the *_fmt calls for host and for
 * device frames, and the group's *_u8 / *_fmt calls -- gets one record of exact integer statistics of those samples as they
 * arrived: before the conversion to float and before the DC-bias removal (correct_dc changes nothing in it).  The record is
 * computed on the device (one launch per frame, in front of the conversion) and travels with the frame's fixed-size part.
 *
 * The integer code v of a component:
 *   SDRX_FMT_CU8   b - 127, in [-127, 128]; the rails are the bytes 0 and 255
 *   SDRX_FMT_CS8   the int8, in [-128, 127]
 *   SDRX_FMT_CS16  the int16 ITSELF -- not scaled by 2^-8 --, in [-32768, 32767]
 * "At a rail": equal to the format's lowest or highest code.  Multiply CS16 figures by 2^-8 (sums) or 2^-16 (sums of squares and
 * of products) for the chain's units, "dongle LSB"; the 8-bit formats are in those units already.
 *
 * Everything is an exact integer and fits its type: a frame is at most one second long and n_complex < 2^31, so
 * sum_sq <= n_complex * 2^30 < 2^61, |sum| and |sum_iq| likewise, and every count is at most 2 n_complex < 2^32.  The device's
 * answer is therefore bit for bit a plain integer model of the definitions below; there is no tolerance.
 *
 * sdrx_get_adc_meter answers for the last DELIVERED frame, the one sdrx_get_output serves, and is readable while the next frame
 * is in flight; frames queued with sdrx_process_device_fmt are brought over first (as for sdrx_get_meters).  A cf32 frame
 * (sdrx_process, sdrx_submit, sdrx_process_device, sdrx_submit_device) and a shared frame (sdrx_*_shared, sdrx_*_if_same) did
 * not arrive here as ADC samples: the record then has that frame's `frame`, measured = 0, fmt = -1 and zeros elsewhere, and
 * nothing was launched for it.  SDRX_ESTATE with the option off, before sdrx_finalize or before any frame was delivered;
 * SDRX_EINVAL for a NULL `out` (checked in this order, as the per-leaf calls do).  With the option off nothing changes at all:
 * the same kernels, launches, device_bytes, payloads and callbacks.  The launch is not one of sdrx_get_kernel_times' kinds. */
typedef struct sdrx_adc_arm {    /* 40 bytes: one component (I or Q) of the frame */
    int64_t  sum;                /* sum of v */
    uint64_t sum_sq;             /* sum of v*v */
    int32_t  min, max;           /* smallest / largest v */
    uint32_t at_lo, at_hi;       /* components equal to the lowest / highest code */
    uint32_t longest_rail_run;   /* longest run of CONSECUTIVE samples of this arm that are each at a rail (either one) */
    uint32_t reserved;
} sdrx_adc_arm;
typedef struct sdrx_adc_meter {  /* 184 bytes */
    int64_t  frame;              /* as sdrx_meter.frame */
    uint32_t n_complex;
    int32_t  fmt;                /* SDRX_FMT_* of that frame; -1 if not measured */
    uint32_t measured;           /* 0: the frame did not arrive here as integer samples; everything below is 0 */
    uint32_t reserved;
    sdrx_adc_arm i, q;
    int64_t  sum_iq;             /* sum of vI * vQ */
    uint32_t bits[17];           /* bits[k]: components, I and Q together, with bit_length(|v|) == k (0 for v = 0, 16 for -32768); sums to 2 n_complex */
    uint32_t reserved2;
} sdrx_adc_meter;
int sdrx_get_adc_meter(sdrx_ctx *ctx, sdrx_adc_meter *out);

/* ---- Resampler (sdrx_set_resampler before sdrx_finalize) ---------------------------------------------------------
 * A tree can only halve, and end in /5 or /6: its root rate is 48 kHz or 12 kHz times a power of two, times 1, 5 or 6.  A front
 * end with a fixed master clock -- Airspy R2 at 10 and 2.5 MS/s, Airspy Mini at 6 and 3 MS/s, an RTL dongle at 2.4 or 2.048 MS/s
 * -- delivers another rate.  With a resampler set, the frames handed to the context are at the front end's rate fs_in, and one
 * more kernel, a polyphase rational resampler L/M behind the ingest kernels, makes the tree's raw frame from them.  The
 * reference has no counterpart: this text is the definition.  Off (the default) nothing changes at all: the same kernels,
 * launches, device_bytes, payloads and callbacks.
 *
 * Ratio and frame lengths.  fs_out is the fs of the parent-less VFOs and n their samples_per_buffer.  With g = gcd(fs_in, fs_out):
 * L = fs_out / g, M = fs_in / g, and the incoming frame has n_in = n M / L samples.  Required, else SDRX_EUNSUPPORTED at
 * sdrx_finalize with the reason in sdrx_last_error:
 *   n M % L == 0, so that every frame starts at phase 0;   n_in % 16 == 0 (the DC and ADC-meter kernels);   n_in >= taps_per_phase;
 *   L <= 1024;   1/2 <= M / L <= 4;   taps_per_phase T a multiple of 4 in 8 .. 64;   L T <= 32768;
 *   all parent-less VFOs have one fs and one frame length.
 *
 * Filter arithmetic.  The prototype is h[k], k < L T, fp32.  x_f[j] is frame f's cf32 input at the input rate: after the format
 * conversion and, if asked for, after the DC-bias removal (in that order: the removal keeps the |x| <= 128 bound it is proved
 * for).  For j < 0, x_f[j] := x_{f-1}[n_in + j], zero for the first frame after sdrx_finalize.  For output m in [0, n):
 *   p = m M in 64 bits, i = p div L, ph = p mod L, and separately for re and im
 *   acc_0 = +0.0f;  acc_{t+1} = fl(acc_t + fl(h[ph + t L] * x[i - t])), t = 0 .. T-1 ascending;  y[m] = acc_T
 * -- two roundings per tap, no FMA, the same in all three settings of option "exact".  y is the tree's raw frame.  The group
 * delay is (L T - 1) / (2 M) output samples.
 *
 * The built-in design (sdrx_resampler_design; host only, IEEE double, rounded once to fp32).  With N = L T and A = atten_db,
 * 50 < A <= 120 (SDRX_EINVAL otherwise):
 *   beta = 0.1102 (A - 8.7);   tw = (A - 7.95) / (2.285 (N - 1) 2 pi);   fn = 0.5 / max(L, M);   fc = fn - tw / 2
 *   h[k] = L * 2 fc * sinc(2 fc (k - (N-1)/2)) * I0(beta sqrt(1 - (2k/(N-1) - 1)^2)) / I0(beta),   sinc(x) = sin(pi x) / (pi x)
 * SDRX_EFILTER if fn - tw <= 0: the transition is wider than the band (5/3 with T = 8).  The stop band starts at the lower
 * Nyquist rate, so nothing aliases into the pass band, which is (fn - tw) L fs_in Hz wide.
 *
 * sdrx_resampler_design needs no context and no device: the ratio rules above (SDRX_EUNSUPPORTED), then the design into `taps`
 * (L T floats, prototype order; NULL: only `info`; SDRX_EINVAL if cap < L T).  in_frame and out_frame of `info` are 0.
 * sdrx_set_resampler: before sdrx_finalize (SDRX_ESTATE after it) and after the first parent-less VFO was added (SDRX_ESTATE
 * before: its fs is fs_out, which says how many taps L T the call copies from `taps` -- the caller's own, so a test can craft
 * them; passband_hz of the info is then 0).  fs_in = 0 switches the resampler off again.
 * sdrx_get_resampler: the info (in_frame and out_frame once finalized) and up to `cap` taps in prototype order (`taps` may be
 * NULL); SDRX_ESTATE without a resampler.
 * sdrx_get_resampler_input: the staged input-rate frame x_f of the last frame in natural order, under sdrx_get_raw's rules
 * (and after caller-owned device frames too: the staging buffer is the context's).
 *
 * With a resampler set every frame call of the context -- sdrx_process, _u8, _fmt, _device*, their submit forms, cf32 and integer
 * frames alike -- takes n_complex == in_frame; a frame of out_frame samples is SDRX_EINVAL.  sdrx_get_raw, the raw spectrum and
 * the raw watch see the resampled frame (sdrx_get_raw also after sdrx_process_device); the ADC meter sees the in_frame samples
 * as they arrived.  Dongle bytes without DC removal take the conversion pass too.  sdrx_*_shared and sdrx_*_if_same return
 * SDRX_ESTATE if either context resamples.  Groups do not offer it. */
typedef struct sdrx_resampler_info { /* 48 bytes */
    int32_t fs_in, fs_out, L, M, taps_per_phase, in_frame, out_frame, reserved;
    double delay_out_samples, passband_hz;
} sdrx_resampler_info;
int sdrx_resampler_design(int32_t fs_in, int32_t fs_out, int32_t taps_per_phase, double atten_db, float *taps, int32_t cap,
                          sdrx_resampler_info *info);
int sdrx_set_resampler(sdrx_ctx *ctx, int32_t fs_in, const float *taps, int32_t taps_per_phase);
int sdrx_get_resampler(sdrx_ctx *ctx, sdrx_resampler_info *info, float *taps, int32_t cap);
int sdrx_get_resampler_input(sdrx_ctx *ctx, float *out_iq, int32_t cap_complex);

/* ---- Front stage (sdrx_set_front before sdrx_finalize) -----------------------------------------------------------
 * 1 .. 3 half-band decimations by 2 between the ingest kernels and the resampler -- or level 0 where no resampler is set.  Two
 * kinds of front end need it: one that delivers REAL samples of an IF (Airspy R2 / Mini: 20, 12, 10, 6 MS/s real), which the
 * first stage turns into I/Q on the device (fs/4 translation, half-band, decimation by 2) from 2 bytes a sample, and one whose
 * rate is more than 4 times the tree's, which a stage in front brings into the resampler's 1/2 <= M/L <= 4.  The reference has
 * no counterpart: this text is the definition.  Off (the default) nothing changes at all: the same kernels, launches,
 * device_bytes, payloads and callbacks.
 *
 * sdrx_set_front(ctx, real_input, stages, taps, K, atten_db): before sdrx_finalize (SDRX_ESTATE after it) and after the first
 * parent-less VFO was added (SDRX_ESTATE before), before or after sdrx_set_resampler.  stages in 1 .. 3, real_input 0 or 1,
 * 2 <= K <= 31, else SDRX_EINVAL.  One prototype h[0 .. N-1], N = 4 K + 3, centre C = 2 K + 1, serves every stage; h[k] must
 * be +0.0f (that bit pattern) for every odd k != C, else SDRX_EINVAL; symmetry is not required.  taps == NULL: the built-in
 * design below at `atten_db`, which is not read otherwise.  stages == 0 switches the stage off again.
 *
 * Frame lengths.  n0 is the frame the stage feeds: the resampler's in_frame if one is set, else the parent-less VFOs' frame.
 * Stage s (s = stages .. 1; stage 1 reads the caller's samples) has n0 2^(stages - s) outputs and twice as many inputs.  Every
 * frame call of the context -- *_fmt, cf32, host and device frames -- takes in_frame = n0 2^stages samples; for the real formats
 * the count argument counts REAL samples.  Any other count is SDRX_EINVAL.  SDRX_EUNSUPPORTED at sdrx_finalize, with the reason
 * in sdrx_last_error, if the parent-less VFOs do not share one fs and one frame.  With a resampler, fs_in of
 * sdrx_set_resampler stays the rate at the RESAMPLER's input: the front end's rate over 2^stages.
 *
 * A stage with input z and output y.
 *   Complex stage: z[n] is the stage's cf32 input; in stage 1 the format conversion, after the DC-bias removal if asked for.
 *   Real stage (stage 1 with real_input = 1 only): r[n] is the converted real sample, n counted from the start of the frame,
 *     and z[n] = r[n] (-j)^n: Re z = +r, 0, -r, 0 and Im z = 0, -r, 0, +r for n mod 4 = 0, 1, 2, 3 (-r is the negation: -0.0f
 *     for r = +0.0f).  in_frame is a multiple of 4, so the pattern runs on across frames.  The band [0, fs_r / 2] comes out as
 *     [-fs_r / 4, +fs_r / 4]: the tuned centre is fs_r / 4.
 *   History: z[n] := z_prev_frame[n_in_stage + n] for n < 0, zero before the first frame.  Every stage keeps its own.
 *   Output y[m], separately for re and im: acc = +0.0f; acc = fl(acc + fl(h[k] z[2m - k])) over the structurally non-zero k in
 *     ascending order, k = 0, 2, .. 2K, 2K+1, 2K+2, .. 4K+2 -- two roundings per tap, no FMA, the same in all three settings of
 *     option "exact".  Real stage: the products whose z component is structurally zero are not formed -- I sums the even k only
 *     (2K + 2 products), Q is the single product fl(h[C] Im z[2m - C]).
 *
 * Real formats, valid only on a context whose front stage has real_input = 1; on such a context the complex formats and cf32
 * frames are SDRX_EINVAL, and correct_dc != 0 is SDRX_EINVAL (DC lands at the edge of the output band, where the stages behind
 * discard it):
 *   SDRX_FMT_RS16 = 3   native-endian int16, real                    x = (float)v * 2^-8                      [-128, 128)
 *   SDRX_FMT_RU12 = 4   uint16 holding a 12-bit offset code, real    x = (float)((v & 4095) - 2048) * 2^-4    [-128, 128)
 * One fixed scale, as for the complex formats.  The half-band has unit DC gain, so a real sine of amplitude a arrives as a
 * complex tone of magnitude a / 2; a caller who wants a passes the doubled taps, which is exact in fp32.
 * The ADC meter records a real frame as the same memory read as pairs -- even samples in arm I, odd samples in arm Q,
 * n_complex = in_frame / 2 -- with fmt the real format; the integer code is the int16 itself (RS16) or (v & 4095) - 2048 (RU12,
 * rails -2048 and 2047).
 *
 * The built-in design (sdrx_front_design; host only, IEEE double rounded once to fp32).  With A = atten_db, 50 < A <= 120
 * (SDRX_EINVAL otherwise):
 *   beta = 0.1102 (A - 8.7);   tw = (A - 7.95) / (2.285 (N - 1) 2 pi), a fraction of the stage's input rate
 *   h[k] = 0.5 sinc(0.5 (k - C)) I0(beta sqrt(1 - (2k/(N-1) - 1)^2)) / I0(beta),   sinc(x) = sin(pi x) / (pi x)
 * with the odd k != C set to +0.0 exactly.  SDRX_EFILTER if 0.25 - tw / 2 <= 0 (K = 2 at A = 80).  `taps`: N floats (NULL: only
 * `info`; SDRX_EINVAL if cap < N).  `info` carries N, tw and the alias-free share of the output band, 1 - 2 tw.
 *
 * sdrx_get_front: the info (in_frame and out_frame once finalized; tw and alias_free 0 for the caller's own taps) and up to `cap`
 * taps (`taps` may be NULL); SDRX_ESTATE without a front stage.  With no resampler the last stage's output is the raw frame
 * (sdrx_get_raw, raw spectrum, raw watch); with one it is what sdrx_get_resampler_input serves.  sdrx_*_shared and sdrx_*_if_same
 * return SDRX_ESTATE if either context has a front stage.  Groups do not offer it. */
#define SDRX_FMT_RS16 3
#define SDRX_FMT_RU12 4
typedef struct sdrx_front_info { /* 48 bytes */
    int32_t real_input, stages, K, N, in_frame, out_frame, reserved[2];
    double tw, alias_free;
} sdrx_front_info;
int sdrx_front_design(int32_t K, double atten_db, float *taps, int32_t cap, sdrx_front_info *info);
int sdrx_set_front(sdrx_ctx *ctx, int32_t real_input, int32_t stages, const float *taps, int32_t K, double atten_db);
int sdrx_get_front(sdrx_ctx *ctx, sdrx_front_info *info, float *taps, int32_t cap);

/* ---- Impulse blanker (sdrx_set_blanker before sdrx_finalize) -----------------------------------------------------
 * Zeroes short, strong pulses (radar, ignition, a switching supply, a USB dropout) in the wideband frame, behind the format
 * conversion and the DC-bias removal and in front of the front stage, the resampler or level 0: one pass over the frame instead
 * of a pulse ringing in every channel.  The reference has no counterpart: this text is the definition, sdrreceiver_amd/blank.py
 * restates it in numpy, and the device is held to that bit for bit.  Off (the default) nothing changes at all: the same kernels,
 * launches, device_bytes, payloads and callbacks.
 *
 * Settings (sdrx_blanker_cfg; anything else is SDRX_EINVAL, there are no defaults):
 *   ratio      fp32, finite, >= 1: a hit is a power above ratio times the reference
 *   floor      fp32, finite, >= 0: ... and above this, in chain units squared
 *   rank_q16   1 .. 65536: the reference is this rank of the previous frame's powers (32768: the median)
 *   guard      G in 0 .. 64: samples blanked on either side of a hit
 *
 * Frame f, x its n cf32 samples as they reach the stage.  State: ref_bin (-1 after sdrx_finalize), tail_gap (G_max + 1 = 65 after
 * sdrx_finalize: no carry), last_blank (0).
 *   1. p[j] = fl(fl(re re) + fl(im im)): three roundings, no FMA, in every setting of option "exact".
 *   2. bin(p) = (bits(p) & 0x7fffffff) >> 20, 0 .. 2047: an eighth of an octave of power; +inf is bin 2040.  edge(b) is the float
 *      whose bits are b << 20.
 *   3. thr = +inf if ref_bin < 0, else max(fl(ratio edge(ref_bin)), floor) -- from the settings current at this frame.
 *   4. hit[j] = p[j] > thr (IEEE: a NaN power is no hit).
 *   5. blank[j] = some hit[m] of this frame with |m - j| <= G, or j <= G - 1 - tail_gap.  Lookahead stops at the frame's end.  A
 *      blanked sample becomes (+0.0f, +0.0f); every other keeps its bits.
 *   6. h[bin(p[j])] over all n samples as they arrived; next_ref_bin = min(2040, the smallest b with 65536 (h[0] + .. + h[b]) >=
 *      rank_q16 n), in 64-bit unsigned; it is ref_bin of frame f + 1.
 *   7. tail_gap of frame f + 1 = min(65, n - 1 - the last hit's index), 65 without a hit; last_blank = blank[n - 1].
 * The record of frame f: thr_bits, ref_bin (the one used), next_ref_bin; hits, blanked = the j with hit, with blank; runs = the j
 * with blank[j] and not blank[j - 1], blank[-1] being last_blank; carry_in = the j with j <= G - 1 - tail_gap.
 *
 * sdrx_set_blanker(ctx, cfg): before sdrx_finalize it switches the stage on (cfg == NULL: off again).  After sdrx_finalize it
 * changes the four settings between two frames (SDRX_ESTATE with submitted frames not yet delivered; the calls in flight are
 * drained first); SDRX_ESTATE if the stage was not on at sdrx_finalize, or for cfg == NULL.  The state stays: the next frame uses
 * the old ref_bin and tail_gap under the new settings.
 * sdrx_get_blanker(ctx, cfg_out, record_out): the settings the last delivered frame ran with and its record (either may be NULL),
 * under sdrx_get_adc_meter's rules.  sdrx_get_blanker_input(ctx, out_iq, cap): the last frame handed over as it reached the
 * stage, natural order, up to cap samples, under sdrx_get_resampler_input's rules.
 * in_frame is unchanged.  sdrx_get_raw, the raw spectrum and the raw watch see the blanked frame (behind a resampler or a front
 * stage: what those make of it); the ADC meter sees the samples as they arrived.  SDRX_EUNSUPPORTED at sdrx_finalize with a real
 * first front stage (it reads the caller's words itself: there is no complex frame in front of it).  sdrx_*_shared and
 * sdrx_*_if_same return SDRX_ESTATE if either context blanks.  Groups do not offer it. */
typedef struct sdrx_blanker_cfg { /* 32 bytes */
    float ratio, floor;
    int32_t rank_q16, guard;
    int32_t reserved[4];
} sdrx_blanker_cfg;
typedef struct sdrx_blanker_record { /* 64 bytes */
    int64_t frame;
    uint32_t n_complex, measured;
    uint32_t thr_bits;
    int32_t ref_bin, next_ref_bin;
    uint32_t hits, blanked, runs, carry_in;
    uint32_t reserved[5];
} sdrx_blanker_record;
int sdrx_set_blanker(sdrx_ctx *ctx, const sdrx_blanker_cfg *cfg);
int sdrx_get_blanker(sdrx_ctx *ctx, sdrx_blanker_cfg *cfg_out, sdrx_blanker_record *record_out);
int sdrx_get_blanker_input(sdrx_ctx *ctx, float *out_iq, int32_t cap_complex);

/* ---- IQ balance (sdrx_set_iq_balance before sdrx_finalize) ---------------------------------------------------------
 * Cancels the image a direct-conversion front end (SDRX_FMT_CS8, SDRX_FMT_CS16) puts at the mirror frequency of every carrier: with
 * 5 % gain error and 3 degrees phase error about 29 dB down, in someone else's channel.  One elementwise pass over the wideband
 * frame, in place, behind the format conversion and the DC-bias removal and in front of the blanker, the front stage, the
 * resampler or level 0; cf32 frames pass through it as well.  The reference has no counterpart: this text is the definition,
 * sdrreceiver_amd/iqbal.py restates it in numpy, and the device is held to that bit for bit.  No FMA anywhere; the same in every
 * setting of option "exact".  Off (the default) nothing changes at all: the same kernels, launches, device_bytes, payloads and
 * callbacks.
 *
 * Settings (sdrx_iq_cfg; anything else is SDRX_EINVAL, there are no defaults):
 *   mu         fp32, 0 <= mu <= 1: the step; 0 means hold -- apply, measure, never move
 *   min_power  fp32, finite, >= 0, chain units squared: a frame with less variance in I and Q together is not measured
 *   c0         fp32, |c0| <= 0.5
 *   d0         fp32, 0.5 <= d0 <= 2
 *   flags      bit 0 SDRX_IQ_LOAD; the other bits 0
 *   reserved   zeros
 *
 * State: c and d, fp32.  After sdrx_finalize they are c0 and d0.
 * Frame f of n samples (I, Q) as they reach the stage:
 *   1. Apply.  I' = I, bits kept.  Q' = fl(fl(c I) + fl(d Q)): three fp32 roundings.  (At c = 0, d = 1 a -0.0f in Q may become
 *      +0.0f: fl(0 I) + (-0) is +0 for I >= 0.  A non-finite I makes Q' NaN, at c = 0 too: 0 inf is NaN.  A Q' that is a NaN is the
 *      quiet NaN 0x7fc00000, whatever produced it: sign and payload of a generated NaN differ between processors.)
 *   2. Quantise the output, for the statistics only.  v = fl(x 256), which is exact; q(x) = 0 for a NaN, else v rounded to the
 *      nearest integer, ties to even, saturated to +-32767.
 *   3. Exact integer sums over the n samples of the frame, of qi = q(I') and qq = q(Q'): S_i, S_q, S_iq = sum qi qq (int64); S_ii,
 *      S_qq (uint64).  Tile padding is not in them.  With n < 2^31 everything is below 2^61.
 *   4. Step.  Every operation is one IEEE double operation, in this order:
 *        N = (double)n;  mi = (double)S_i / N;  mq = (double)S_q / N
 *        A = (double)S_ii / N - mi mi;  B = (double)S_qq / N - mq mq;  C = (double)S_iq / N - mi mq
 *        measured = A > 0 && B > 0 && (A + B) 2^-16 >= (double)min_power
 *      If measured and mu > 0:
 *        ep = C / A;  eg = (A - B) / (A + B);  g = 1 + mu eg
 *        c_next = (float)(g ((double)c - mu ep));  d_next = (float)(g (double)d)
 *      If either is not finite, or |c_next| > 0.5, or d_next is outside [0.5, 2], the old pair stays and rejected = 1; otherwise
 *      the pair is the state of frame f + 1 and adapted = 1.  No square root, nothing transcendental.
 * The record of frame f (sdrx_iq_record): measured, adapted, rejected; c_bits, d_bits -- the pair the frame used; next_c_bits,
 * next_d_bits -- the pair of frame f + 1; the five sums.
 *
 * sdrx_set_iq_balance(ctx, cfg): before sdrx_finalize it switches the stage on (cfg == NULL: off again).  After sdrx_finalize it
 * changes mu and min_power between two frames (SDRX_ESTATE with submitted frames not yet delivered; the calls in flight are
 * drained first); SDRX_ESTATE if the stage was not on at sdrx_finalize, or for cfg == NULL.  With SDRX_IQ_LOAD it also writes c0,
 * d0 into the device state in stream order -- a bench calibration, loaded and (mu = 0) held; without the flag the state stays and
 * c0, d0 are only checked.
 * sdrx_get_iq_balance(ctx, cfg_out, record_out): the settings the last delivered frame ran with (c0, d0: what sdrx_finalize or the
 * last SDRX_IQ_LOAD wrote) and its record (either may be NULL), under sdrx_get_blanker's rules.
 * in_frame is unchanged.  sdrx_get_blanker_input, sdrx_get_resampler_input and sdrx_get_raw see the corrected frame (or what the
 * stages behind make of it); the ADC meter sees the samples as they arrived.  SDRX_EUNSUPPORTED at sdrx_finalize with a real first
 * front stage (there is no complex frame in front of it, and I/Q made digitally has no imbalance).  sdrx_*_shared and
 * sdrx_*_if_same return SDRX_ESTATE if either context has the stage.  Groups do not offer it. */
#define SDRX_IQ_LOAD 1u
typedef struct sdrx_iq_cfg { /* 32 bytes */
    float mu, min_power, c0, d0;
    uint32_t flags;
    uint32_t reserved[3];
} sdrx_iq_cfg;
typedef struct sdrx_iq_record { /* 96 bytes */
    int64_t frame;
    uint32_t n_complex, measured;
    uint32_t adapted, rejected;
    uint32_t c_bits, d_bits;
    uint32_t next_c_bits, next_d_bits;
    int64_t sum_i, sum_q, sum_iq;
    uint64_t sum_ii, sum_qq;
    uint32_t reserved[4];
} sdrx_iq_record;
int sdrx_set_iq_balance(sdrx_ctx *ctx, const sdrx_iq_cfg *cfg);
int sdrx_get_iq_balance(sdrx_ctx *ctx, sdrx_iq_cfg *cfg_out, sdrx_iq_record *record_out);

/* ---- Frequency shift (sdrx_set_shift before sdrx_finalize) -----------------------------------------------------------
 * The reference's mix_offset ("tune ALL VFO's up or down by a number of Hz", after a dongle change or while the dongle warms up)
 * as one stage: one elementwise complex mix over the wideband frame, once instead of once per VFO, phase-continuous across frames
 * and across changes of the shift.  It is the last stage of the ingest chain: in place on the tree's raw frame, behind the
 * resampler or whatever comes last, in front of the raw-frame spectrum, the watch and level 0, at the tree's rate -- its Hz are
 * mix_offset's Hz.  This text is the definition, sdrreceiver_amd/shift.py restates it in numpy, and the device is held to that bit
 * for bit.  No FMA anywhere; the same in every setting of option "exact".  Off (the default) nothing changes at all: the same
 * kernels, launches, device_bytes, payloads and callbacks.
 *
 * State: phase and inc, uint32.  One unit of phase is 2^-32 turn, so inc is the shift in units of fs_tree / 2^32 per sample.  A
 * positive inc moves the spectrum up: the mixer's own sign convention, multiplication by exp(+j 2 pi f t).  After sdrx_finalize
 * they are phase0 and inc of the settings.
 * Tables: three of 256 cf32 entries, built on the host in double with the C library's cos / sin and rounded once to float:
 *   A[k] = (cos, sin)(2 pi k / 2^8),  B[k] = (cos, sin)(2 pi k / 2^16),  C[k] = (cos, sin)(2 pi k / 2^24)
 * sdrx_shift_tables(out) hands them out: A | B | C, (re, im) interleaved, 3 * 256 * 2 floats.
 * Frame f of n samples (n: the tree's raw frame).  Sample j has phase p = (phase + j inc) mod 2^32, and
 *   h = p >> 24,  m = (p >> 16) & 255,  l = (p >> 8) & 255          (the low 8 bits are dropped: truncated, not rounded)
 *   r1 = A[h] (x) B[m],  rot = r1 (x) C[l],  y = x (x) rot
 *   a (x) b = ( fl(fl(ar br) - fl(ai bi)), fl(fl(ar bi) + fl(ai br)) )
 * three fp32 roundings per component, in this association and operand order.  A component of y that is a NaN is the quiet NaN
 * 0x7fc00000, whatever produced it.  At phase = 0, inc = 0 the output has the input's bits for finite samples other than -0.
 * Behind the frame: phase <- (phase + n inc) mod 2^32.
 * The record of frame f (sdrx_shift_record): phase, inc -- what the frame used; next_phase, next_inc -- what it left behind.
 *
 * Settings (sdrx_shift_cfg): inc, phase0; flags: bit 0 SDRX_SHIFT_LOAD_PHASE, the other bits 0 (else SDRX_EINVAL); reserved zeros.
 * sdrx_shift_inc(fs_tree, hz, &inc): rint(hz / fs_tree 2^32) in double, ties to even, mod 2^32; SDRX_EINVAL for non-finite input,
 * fs_tree <= 0 or |hz| > fs_tree / 2.  sdrx_shift_hz(fs_tree, inc): the signed inverse.
 *
 * sdrx_set_shift(ctx, cfg): before sdrx_finalize it switches the stage on (cfg == NULL: off again).  After sdrx_finalize it
 * changes inc between two frames with a one-thread launch in stream order -- the phase carries on, every channel stays
 * phase-continuous -- and with SDRX_SHIFT_LOAD_PHASE also sets the phase to phase0 (SDRX_ESTATE with submitted frames not yet
 * delivered; the calls in flight are drained first); SDRX_ESTATE if the stage was not on at sdrx_finalize, or for cfg == NULL.
 * sdrx_get_shift(ctx, cfg_out, record_out): the settings the last delivered frame ran with (phase0: what sdrx_finalize or the last
 * SDRX_SHIFT_LOAD_PHASE wrote) and its record (either may be NULL), under sdrx_get_blanker's rules.
 * in_frame is unchanged.  sdrx_get_raw, the raw-frame spectrum, the watch, the drift estimate and the band scan see the shifted
 * frame (so the drift estimate reads the residual); sdrx_get_resampler_input, sdrx_get_blanker_input and the ADC meter see what
 * they saw.  A cf32 host frame or a caller's device frame is copied into the context's own buffer first: the caller's buffer is
 * never written.  Offered behind every ingest chain, a real first front stage included.  sdrx_*_shared and sdrx_*_if_same return
 * SDRX_ESTATE if either context has the stage.  Groups do not offer it. */
#define SDRX_SHIFT_LOAD_PHASE 1u
typedef struct sdrx_shift_cfg { /* 32 bytes */
    uint32_t inc, phase0;
    uint32_t flags;
    uint32_t reserved[5];
} sdrx_shift_cfg;
typedef struct sdrx_shift_record { /* 64 bytes */
    int64_t frame;
    uint32_t n_complex, applied;
    uint32_t phase, inc;
    uint32_t next_phase, next_inc;
    uint32_t reserved[8];
} sdrx_shift_record;
int sdrx_set_shift(sdrx_ctx *ctx, const sdrx_shift_cfg *cfg);
int sdrx_get_shift(sdrx_ctx *ctx, sdrx_shift_cfg *cfg_out, sdrx_shift_record *record_out);
void sdrx_shift_tables(float *out);
int sdrx_shift_inc(double fs_tree, double hz, uint32_t *inc);
double sdrx_shift_hz(double fs_tree, uint32_t inc);

/* ---- Spur canceller (sdrx_set_notch before sdrx_finalize) ------------------------------------------------------------
 * Narrow steady carriers that are not signals -- a dongle's clock spurs, a switching regulator's harmonics, a neighbour's birdie --
 * removed from the wideband frame in one pass before the tree fans out: up to SDRX_NOTCH_MAX tones, each a complex amplitude times
 * a table oscillator, the amplitude estimated in blocks of L = 4096 samples, smoothed by a one-pole loop and subtracted one block
 * late, the frequency of each tone re-estimated once a frame from how the block estimates rotate.  A tone given to within tens of Hz
 * is locked and removed, and the record tells where it really is.  The stage sits behind the resampler or whatever comes last in the
 * ingest chain and directly in front of the frequency shift: in place on the tree's raw frame, at the tree's rate, so a tone's
 * frequency is the front end's and does not move when the shift does.  The reference has no counterpart (its DC removal is a notch
 * at 0 Hz only).  This text is the definition, sdrreceiver_amd/notch.py restates it in numpy, and the device is held to that bit for
 * bit.  No FMA anywhere; the same in every setting of option "exact".  Off (the default) nothing changes at all: the same kernels,
 * launches, device_bytes, payloads and callbacks.
 *
 * Settings (sdrx_notch_cfg): n_tones (0 .. 8; 0 = off), inc0[k] (uint32, units of 2^-32 turn a sample, made by sdrx_shift_inc), mu
 * (fp32, 0 < mu <= 1), afc_gain (fp32, 0 .. 1; 0 holds the frequencies), min_coherence (fp32, 0 < c <= 1), max_pull (uint32, inc
 * units: how far a tone may move from its inc0), flags (bit 0 SDRX_NOTCH_LOAD), reserved words and unused tone slots 0.  Anything
 * else is SDRX_EINVAL; no defaults are offered.  Two tones whose inc0 are closer than 8 2^32 / L = 2^23 (circular distance) are
 * refused: a block correlation sees another tone D bins away at 1 / (pi D) of its amplitude, and that leakage is never cancelled
 * because the measurement is on the input -- at 8 bins it is 4 % of the other tone's amplitude.
 * State, per tone: phase, inc (uint32), a (two fp32).  After sdrx_finalize: 0, inc0, 0.
 *
 * A frame of n samples is cut into blocks b = 0 .. of L samples; the last has L_b = n - b L samples, which may be fewer than L.
 * 1. Oscillator.  rot_k[j] is the frequency shift's rotation for p = phase_k + j inc_k (mod 2^32): the same three tables
 *    (sdrx_shift_tables), the same index split, the same (x) of three fp32 roundings a component in the same operand order.
 * 2. Block correlation.  t = x[j] (x) conj(rot_k[j]), the conjugate exact.  A lane sums its 16 consecutive samples in ascending
 *    order from +0, one fp32 addition a step and a component.  The 64 lanes of a wave (1024 samples) combine in the fixed tree "at
 *    distance s = 1, 2, 4, .., 32, lane l with l mod 2s = 0 takes fl(v[l] + v[l + s])"; the four waves of the block combine as
 *    fl(fl(w0 + w1) + fl(w2 + w3)).  Lanes behind the frame's end carry +0.  The result is c[b][k].  The order does not depend on
 *    the frame.
 * 3. Loop.  One sequence per tone, b ascending, every operation a single IEEE double operation in the written order:
 *      m_b = c[b][k] / L_b                       per component
 *      used[b][k] = a                            as fp32: the value in front of the update -- the estimate of block b comes from the
 *                                                blocks before it, for block 0 from the frame before
 *      a <- (float)(a + mu (m_b - a))            per component
 *    and if either component of the new a is not finite: a <- 0 (both), rejected += 1, and the sequence goes on.
 * 4. Subtraction.  y[j] = x[j]; then for k ascending y <- fl(y - (used[b][k] (x) rot_k[j])) per component.  A component that is a
 *    NaN is the quiet NaN 0x7fc00000.
 * 5. Frequency.  Over the FULL blocks only, b = 1 .. nfull - 1 (nfull = floor(n / L)); nothing is done with fewer than two full
 *    blocks.  Accumulated in double, b ascending (each term fl(fl(.) +- fl(.)), then one addition to the sum):
 *      S_re = sum (mr_b mr_{b-1} + mi_b mi_{b-1})     S_im = sum (mi_b mr_{b-1} - mr_b mi_{b-1})     P = sum (mr_b^2 + mi_b^2)
 *      E    = sum ((mr_b - used_re)^2 + (mi_b - used_im)^2)      with used[b][k]: what the estimate missed
 *      coherent = S_re > 0 && S_re >= min_coherence P
 *    If coherent and afc_gain > 0 (adapted = 1):
 *      r = S_im / S_re;  r = r > 1 ? 1 : r;  r = r >= -1 ? r : -1          (a NaN is -1)
 *      d = rint((afc_gain r) 166886.05360752725)                          (2^20 / (2 pi) = 2^32 / (2 pi L): one block's rotation
 *                                                                          in inc units; ties to even)
 *      inc_next = inc + d, then clamped so that the signed wrapped difference inc_next - inc0 stays within +-max_pull (clamped = 1
 *      if that changed it)
 *    else inc_next = inc.  Without the gate a tone that is not there lets inc walk on noise.  Only division, multiplication,
 *    addition, comparison and rint occur.
 * 6. Frame end.  phase_k += n inc_k with the inc that was USED; then inc_k = inc_next: the tone is phase-continuous across frames
 *    and across frequency steps.
 * The record of frame f (sdrx_notch_record): frame, n_complex, n_tones, blocks; per tone the inc used, inc_next, the bits of a at the
 * end, coherent, adapted, clamped, rejected, and the doubles S_re, S_im, P, E (slots from n_tones on: zeros).
 *
 * sdrx_set_notch(ctx, cfg): before sdrx_finalize it switches the stage on (cfg == NULL or n_tones == 0: off again).  After
 * sdrx_finalize it changes mu, afc_gain, min_coherence, max_pull and the tone list between two frames (n_tones may be 0 then: the
 * frame passes unchanged); the list is held within the eight slots allocated at sdrx_finalize.  A slot whose inc0 is unchanged
 * keeps phase, inc and a; a changed or new slot starts at (0, inc0, 0); SDRX_NOTCH_LOAD restarts every slot.  The write is a
 * one-thread launch in stream order.  SDRX_ESTATE with submitted frames not yet delivered (the calls in flight are drained first),
 * if the stage was not on at sdrx_finalize, or for cfg == NULL.
 * sdrx_get_notch(ctx, cfg_out, record_out): the settings as last written, and the record of the last delivered frame under
 * sdrx_get_blanker's rules (either may be NULL).
 * in_frame is unchanged.  sdrx_get_raw, the raw-frame spectrum, the watch, the drift estimate, the band scan and the frequency shift
 * see the notched frame; sdrx_get_resampler_input, sdrx_get_blanker_input and the ADC meter see what they saw.  A cf32 host frame
 * or a caller's device frame is copied into the context's own buffer first: the caller's buffer is never written.  Offered behind
 * every ingest chain, a real first front stage included.  sdrx_*_shared and sdrx_*_if_same return SDRX_ESTATE if either context has
 * the stage.  Groups do not offer it. */
#define SDRX_NOTCH_MAX 8
#define SDRX_NOTCH_LOAD 1u
typedef struct sdrx_notch_cfg { /* 96 bytes */
    uint32_t n_tones, flags;
    uint32_t max_pull, reserved0;
    float mu, afc_gain, min_coherence;
    uint32_t reserved1;
    uint32_t inc0[SDRX_NOTCH_MAX];
    uint32_t reserved[8];
} sdrx_notch_cfg;
typedef struct sdrx_notch_tone { /* 64 bytes */
    uint32_t inc, inc_next;
    uint32_t a_re_bits, a_im_bits;
    uint32_t coherent, adapted, clamped, rejected;
    double s_re, s_im, p, e;
} sdrx_notch_tone;
typedef struct sdrx_notch_record { /* 544 bytes */
    int64_t frame;
    uint32_t n_complex, n_tones, blocks;
    uint32_t reserved[3];
    sdrx_notch_tone tone[SDRX_NOTCH_MAX];
} sdrx_notch_record;
int sdrx_set_notch(sdrx_ctx *ctx, const sdrx_notch_cfg *cfg);
int sdrx_get_notch(sdrx_ctx *ctx, sdrx_notch_cfg *cfg_out, sdrx_notch_record *record_out);

/* decimate[decimateCount] of node `id` (public member vfo.h:39 -- what the fftData signal
 * carries, vfo.cpp:290-293): copies up to max_complex cf32 to `out`, returns the count in *n. */
int sdrx_get_stream(sdrx_ctx *ctx, int id, float *out_iq, int max_complex, int *n);
/* fftVFOSlot(topic) (vfo.cpp:492-509, sdrj.cpp:84-101): the GUI names the VFO(s) whose decimate[decimateCount] it wants
 * from the next frame on -- every VFO whose topic equals the selected string gets emitFFT, so an INI with one topic on two
 * VFOs (or several empty topics) has several taps.  Every node keeps that stream in HBM anyway, with one exception: a leaf
 * whose late decimation is fused into the mix wave (option "fuse_late") writes only its decimated stream -- sdrx_get_stream
 * on it returns SDRX_ENOSTREAM unless it was selected here before the frame was processed (or "keep_streams" is set).
 * sdrx_set_tap REPLACES the selection by `id` (-1: nothing selected: a deselected leaf stops writing its decimate[0]);
 * sdrx_add_tap adds `id` to it.  Not while submitted frames are in flight; contexts are single-caller (one thread). */
int sdrx_set_tap(sdrx_ctx *ctx, int id);
int sdrx_add_tap(sdrx_ctx *ctx, int id);
/* The raw frame exactly as the parent-less VFOs consumed it -- `samples` of sdrj::demodData
 * (sdrj.cpp:266-305) after the byte LUT and the DC-bias removal, what sdrj's own fftData signal
 * carries (sdrj.cpp:296-303) -- natural order, cf32.  Available after sdrx_process,
 * sdrx_process_u8 and the *_fmt calls (after SDRX_FMT_CS8 / SDRX_FMT_CS16 frames, device ones included: the converted floats);
 * after sdrx_process_device the frame was the caller's own device memory and the call returns SDRX_ESTATE. */
int sdrx_get_raw(sdrx_ctx *ctx, float *out_iq, int max_complex, int *n);
int sdrx_get_prequant(sdrx_ctx *ctx, int id, float *out, int max, int *n);
/* Designed tap sets, for parity checks: which = 0 audio low-pass, 1 late-decimation low-pass,
 * 2 Hilbert. */
int sdrx_get_taps(sdrx_ctx *ctx, int id, int which, float *out, int max, int *n);
/* NCO table entries [first, first+count) of node `id` as the device generated them. */
int sdrx_get_nco(sdrx_ctx *ctx, int id, long first, long count, float *out_iq);

/* ---- retuning a running tree ---------------------------------------------------------------------------------
 * sdrx_set_mixer_freqs: VFO ids[k] gets the mixer frequency mixer_freq_hz[k] (vfo::setMixerFreq) from the next frame
 * submitted on.  A retune is the reference's own primitive between two frames, `delete osc_mix; osc_mix = new
 * Oscillator(Fs, f)`: the NCO restarts as a fresh oscillator does (sample 0 of that frame takes the new table's entry L-1,
 * then entries 1, 2, ...: oscillator.cpp:20-50), and everything else is carried over -- half-band histories, the late
 * decimation's FIR, delay line, Hilbert and audio low-pass, the children (they receive the new stream) and an enabled
 * spectrum's state.  sdrx_get_nco reports the new table.  Used for a dongle's drift: a change of mix_offset by D moves the
 * mixer of every sub VFO by -D (mainwindow.cpp:141-225).
 * sdrx_set_gains: vfo::setGain between two vfo::process calls (the reference reads `gain` on every sample, vfo.cpp:328,364):
 * from the next frame on.  The gain of a VFO that does not demodulate USB is stored and has no effect, as in the reference.
 * Both are batched (the drift case retunes thousands of VFOs) and atomic: the whole list is checked first, and a bad or
 * duplicate id, a value that is not finite or n < 0 is SDRX_EINVAL with nothing changed; n == 0 does nothing.  SDRX_ESTATE
 * before sdrx_finalize and while submitted frames are undelivered (as sdrx_set_tap); frames the software pipeline of
 * sdrx_process_device still holds run to their end with the old values first.  One small upload and one launch per call; the
 * call returns when the device has applied it (a retune replays the new table once: a serial chain of Fs steps). */
int sdrx_set_mixer_freqs(sdrx_ctx *ctx, const int *ids, const double *mixer_freq_hz, int n);
int sdrx_set_gains(sdrx_ctx *ctx, const int *ids, const float *gains, int n);

/* ---- device-side AGC (option "agc" = 1) ------------------------------------------------------------------------
 * After every frame a small kernel steps the gain of each USB leaf from that frame's output meter, for the NEXT frame.  The
 * reference has no AGC (its README tells the user to move the VFO gain until JAERO's volume light is green); a change of gain
 * between two frames is the reference's own vfo::setGain between two vfo::process calls, so every frame stays bit for bit what
 * the reference produces with the gain that frame had.  Settings per leaf (sdrx_agc_cfg, 32 bytes, all zero after
 * sdrx_finalize: AGC off) and one word of device state, quiet_run (0 after sdrx_finalize and after every sdrx_set_agc that
 * names the leaf).  The gain itself is the float the demodulation reads (what sdrx_set_gains sets).
 * The step, for every frame f the context processes, on whichever path, once the leaf's meter records of f are complete; with
 * s = the leaf's sum_sq, n = n_values, clipped as sdrx_get_meters defines them, g = the gain frame f was computed with, products
 * in uint64 (< 2^62: no overflow):
 *     parked in f, or n == 0, or hi_ms == 0:   g' = g, action 0, quiet_run unchanged
 *     hot    = clipped > 0 || s > (u64)hi_ms * n
 *     silent = !hot && s < (u64)silent_ms * n
 *     cold   = !hot && !silent && s < (u64)lo_ms * n
 *     hot:     g' = clamp(fl(g * down)); quiet_run = 0; action -1
 *     silent:  g' = g; action 0; quiet_run unchanged
 *     cold:    quiet_run = min(quiet_run + 1, 2^32 - 1);
 *              if quiet_run > hold_frames: g' = clamp(fl(g * up)), action +1   else g' = g, action 0
 *     else:    g' = g; quiet_run = 0; action 0
 *     clamp(x) = fminf(fmaxf(x, gain_min), gain_max)    (one fp32 multiply, no contraction; an overflow to +inf clamps to gain_max)
 * hot wins because a wrapped payload's sum_sq is that of the wrapped values.  The clamp acts only when the AGC moves the gain:
 * a gain the host set outside [gain_min, gain_max] stays while the leaf is in its window.
 * Choosing the window: the output scales with g, its mean square with g^2, so a steady input never alternates between the two
 * steps when hi_ms >= lo_ms * max(up^2, 1 / down^2).  (Not validated: the comparison would mix integers and floats.)  No default
 * window or step is offered: what JAERO's green light corresponds to has not been measured.
 * sdrx_set_agc: batched and atomic, with the calling rules and check order of sdrx_set_squelch_auto; SDRX_ESTATE with the option
 * off.  A setting with hi_ms == 0 is accepted as it is (the other fields are stored and ignored).  Otherwise SDRX_EINVAL with
 * nothing changed unless silent_ms <= lo_ms <= hi_ms <= 2^30 (= 32768^2), up >= 1, 0 < down <= 1, 0 < gain_min <= gain_max, all
 * four floats finite, and the leaf demodulates USB (the gain does not act on a compress() leaf).  One small upload and one
 * small launch per call.
 * sdrx_get_agc: for the last DELIVERED frame (calling rules of sdrx_get_meters), the gain it was computed with, the gain the
 * step left for the next frame, what the step did and quiet_run behind it; the settings as set.  The step's record travels in
 * the frame's fixed-size part beside the meter records, so it can be read while the next frame is in flight.  Leaves without
 * AGC and compress() leaves report gain_used = gain_next = the stored gain and action 0.
 * What goes with it:
 *   sdrx_set_gains on an AGC leaf sets the value the AGC continues from (stream-ordered as before); quiet_run is not touched.
 *     The host's copy of the descriptor gain is stale once the device has stepped: sdrx_get_agc is how a host reads the gain.
 *   Parking: a parked frame is no observation; an unparked leaf continues from the gain the device holds, with quiet_run = 0;
 *     a caught-up frame ("catchup") runs with that gain and gets no step (and no gate): sdrx_get_catchup tells what it held.
 *   Squelch: the gate and the step both read the meter of f and are independent (the step runs behind the gate).  Fixed
 *     thresholds (sdrx_set_squelch) are in output units and so move with the gain: use "squelch_auto", whose floor follows.
 *   Planning: as with "preroll", a tree with a "fuse_demod" leaf off the last level does not use the software pipeline, a tree
 *     with "fuse_demod" leaves does not use "tail_in_levels", and "pipeline" = 1 loses its overlap on such a tree.
 * "agc" = 1 implies "meter".  0 changes nothing: the same kernels, launches, device_bytes, payloads and callbacks.  With 1 and
 * every hi_ms 0 (the start) every payload, meter, stream and gate decision is bit for bit what "meter" = 1 gives. */
typedef struct sdrx_agc_cfg {
    uint32_t lo_ms, hi_ms; /* window on the payload's mean square, LSB^2; hi_ms = 0: AGC off for this leaf */
    uint32_t silent_ms;    /* below this mean square the frame is no observation (dead channel, antenna off) */
    uint32_t hold_frames;  /* consecutive cold frames to sit out before the gain is raised */
    float up, down;        /* step factors */
    float gain_min, gain_max;
} sdrx_agc_cfg;
typedef struct sdrx_agc_state {
    int64_t frame;      /* the frame the step followed */
    float gain_used;    /* the gain that frame was computed with */
    float gain_next;    /* the gain the step left for the next frame */
    int32_t action;     /* -1 lowered | 0 kept | +1 raised */
    uint32_t quiet_run; /* behind the step */
    sdrx_agc_cfg cfg;   /* as set */
} sdrx_agc_state;
int sdrx_set_agc(sdrx_ctx *ctx, const int *ids, const sdrx_agc_cfg *cfgs, int n);
int sdrx_get_agc(sdrx_ctx *ctx, const int *ids, int n, sdrx_agc_state *out);

/* ---- spectrum display ( = MainWindow::fftHandlerSlot, mainwindow.cpp:411-478, on the device) -------------------
 * One display state per enabled spectrum: VFO `id` (its decimate[decimateCount], what vfo.cpp:290-293 emits as fftData)
 * or SDRX_SPECTRUM_RAW (the raw frame exactly as sdrx_get_raw would return it -- for sdrx_process_device /
 * sdrx_submit_device frames the caller's device frame, read inside that frame's own launch sequence).  Per update: the
 * first n_in = min(stream length, 8192) samples times the Hann window (a shorter stream is zero-padded), a kiss_fft of 8192
 * points in kiss_fft's own butterfly order (bins bit-identical to kiss_fft on the same input, whatever option "exact" is),
 * then pwr[(i + 4096) mod 8192] = pwr*0.95 + 0.5*log10(fmax(100000*|bin_i|/8192, 1)) in double, maxval / aveval of pwr and
 * the "maxval - aveval < 10 -> maxval = aveval + 10" rule.
 * Cadence: a VFO spectrum is updated after every frame whose stream exists (a leaf whose late decimation or demodulation
 * is fused into the mix wave keeps its stream only while it is tapped, sdrx_set_tap: otherwise `updates` does not move);
 * the raw spectrum follows sdrj's counter (sdrj.cpp:296-303): the 5th frame after enabling, then every 4th.
 * Deliberately not reproduced: the reference's ONE shared display when a GUI topic names several VFOs (their updates and
 * stale tails mixed in tree order) -- here every VFO has its own state, which equals the reference whenever one VFO is
 * selected.  No spectrum enabled: no launch, no allocation, no event -- payloads and streams are identical either way. */
#define SDRX_SPECTRUM_BINS 8192 /* nFFT, mainwindow.cpp:243 */
#define SDRX_SPECTRUM_RAW (-2)  /* sdrj's own fftData: the raw frame, at sdrj's every-4th-call cadence */
typedef struct sdrx_spectrum_info {
    int64_t updates;        /* fftHandlerSlot calls since the spectrum was enabled */
    int32_t n_in;           /* samples each update windows: min(stream length, 8192) */
    int32_t reserved;
    double maxval, aveval;  /* of the last update, after the "< 10 dB" rule */
} sdrx_spectrum_info;
/* enable = 1: allocate (if needed) and ZERO the state and, for SDRX_SPECTRUM_RAW, the cadence counter (the GUI's combo-box
 * reset, mainwindow.cpp:539-549); 0: release it.  After sdrx_finalize, not while submitted frames are in flight. */
int sdrx_set_spectrum(sdrx_ctx *ctx, int id, int enable);
/* The state after the last frame: `pwr` 8192 doubles (display order), `smooth` 8182 doubles (the 5-point mean of
 * mainwindow.cpp:454-458), `bins_iq` 2*8192 floats (the last update's FFT output, natural order); each may be NULL.
 * SDRX_ESTATE before sdrx_finalize, while frames are in flight, or for a spectrum that is not enabled; SDRX_EINVAL for a bad
 * id.  Runs what the software pipeline of sdrx_process_device still holds first. */
int sdrx_get_spectrum(sdrx_ctx *ctx, int id, sdrx_spectrum_info *info, double *pwr, double *smooth, float *bins_iq);
/* The many-channel monitor: maxval / aveval / updates of n enabled spectra `ids` in one small device-to-host copy (each
 * output array may be NULL). */
int sdrx_get_spectrum_levels(sdrx_ctx *ctx, const int *ids, int n, double *maxval, double *aveval, int64_t *updates);

/* ---- Detector leaves: an AM envelope or an FM discriminator in place of compress() -------------------------------------------
 * No counterpart in the reference.  A leaf with demod_usb = 0 can be given a detector before sdrx_finalize.  Its payload is then n
 * int16 per frame -- n = fs-side samples_per_buffer / 2^decimate_count, the leaf's stream length -- in place of compress()'s bytes
 * (the same byte count as cstyle 0).  sdrx_vfo_desc is unchanged: any non-zero demod_usb means USB, every cstyle is taken.
 *
 * This text is the definition; csrc/sdrx_detect.h spells it per sample and sdrreceiver_amd/detect.py is the model the tests hold the
 * device to, bit for bit.  Every operation is ONE fp32 operation, separately rounded, no FMA -- the same in all three settings of
 * option "exact", given the stream the device holds (as the watch's PSD is).  z[i] = (re, im) is sample i of the leaf's stream.
 *
 * SDRX_DETECT_AM
 *   1. e[i] = sqrt(fl(fl(re re) + fl(im im))), the correctly rounded fp32 square root;
 *   2. the frame's carrier: S = sum of q[i] over the frame's n samples, q[i] = min(e[i], 2^15) 2^8 rounded to nearest even as an
 *      unsigned integer (a NaN counts as 2^15), summed in 64-bit integers: independent of order and geometry;
 *   3. c = (float)((double)S / (double)(256 n));
 *   4. pre[i] = fl(fl(e[i] - c) gain), then the USB leaves' conversion: pre 32768 in double, truncated to int32 as the x86-64
 *      build does (INT32_MIN outside it), the low 16 bits kept.
 *   The carrier is the frame's own: an AM leaf carries nothing from frame to frame, and a frame of zeros gives zeros.
 * SDRX_DETECT_FM
 *   1. with z[i] = (a, b) and z[i-1] = (p, q): d_re = fl(fl(a p) + fl(b q)), d_im = fl(fl(b p) - fl(a q));
 *   2. x = ANG(d_im, d_re), the angle in half-turns, in [-1, 1]: t = min(|y|, |x|) / max(|y|, |x|) (one correctly rounded division;
 *      0 where both are 0), atan(t) / pi = t P(t t) with P of degree 5 in separately rounded Horner steps (the coefficients are in
 *      sdrx_detect.h), 1/2 - r where |y| > |x|, 1 - r where x < 0, negated where y < 0; ANG(0, 0) = 0.  Its error against atan2 is
 *      below 1e-5 rad: at gain = 1 -- full scale = a deviation of fs / 2 -- a third of one LSB;
 *   3. pre[i] = fl(x gain), then the same conversion.
 *   z[-1] of a frame is the last stream sample of the leaf's frame before; 0 + 0j for a leaf that sdrx_finalize, sdrx_set_active,
 *   the catch-up or the wake starts as a new vfo.
 *
 * `gain` acts as on a USB leaf (sdrx_set_gains included); cstyle, scalecomp and filter_bw_hz are ignored -- the post-detection
 * filter is a setting of its own ("Post-detection filter", below).  The leaf publishes by the IQ leaf's rule (only with a topic; rate = fs / 2^decimate_count, len = 2 n), its
 * watch band is the IQ leaf's, and its output meter is the USB leaves' (n_values = n, int16 full scale).  The squelch gate, the
 * auto-squelch, the pre-roll, parking, the catch-up, the watch and the wake serve it as they serve any leaf; sdrx_set_agc answers
 * what it answers for an IQ leaf; fuse_demod and keep_prequant do not apply.  sdrx_get_kernel_times books its launches with
 * k_compress.  With no detector set anywhere the library launches, allocates and delivers exactly what it did without this section.
 *
 * sdrx_set_detector: before sdrx_finalize (SDRX_ESTATE after it); SDRX_EINVAL for a bad id, a node with demod_usb != 0, an unknown
 * kind or a non-zero reserved word.  SDRX_DETECT_NONE takes the detector away again.  sdrx_finalize returns SDRX_EINVAL for a node
 * with children that carries a detector.  sdrx_get_detector: the setting of any node, at any time.
 * Groups do not offer it: a group's members are made by sdrx_group_finalize, and on a member handed out by sdrx_group_member the
 * call returns SDRX_ESTATE as on every finalized context. */
#define SDRX_DETECT_NONE 0
#define SDRX_DETECT_AM 1
#define SDRX_DETECT_FM 2
typedef struct sdrx_detect_cfg { /* 16 bytes */
    int32_t kind;
    int32_t reserved[3];
} sdrx_detect_cfg;
int sdrx_set_detector(sdrx_ctx *ctx, int id, const sdrx_detect_cfg *cfg);
int sdrx_get_detector(sdrx_ctx *ctx, int id, sdrx_detect_cfg *cfg_out);

/* ---- Post-detection filter: a FIR low-pass and a decimation on a detector leaf ---------------------------------------------------
 * No counterpart in the reference.  A detector leaf can be given a real FIR of the caller's taps h[t], t < T, over the detector's
 * pre-quantisation floats, decimated by an integer R, before sdrx_finalize.  It carries its state from frame to frame.  This text
 * is the definition; csrc/sdrx_postdet.h spells it per output and sdrreceiver_amd/postdet.py is the model the tests hold the device
 * to, bit for bit, in every setting of option "exact".
 *
 * pre_f[i], 0 <= i < n, is frame f's value of step 4 (AM) or step 3 (FM) of "Detector leaves", before the conversion.
 *   - The carrier and gain are those frame f had.
 *   - For j < 0, pre_f[j] := pre_{f-1}[n + j].
 *     - This applies recursively when n < T - 1.
 *     - It is +0.0f for a leaf that sdrx_finalize, sdrx_set_active, the catch-up or the wake starts as a new vfo.
 *     - An FM leaf started that way still has z[-1] = 0 as well.
 *   - A gain change or a new AM carrier does not rewrite history: the filter sees what a host filter behind the channel would have
 *     seen.
 *
 * With taps h[t], t < T, and decimation R, for output m in [0, n / R):
 *
 *   acc_0 = +0.0f;   acc_{t+1} = fl(acc_t + fl(h[t] * pre[m R - t])),  t = 0 .. T-1 ascending;   y[m] = acc_T
 *
 *   - Two roundings per tap, no FMA, the same in all three settings of exact.  This is the idiom of the resampler and the front
 *     stage.
 *   - The payload is the USB leaves' conversion of y[m]: n / R int16.
 *   - The output meter is meter_usb over those n / R values (n_values = n / R).
 *   - The leaf publishes by the IQ leaf's rule with rate = fs / 2^decimate_count / R and len = 2 n / R.
 *   - The group delay is (T - 1) / 2 stream samples.
 *   - T = 1, h = {1.0f}, R = 1 is the identity.  Payload and meter records are bit for bit those of the same leaf without the
 *     stage.
 *   - Behaviour on non-finite pre is whatever IEEE gives.
 *
 * Limits: 1 <= T <= 256; 1 <= R <= 16; n % R == 0, else SDRX_EUNSUPPORTED at sdrx_finalize with the reason in sdrx_last_error.
 *
 * The squelch gate, the pre-roll, parking, the catch-up and the wake serve the shorter payload as they serve any leaf's; the
 * launches are booked with k_compress.  With no post filter anywhere the library launches, allocates and delivers exactly what it
 * did without this section.  Not offered: IIR de-emphasis, a DC block for FM, changing taps on a running tree, groups, the AGC.
 *
 * sdrx_set_postfilter: before sdrx_finalize (SDRX_ESTATE after it, and so on a group's members); SDRX_EINVAL for a bad id, limits
 * exceeded, null taps or a non-zero reserved word; ntaps = 0 takes the filter away (decim and taps are not looked at).  The taps
 * are copied.  sdrx_finalize returns SDRX_EINVAL for a node that carries a post filter without a detector.
 * sdrx_get_postfilter: at any time; SDRX_ESTATE for a node without one.  `taps` may be NULL; otherwise min(ntaps, cap) floats are
 * written.  out_len = n / R once the tree is finalized (0 before), delay_samples = (T - 1) / 2; pass_hz = stop_hz = 0: the
 * library does not know how the caller's taps were made.
 * sdrx_postfilter_design needs no context and no device: a Kaiser low-pass in IEEE double, rounded once to fp32.  With
 * N = ntaps and A = atten_db: beta = 0.1102 (A - 8.7) and tw = (A - 7.95) / (2.285 (N - 1) 2 pi) -- sdrx_resampler_design's --,
 * fc = cutoff_hz / fs, h[k] = 2 fc sinc(2 fc (k - (N-1)/2)) I0(beta sqrt(1 - (2k/(N-1) - 1)^2)) / I0(beta), divided by the double
 * sum of the h[k] taken with k ascending: unit DC gain.  SDRX_EINVAL unless 50 < A <= 120, 1 <= N <= 256, fs > 0, cutoff_hz > 0
 * and (with taps given) cap >= N; SDRX_EFILTER if fc - tw/2 <= 0 or fc + tw/2 > 0.5 (N = 1 always).  `taps` and `info` may be
 * NULL.  info: decim = 0, out_len = 0, ntaps = N, delay_samples = (N - 1) / 2, pass_hz = (fc - tw/2) fs, stop_hz = (fc + tw/2) fs.
 * Whether stop_hz <= fs / (2 R) is the caller's decision; no default is offered. */
#define SDRX_POSTFILTER_MAX_TAPS 256
#define SDRX_POSTFILTER_MAX_DECIM 16
typedef struct sdrx_postfilter_cfg { /* 16 bytes */
    int32_t decim, ntaps;
    int32_t reserved[2];
} sdrx_postfilter_cfg;
typedef struct sdrx_postfilter_info { /* 40 bytes */
    int32_t decim, ntaps, out_len, reserved;
    double delay_samples, pass_hz, stop_hz;
} sdrx_postfilter_info;
int sdrx_set_postfilter(sdrx_ctx *ctx, int id, const sdrx_postfilter_cfg *cfg, const float *taps);
int sdrx_get_postfilter(sdrx_ctx *ctx, int id, sdrx_postfilter_info *info, float *taps, int32_t cap);
int sdrx_postfilter_design(double fs, double cutoff_hz, int32_t ntaps, double atten_db, float *taps, int32_t cap, sdrx_postfilter_info *info);

/* ---- one tree on several GPUs, one host process ---------------------------------------------------
 * The fan-out the reference does on one thread -- sdrj::demodData over the main VFOs (sdrj.cpp:288-294),
 * each main over its sub VFOs (vfo.cpp:253-264) -- sharded over the devices of one node:
 * a group owns one sdrx_ctx per device.  sdrx_group_add_vfo describes the WHOLE tree exactly like
 * sdrx_add_vfo; sdrx_group_finalize gives device k of W, for every parent-less VFO with children, the
 * block [K k / W, K (k+1) / W) of its K children together with everything below them, plus a replica of
 * the parent where that block is not empty (parent-less leaves are block-partitioned among themselves).
 * Per frame the raw IQ lands on the FIRST device of the list and is fanned out to the others by one
 * peer-to-peer copy each (hipMemcpyPeerAsync on the receiving device's stream: over xGMI every peer is
 * one direct link from the source, the copies run on different links at once), double-buffered by frame
 * parity; every device then runs its shard and copies its payloads back itself.  The publish callback is
 * invoked in the reference's order over the whole tree, whichever device computed a leaf.  Ids are those
 * of sdrx_group_add_vfo.  `devices` may name a device more than once (two shards on one GPU: tests).
 * sdrx_group_submit* / _wait / _process mirror sdrx_submit* / sdrx_wait / sdrx_process.  For
 * sdrx_group_submit_device the frame (cf32, on the first device) must be complete in the order of
 * `producer_stream` (a hipStream_t of that device; NULL: complete already) and stay untouched until
 * it was waited for.  A device that ends up without VFOs (more devices than sub VFOs) stays idle. */
typedef struct sdrx_group sdrx_group;
int sdrx_group_create(sdrx_group **grp, const int *device_ordinals, int n_devices);
int sdrx_group_destroy(sdrx_group *grp);
const char *sdrx_group_last_error(const sdrx_group *grp); /* grp may be NULL: error of a failed create */
int sdrx_group_size(const sdrx_group *grp);
/* 1: every member reaches the first device's frame buffer directly (same device, or peer access enabled: one
 * xGMI link per peer, the N-1 copies run at once); 0: the runtime stages at least one peer copy through host
 * memory (still correct, slower) -- sdrx_group_last_error() right after sdrx_group_create names the device. */
int sdrx_group_peer_access(const sdrx_group *grp);
int sdrx_group_add_vfo(sdrx_group *grp, const sdrx_vfo_desc *desc, int *id_out);
int sdrx_group_set_option(sdrx_group *grp, const char *name, int value); /* applied to every member */
int sdrx_group_set_publish_callback(sdrx_group *grp, sdrx_publish_fn fn, void *user);
int sdrx_group_finalize(sdrx_group *grp);
int sdrx_group_process(sdrx_group *grp, const float *iq, int n_complex);
int sdrx_group_submit(sdrx_group *grp, const float *iq, int n_complex);
/* Dongle bytes: a quarter of the bytes cross PCIe and xGMI, every device applies the b - 127 LUT itself
 * (jonti/sdr.cpp:43-49) and, if correct_dc != 0, the DC-bias IIR of sdrj.cpp:271-286 on the whole frame with
 * an accumulator of its own -- identical bytes and identical start state keep the devices' estimates
 * identical, so only the bytes travel.  What the shipped sdr_25E.ini (correct_dc_bias=1) needs. */
int sdrx_group_submit_u8(sdrx_group *grp, const uint8_t *iq_bytes, int n_complex, int correct_dc);
int sdrx_group_process_u8(sdrx_group *grp, const uint8_t *iq_bytes, int n_complex, int correct_dc);
/* Integer samples of any format (SDRX_FMT_*, above): the raw integers are fanned out -- 2 or 4 bytes a sample, a quarter or
 * half of a cf32 frame's traffic -- and every member converts them and, if correct_dc != 0, removes the DC bias with an
 * accumulator of its own, as for bytes.  (No device-frame forms of these for groups.) */
int sdrx_group_submit_fmt(sdrx_group *grp, const void *iq, int n_complex, int fmt, int correct_dc);
int sdrx_group_process_fmt(sdrx_group *grp, const void *iq, int n_complex, int fmt, int correct_dc);
int sdrx_group_submit_device(sdrx_group *grp, const void *dev_iq_on_first_device, int n_complex, void *producer_stream);
/* like sdrx_process_device: kernels only, asynchronous; the frame must stay untouched until sdrx_group_sync */
int sdrx_group_process_device(sdrx_group *grp, const void *dev_iq_on_first_device, int n_complex, void *producer_stream);
int sdrx_group_wait(sdrx_group *grp);
int sdrx_group_in_flight(sdrx_group *grp);
int sdrx_group_sync(sdrx_group *grp);
int sdrx_group_get_output(sdrx_group *grp, int id, const void **buf, uint32_t *len_bytes, uint32_t *rate);
/* Where a VFO lives: *member = index into the device list (the owner of a leaf; the first replica of
 * a VFO with children), *local_id = its id inside that member's context; sdrx_group_member hands out
 * that context (NULL for a member that holds no VFOs) for sdrx_get_stream / sdrx_get_stats / kernel
 * timing. */
int sdrx_group_locate(sdrx_group *grp, int id, int *member, int *local_id);
int sdrx_group_member(sdrx_group *grp, int k, sdrx_ctx **ctx, int *device_ordinal);
/* sdrx_set_mixer_freqs / sdrx_set_gains with ids of the whole tree: applied on every member that holds the VFO (a VFO with
 * children is replicated on each member that holds part of its subtree); a member with nothing listed makes no launch. */
int sdrx_group_set_mixer_freqs(sdrx_group *grp, const int *ids, const double *mixer_freq_hz, int n);
int sdrx_group_set_gains(sdrx_group *grp, const int *ids, const float *gains, int n);
/* sdrx_get_meters with ids of the whole tree (group option "meter" = 1): each id is answered by the member that owns the
 * leaf (sdrx_group_locate); `frame` counts the group's frames. */
int sdrx_group_get_meters(sdrx_group *grp, const int *ids, int n, sdrx_meter *out);
/* sdrx_set_squelch / sdrx_get_squelch with ids of the whole tree (group option "squelch" = 1), each id routed to the member
 * that owns the leaf; sdrx_group_get_egress sums n_open, n_leaves and payload_bytes_copied over the members. */
int sdrx_group_set_squelch(sdrx_group *grp, const int *ids, const uint64_t *thr_sum_sq, const uint32_t *hang_frames, int n);
int sdrx_group_get_squelch(sdrx_group *grp, const int *ids, int n, sdrx_squelch_state *out);
int sdrx_group_get_egress(sdrx_group *grp, int64_t *frame, uint32_t *n_open, uint32_t *n_leaves, uint64_t *payload_bytes_copied);
/* sdrx_set_squelch_auto / sdrx_get_squelch_auto with ids of the whole tree (group option "squelch_auto" = 1), each id routed
 * to the member that owns the leaf. */
int sdrx_group_set_squelch_auto(sdrx_group *grp, const int *ids, const uint32_t *ratio_q8, const uint32_t *window_frames, int n);
int sdrx_group_get_squelch_auto(sdrx_group *grp, const int *ids, int n, sdrx_squelch_auto_state *out);
/* sdrx_set_agc / sdrx_get_agc with ids of the whole tree (group option "agc" = 1), each id routed to the member that owns the
 * leaf; `frame` counts the group's frames. */
int sdrx_group_set_agc(sdrx_group *grp, const int *ids, const sdrx_agc_cfg *cfgs, int n);
int sdrx_group_get_agc(sdrx_group *grp, const int *ids, int n, sdrx_agc_state *out);
/* sdrx_set_active / sdrx_get_active with ids of the whole tree (group option "park" = 1), each id routed to the member that
 * owns the leaf; `since_frame` counts the group's frames. */
int sdrx_group_set_active(sdrx_group *grp, const int *ids, const int32_t *active, int n);
int sdrx_group_get_active(sdrx_group *grp, const int *ids, int n, sdrx_active_state *out);
/* sdrx_get_catchup with ids of the whole tree (group option "catchup" = 1; sdrx_group_set_active is unchanged in form), each id
 * routed to the member that owns the leaf, as sdrx_group_get_meters. */
int sdrx_group_get_catchup(sdrx_group *grp, const int *ids, int n, sdrx_meter *out);
/* sdrx_set_watch / sdrx_get_watch / sdrx_get_watch_psd with ids of the whole tree (group option "watch" = 1), each id routed to
 * the member that owns the leaf; each member measures the replicas of the source streams it holds. */
int sdrx_group_set_watch(sdrx_group *grp, const int *ids, const int32_t *on, int n);
int sdrx_group_get_watch(sdrx_group *grp, const int *ids, int n, sdrx_watch_level *out);
int sdrx_group_get_watch_psd(sdrx_group *grp, int leaf_id, double *psd, int64_t *frame);
/* sdrx_set_drift / sdrx_get_drift / sdrx_get_drift_profile with an id of the whole tree, routed to the member that holds the
 * leaf.  A source replicated on several members has one template per member: set it through a leaf of each member that is to
 * measure it. */
int sdrx_group_set_drift(sdrx_group *grp, int leaf_id, const double *templ, int max_shift);
int sdrx_group_get_drift(sdrx_group *grp, int leaf_id, sdrx_drift_level *out);
int sdrx_group_get_drift_profile(sdrx_group *grp, int leaf_id, double *profile, int64_t *frame);
/* sdrx_set_scan / sdrx_get_scan / sdrx_get_scan_hits / sdrx_get_scan_cells with an id of the whole tree, routed to the member
 * that holds the leaf.  A source replicated on several members has one scan state per member, as it has one template. */
int sdrx_group_set_scan(sdrx_group *grp, int leaf_id, const sdrx_scan_cfg *cfg);
int sdrx_group_get_scan(sdrx_group *grp, int leaf_id, sdrx_scan_level *out);
int sdrx_group_get_scan_hits(sdrx_group *grp, int leaf_id, sdrx_scan_hit *hits, int max_hits, int *n, int64_t *frame);
int sdrx_group_get_scan_cells(sdrx_group *grp, int leaf_id, double *cells, int64_t *frame);
/* sdrx_set_wake / sdrx_get_wake with ids of the whole tree (group option "wake" = 1), each id routed to the member that owns
 * the leaf; `frame` and `since_frame` count the group's frames. */
int sdrx_group_set_wake(sdrx_group *grp, const int *ids, const sdrx_wake_cfg *cfgs, int n);
int sdrx_group_get_wake(sdrx_group *grp, const int *ids, int n, sdrx_wake_state *out);
/* sdrx_get_adc_meter for the group (group option "adc_meter" = 1, applied to every member): every member that is sent the
 * integers measures them, the records are identical, and the first member answers. */
int sdrx_group_get_adc_meter(sdrx_group *grp, sdrx_adc_meter *out);

/* sdrx_get_preroll routed to the member that owns the leaf; sdrx_get_preroll_count summed over the members (group option
 * "preroll" = 1). */
int sdrx_group_get_preroll(sdrx_group *grp, int id, const void **buf, uint32_t *len_bytes, int64_t *frame);
int sdrx_group_get_preroll_count(sdrx_group *grp, uint32_t *n_preroll, uint64_t *preroll_bytes);

/* ---- introspection / measurement ------------------------------------------------------------- */
typedef struct sdrx_stats {
    int32_t n_vfos, n_leaves, n_levels;
    int32_t exact;
    int64_t algorithmic_bytes_per_frame; /* sum of 8*n_in + W_out              */
    int64_t vfo_samples_per_frame;       /* sum of n_in over all VFOs                        */
    int64_t device_bytes;                /* HBM allocated by this context                    */
    int64_t frames;                      /* frames processed so far                          */
    int64_t mix_chunks_per_frame;        /* 1024-sample chunks the k_mix_decimate waves walk  */
                                         /*   per frame, warm-up chunks of segments included  */
    int64_t dc_blocks;                   /* exact DC-bias removal (sdrx_process_u8 .. correct_dc): 1024-sample blocks of one */
    int64_t dc_fallback_blocks;          /*   component walked so far / of those, redone with the sequential operations     */
    int64_t dc_retried_blocks;           /*   / taken again on their own because the step of several blocks they were part of */
                                         /*   did not verify as a whole (and then did: not counted as redone)                */
} sdrx_stats;
/* Everything but the three dc_* counters is host-side bookkeeping and costs nothing.  Once the context has run a frame with
 * correct_dc the dc_* counters live on the device: the call then WAITS for whatever is queued on the context's stream and
 * copies them back (a measurement call: a host that polls it between sdrx_submit and sdrx_wait serialises the frame it has
 * just queued).  They count what has EXECUTED, so they can lag `frames` by the frames still inside the launch pipeline
 * of sdrx_process_device (sdrx_sync / sdrx_fetch first for a consistent reading). */
int sdrx_get_stats(sdrx_ctx *ctx, sdrx_stats *out);
/* Per-kernel GPU time from HIP events recorded on the launch stream.  enable=1 brackets every
 * kernel launch with events (small overhead: use for profiling runs, not for throughput runs).
 * sdrx_get_kernel_times: accumulated milliseconds and launch counts since enabling, for
 * kernel kinds 0..SDRX_NKERNELS-1 (names from sdrx_kernel_name). */
#define SDRX_NKERNELS 8
int sdrx_enable_kernel_timing(sdrx_ctx *ctx, int enable);
int sdrx_get_kernel_times(sdrx_ctx *ctx, double ms[SDRX_NKERNELS], int64_t launches[SDRX_NKERNELS],
                          int64_t alg_bytes[SDRX_NKERNELS]);
const char *sdrx_kernel_name(int kind);

#ifdef __cplusplus
}
#endif
#endif /* SDRX_H */
