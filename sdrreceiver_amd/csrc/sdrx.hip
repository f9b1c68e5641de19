// sdrx.hip -- host side of libsdrx.so: the C ABI of include/sdrx.h, VFO-tree bookkeeping,
// HBM layout, and the per-frame launch sequence.  The arithmetic lives in the files kernels.hip includes.
//
// Data layout in HBM (all in one arena, zeroed at finalize == the reference's zero start state):
//   per VFO   NCO checkpoints  (L/16+1) cf32           cp[j] = table[16j-1]
//             half-band state  2 x d x 10 cf32         ping-pong by frame parity
//             stream           2 x (H + n/2^d) cf32    decimate[d] of the current frame behind H
//                                                       history samples of the previous frame
//                                                       (H = 0 for VFOs that only feed children)
//             late-dec stream  2 x (H' + n_out) cf32   only for lateDecimate leaves
//   per leaf  payload          n_out int16 | n (or 2n) int8, packed in one buffer => one D2H copy
// Frame f reads state[f&1] and writes state[(f+1)&1]; nothing is copied between frames.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/sdrx.h"
#include "kernels.hip"
#include "spectrum.hip"
#include "squelch.hip"
#include "agc.hip"
#include "watch.hip"
#include "wake.hip"
#include "drift.hip"
#include "scan.hip"
#include "tapdesign.h"

#include "sdrx_mem.h"

using namespace sdrx;

static_assert(sizeof(sdrx_vfo_desc) == 56 && offsetof(sdrx_vfo_desc, topic) == 48, "sdrx_vfo_desc ABI layout");
static_assert(sizeof(sdrx_stats) == 80, "sdrx_stats ABI layout");
static_assert(sizeof(sdrx_spectrum_info) == sizeof(SpecRecord) && offsetof(sdrx_spectrum_info, maxval) == offsetof(SpecRecord, maxval) &&
                  SDRX_SPECTRUM_BINS == kSpecN,
              "sdrx_spectrum_info ABI layout");
static_assert(sizeof(sdrx_agc_cfg) == 32 && sizeof(AgcCfg) == 32 && offsetof(sdrx_agc_cfg, up) == offsetof(AgcCfg, up) && sizeof(sdrx_agc_state) == 56 &&
                  offsetof(sdrx_agc_state, cfg) == 24,
              "sdrx_agc_cfg / sdrx_agc_state ABI layout");
static_assert(sizeof(sdrx_watch_level) == 48 && sizeof(WatchRecord) == 48 && offsetof(sdrx_watch_level, total_pwr) == offsetof(WatchRecord, total_pwr) &&
                  offsetof(sdrx_watch_level, watched) == offsetof(WatchRecord, watched) && SDRX_WATCH_MAX_SEGMENTS == kWatchMaxSeg,
              "sdrx_watch_level ABI layout");
static_assert(sizeof(sdrx_drift_level) == 64 && sizeof(DriftRecord) == 64 && offsetof(sdrx_drift_level, zero) == offsetof(DriftRecord, zero) &&
                  offsetof(sdrx_drift_level, captured) == offsetof(DriftRecord, captured) && SDRX_DRIFT_MAX_SHIFT == kDriftMaxShift,
              "sdrx_drift_level ABI layout");
static_assert(sizeof(sdrx_scan_cfg) == 32 && sizeof(ScanCfg) == 32 && offsetof(sdrx_scan_cfg, min_cells) == offsetof(ScanCfg, min_cells) &&
                  sizeof(sdrx_scan_hit) == 32 && sizeof(ScanHit) == 32 && offsetof(sdrx_scan_hit, peak_pwr) == offsetof(ScanHit, peak_pwr) &&
                  sizeof(sdrx_scan_level) == 64 && sizeof(ScanRecord) == 64 && offsetof(sdrx_scan_level, n_hits) == offsetof(ScanRecord, n_hits) &&
                  offsetof(sdrx_scan_level, complete) == offsetof(ScanRecord, complete) && SDRX_SCAN_MAX_HITS == kScanMaxHits,
              "band scan ABI layout");
static_assert(sizeof(sdrx_wake_cfg) == 32 && sizeof(WakeCfg) == 32 && offsetof(sdrx_wake_cfg, on) == offsetof(WakeCfg, on) && sizeof(sdrx_wake_state) == 32 &&
                  sizeof(WakeRecord) == 32 && offsetof(sdrx_wake_state, hold_left) == offsetof(WakeRecord, hold_left) &&
                  offsetof(sdrx_wake_state, controlled) == offsetof(WakeRecord, controlled),
              "sdrx_wake_cfg / sdrx_wake_state ABI layout");
static_assert(sizeof(sdrx_resampler_info) == 48 && offsetof(sdrx_resampler_info, delay_out_samples) == 32, "sdrx_resampler_info ABI layout");
static_assert(sizeof(sdrx_front_info) == 48 && offsetof(sdrx_front_info, tw) == 32, "sdrx_front_info ABI layout");
static_assert(sizeof(sdrx_blanker_cfg) == 32 && sizeof(BlankCfg) == 32 && offsetof(sdrx_blanker_cfg, rank_q16) == offsetof(BlankCfg, rank_q16) &&
                  offsetof(sdrx_blanker_cfg, guard) == offsetof(BlankCfg, guard) && sizeof(sdrx_blanker_record) == 64 && sizeof(BlankRecord) == 64 &&
                  offsetof(sdrx_blanker_record, thr_bits) == offsetof(BlankRecord, thr_bits) &&
                  offsetof(sdrx_blanker_record, next_ref_bin) == offsetof(BlankRecord, next_ref_bin) &&
                  offsetof(sdrx_blanker_record, carry_in) == offsetof(BlankRecord, carry_in),
              "sdrx_blanker_cfg / sdrx_blanker_record ABI layout");
static_assert(sizeof(sdrx_iq_cfg) == 32 && sizeof(IqCfg) == 32 && offsetof(sdrx_iq_cfg, d0) == offsetof(IqCfg, d0) && offsetof(sdrx_iq_cfg, flags) == offsetof(IqCfg, flags) &&
                  sizeof(sdrx_iq_record) == 96 && sizeof(IqRecord) == 96 && offsetof(sdrx_iq_record, rejected) == offsetof(IqRecord, rejected) &&
                  offsetof(sdrx_iq_record, next_d_bits) == offsetof(IqRecord, next_d_bits) && offsetof(sdrx_iq_record, sum_i) == offsetof(IqRecord, sum_i) &&
                  offsetof(sdrx_iq_record, sum_qq) == offsetof(IqRecord, sum_qq) && sizeof(IqState) == 64 && SDRX_IQ_LOAD == kIqLoad,
              "sdrx_iq_cfg / sdrx_iq_record ABI layout");
static_assert(sizeof(sdrx_shift_cfg) == 32 && sizeof(ShiftCfg) == 32 && offsetof(sdrx_shift_cfg, phase0) == offsetof(ShiftCfg, phase0) &&
                  offsetof(sdrx_shift_cfg, flags) == offsetof(ShiftCfg, flags) && sizeof(sdrx_shift_record) == 64 && sizeof(ShiftRecord) == 64 &&
                  offsetof(sdrx_shift_record, applied) == offsetof(ShiftRecord, applied) && offsetof(sdrx_shift_record, phase) == offsetof(ShiftRecord, phase) &&
                  offsetof(sdrx_shift_record, next_inc) == offsetof(ShiftRecord, next_inc) && offsetof(sdrx_shift_record, reserved) == offsetof(ShiftRecord, reserved) &&
                  sizeof(ShiftState) == 16 && SDRX_SHIFT_LOAD_PHASE == kShLoadPhase,
              "sdrx_shift_cfg / sdrx_shift_record ABI layout");
static_assert(sizeof(sdrx_notch_cfg) == 96 && sizeof(NotchCfg) == 96 && offsetof(sdrx_notch_cfg, max_pull) == offsetof(NotchCfg, max_pull) &&
                  offsetof(sdrx_notch_cfg, mu) == offsetof(NotchCfg, mu) && offsetof(sdrx_notch_cfg, min_coherence) == offsetof(NotchCfg, min_coherence) &&
                  offsetof(sdrx_notch_cfg, inc0) == offsetof(NotchCfg, inc0) && offsetof(sdrx_notch_cfg, reserved) == offsetof(NotchCfg, reserved) &&
                  sizeof(sdrx_notch_tone) == 64 && sizeof(NotchToneRecord) == 64 && offsetof(sdrx_notch_tone, a_re_bits) == offsetof(NotchToneRecord, a_re_bits) &&
                  offsetof(sdrx_notch_tone, rejected) == offsetof(NotchToneRecord, rejected) && offsetof(sdrx_notch_tone, s_re) == offsetof(NotchToneRecord, s_re) &&
                  offsetof(sdrx_notch_tone, e) == offsetof(NotchToneRecord, e) && sizeof(sdrx_notch_record) == 544 && sizeof(NotchRecord) == 544 &&
                  offsetof(sdrx_notch_record, blocks) == offsetof(NotchRecord, blocks) && offsetof(sdrx_notch_record, tone) == offsetof(NotchRecord, tone) &&
                  sizeof(NotchTone) == 32 && SDRX_NOTCH_LOAD == kNtLoad && SDRX_NOTCH_MAX == kNtMax,
              "sdrx_notch_cfg / sdrx_notch_record ABI layout");
static_assert(sizeof(sdrx_detect_cfg) == 16 && sizeof(DetectCfg) == 16 && offsetof(sdrx_detect_cfg, reserved) == offsetof(DetectCfg, reserved) &&
                  SDRX_DETECT_NONE == kDetNone && SDRX_DETECT_AM == kDetAm && SDRX_DETECT_FM == kDetFm,
              "sdrx_detect_cfg ABI layout");
static_assert(sizeof(sdrx_postfilter_cfg) == 16 && sizeof(PostCfg) == 16 && offsetof(sdrx_postfilter_cfg, reserved) == offsetof(PostCfg, reserved) &&
                  sizeof(sdrx_postfilter_info) == 40 && offsetof(sdrx_postfilter_info, delay_samples) == 16 && SDRX_POSTFILTER_MAX_TAPS == kPdMaxTaps &&
                  SDRX_POSTFILTER_MAX_DECIM == kPdMaxDecim,
              "sdrx_postfilter_cfg / sdrx_postfilter_info ABI layout");
static_assert(sizeof(sdrx_adc_arm) == 40 && sizeof(AdcArm) == 40 && offsetof(sdrx_adc_arm, longest_rail_run) == offsetof(AdcArm, longest_rail_run) &&
                  sizeof(sdrx_adc_meter) == 184 && sizeof(AdcRecord) == 184 && offsetof(sdrx_adc_meter, q) == offsetof(AdcRecord, q) &&
                  offsetof(sdrx_adc_meter, sum_iq) == offsetof(AdcRecord, sum_iq) && offsetof(sdrx_adc_meter, bits) == offsetof(AdcRecord, bits),
              "sdrx_adc_arm / sdrx_adc_meter ABI layout");

#include "sdrx_ctx.h"

namespace {
// kiss_fft's twiddles for nfft = 8192, then the display's Hann window (kSpecN floats), from the reference's own double
// expressions: what k_spectrum and k_watch_psd read.
std::vector<float2> spectrum_tables()
{
    std::vector<float2> tab((size_t)kSpecN + kSpecN / 2);
    const double pi = 3.141592653589793238462643383279502884197169399375105820974944; // kiss_fft.c:355-363
    for (int i = 0; i < kSpecN; ++i) {
        const double phase = -2 * pi * i / kSpecN;
        tab[(size_t)i] = make_float2((float)cos(phase), (float)sin(phase));
    }
    float *hann = reinterpret_cast<float *>(tab.data() + kSpecN); // mainwindow.cpp:284-287
    for (int i = 0; i < kSpecN; ++i)
        hann[i] = (float)(0.5 * (1.0 - cos(2 * SDRX_PI * ((float)i) / (kSpecN - 1.0))));
    return tab;
}
} // namespace

#include "sdrx_frame.hip"
#include "sdrx_delivery.hip"
#include "sdrx_watch.hip"
#include "sdrx_finalize.hip"
#include "sdrx_wake.hip"

namespace {

// Everything a context holds on the device and in pinned memory, released with the context's device current; the context is as
// before sdrx_finalize and its first uses.  What stays is host-side: the option dc.waves, the gate's events (sq.ev_dir) and its
// host copies, which squelch_setup sizes again, and the host's view of option park.
void free_device_state(sdrx_ctx *c)
{
    c->taps.clear();
    static_cast<CtxBuffers &>(*c) = CtxBuffers();
    static_cast<sdrx_ctx::DcDevice &>(c->dc) = sdrx_ctx::DcDevice();
    static_cast<sdrx_ctx::SquelchDevice &>(c->sq) = sdrx_ctx::SquelchDevice();
    static_cast<sdrx_ctx::ParkDevice &>(c->park) = sdrx_ctx::ParkDevice();
    c->agc = sdrx_ctx::Agc();
    c->spec = sdrx_ctx::Spectrum();
    c->watch = sdrx_ctx::Watch();
    c->drift = sdrx_ctx::Drift();
    c->scan = sdrx_ctx::Scan();
    c->wake = sdrx_ctx::Wake();
    c->adc = sdrx_ctx::Adc();
    static_cast<sdrx_ctx::ResamplerDevice &>(c->rs) = sdrx_ctx::ResamplerDevice();
    static_cast<sdrx_ctx::FrontDevice &>(c->fr) = sdrx_ctx::FrontDevice();
    static_cast<sdrx_ctx::BlankerDevice &>(c->bl) = sdrx_ctx::BlankerDevice();
    static_cast<sdrx_ctx::IqDevice &>(c->iq) = sdrx_ctx::IqDevice();
    static_cast<sdrx_ctx::ShiftDevice &>(c->sh) = sdrx_ctx::ShiftDevice();
    static_cast<sdrx_ctx::NotchDevice &>(c->nt) = sdrx_ctx::NotchDevice();
    c->route = sdrx_ctx::IngestRoute();
}

// ---- What the setters and getters of the ingest stages with settings and a record share (sdrx_ctx::CfgStage) -------------------------
// `what`: the call's name; `noun`: the stage's, as the messages say it -- "blanker", "IQ balance correction", "frequency shift",
// "spur canceller".  The order of the checks decides which code a call that is wrong twice gets.
constexpr int kStageOff = 1; // stage_set_entry: the call switched the stage off and is finished

// Entry of a setter: an error code, kStageOff (`cfg` null before sdrx_finalize), or SDRX_OK: go on to the stage's argument check
template <class S>
int stage_set_entry(sdrx_ctx *c, S sdrx_ctx::*stage, const void *cfg, const char *what, const char *noun)
{
    if (!c)
        return SDRX_EINVAL;
    if (c->finalized && !(c->*stage).on)
        return fail(c, SDRX_ESTATE, "%s: the %s was not switched on before sdrx_finalize", what, noun);
    if (!cfg) {
        if (c->finalized)
            return fail(c, SDRX_ESTATE, "%s: the %s is switched off before sdrx_finalize only", what, noun);
        (c->*stage).on = false;
        return kStageOff;
    }
    return SDRX_OK;
}

// A setter on a finalized context works between two frames: every frame handed over ran with the settings it was launched with
int stage_set_between_frames(sdrx_ctx *c, const char *what)
{
    if (c->in_flight > 0)
        return fail(c, SDRX_ESTATE, "%s: %d submitted frame(s) not yet delivered -- call sdrx_wait first", what, c->in_flight);
    HIPCHK(c, hipSetDevice(c->device));
    return drain(c);
}

// A getter: the settings the delivered frame ran with -- `cfg_as_written`: the settings as last written, which need no delivered
// frame -- and its record of type Rec; `arrived`: whether the record's slot was ever written (a slot never written holds zeros).
// `what` is "sdrx_get_<stage>": the setter's name is made from it.
template <class Rec, class S, class CfgOut, class RecOut, class Arrived>
int stage_get(sdrx_ctx *c, S sdrx_ctx::*stage, CfgOut *cfg_out, RecOut *out, const char *what, const char *noun, bool cfg_as_written, Arrived arrived)
{
    if (!c)
        return SDRX_EINVAL;
    if (!c->finalized)
        return fail(c, SDRX_ESTATE, "%s before sdrx_finalize", what);
    const S &st = c->*stage;
    if (!st.on)
        return fail(c, SDRX_ESTATE, "%s: no %s set (sdrx_set_%s before sdrx_finalize)", what, noun, what + strlen("sdrx_get_"));
    if (!cfg_out && !out)
        return fail(c, SDRX_EINVAL, "%s: null output pointers", what);
    if (cfg_as_written && cfg_out) {
        memcpy(cfg_out, &st.cfg, sizeof *cfg_out);
        if (!out)
            return SDRX_OK;
    }
    if (int rc = need_delivered(c, what))
        return rc;
    const int p = c->host_slot;
    if (!st.used[p].any || st.used[p].frame != c->host_frame)
        return fail(c, SDRX_EHIP, "%s: frame %llu did not pass the %s", what, c->host_frame, noun);
    if (cfg_out && !cfg_as_written)
        memcpy(cfg_out, &st.used[p].cfg, sizeof *cfg_out);
    if (out) {
        memcpy(out, st.rec.template host<Rec>(p), sizeof *out);
        if (!arrived(*out) || out->frame != (int64_t)c->host_frame)
            return fail(c, SDRX_EHIP, "%s: the record of frame %llu did not arrive (it names frame %lld)", what, c->host_frame, (long long)out->frame);
    }
    return SDRX_OK;
}

} // namespace

// ================================================================================ C ABI
extern "C" {

int sdrx_abi_version(void) { return SDRX_ABI_VERSION; }

#ifndef SDRX_SOURCE_HASH
#define SDRX_SOURCE_HASH "unknown"
#endif
const char *sdrx_build_id(void) { return SDRX_SOURCE_HASH; }

const char *sdrx_last_error(const sdrx_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

const char *sdrx_kernel_name(int kind) { return kind >= 0 && kind < SDRX_NKERNELS ? kKindNames[kind] : ""; }

int sdrx_create(sdrx_ctx **out, int device)
{
    if (!out)
        return fail(nullptr, SDRX_EINVAL, "sdrx_create: null output pointer");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, SDRX_EHIP, "sdrx_create: no HIP device (%s); libsdrx has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev)
        return fail(nullptr, SDRX_EINVAL, "sdrx_create: device %d out of range (0..%d)", device, ndev - 1);
    e = hipSetDevice(device);
    if (e != hipSuccess)
        return fail(nullptr, SDRX_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
    sdrx_ctx *c = new sdrx_ctx();
    c->device = device;
    e = hipStreamCreateWithFlags(&c->st.own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(nullptr, SDRX_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    c->st.stream = c->st.own_stream;
    // odd frames' payloads leave on a copy stream of their own: the next copy's set-up then overlaps the
    // current copy's tail (measured through the ABI on config 3: 0.296 vs 0.306 ms per frame)
    bool ok = hipStreamCreateWithFlags(&c->st.tail_stream, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&c->st.copy_stream, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&c->st.copy_stream2, hipStreamNonBlocking) == hipSuccess;
    for (int p = 0; p < 2 && ok; ++p)
        ok = hipEventCreateWithFlags(&c->st.ev_levels[p], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->st.ev_tail[p], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->st.ev_copied[p], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->st.ev_staged[p], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        sdrx_destroy(c);
        return fail(nullptr, SDRX_EHIP, "sdrx_create: could not create the streams / events of the context");
    }
    *out = c;
    return SDRX_OK;
}

int sdrx_destroy(sdrx_ctx *c)
{
    if (!c)
        return SDRX_EINVAL;
    (void)hipSetDevice(c->device);
    for (hipStream_t st : {c->st.stream, c->st.tail_stream, c->st.copy_stream, c->st.copy_stream2})
        if (st)
            (void)hipStreamSynchronize(st);
    drain_events(c);
    for (hipEvent_t e : c->tm.pool)
        (void)hipEventDestroy(e);
    for (auto *v : {&c->shared_readers[0], &c->shared_readers[1]})
        for (const auto &r : *v)
            (void)hipEventDestroy(r.ev);
    for (int p = 0; p < 2; ++p)
        for (hipEvent_t e : {c->st.ev_levels[p], c->st.ev_tail[p], c->st.ev_copied[p], c->st.ev_staged[p], c->sq.ev_dir[p]})
            if (e)
                (void)hipEventDestroy(e);
    free_device_state(c);
    for (hipStream_t st : {c->st.own_stream, c->st.tail_stream, c->st.copy_stream, c->st.copy_stream2})
        if (st)
            (void)hipStreamDestroy(st);
    delete c;
    return SDRX_OK;
}

int sdrx_set_option(sdrx_ctx *c, const char *name, int value)
{
    if (!c || !name)
        return SDRX_EINVAL;
    if (c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_set_option after sdrx_finalize");
    if (!strcmp(name, "exact"))
        c->opt_exact = value == 2 ? 2 : value != 0; // 1 exact (default) | 0 tolerance | 2 robust
    else if (!strcmp(name, "keep_prequant"))
        c->opt_prequant = value != 0;
    else if (!strcmp(name, "segments"))
        c->opt_segments = value < 0 ? 0 : value;
    else if (!strcmp(name, "dc_blocked_scan"))
        c->opt_dc_blocked = value != 0;
    else if (!strcmp(name, "dc_speculative"))
        c->opt_dc_speculative = value != 0;
    else if (!strcmp(name, "dc_blocks_per_step")) {
        if (value != 1 && value != 2 && value != 4 && value != 8)
            return fail(c, SDRX_EINVAL, "dc_blocks_per_step: 1, 2, 4 or 8");
        c->dc.waves = value;
    }
    else if (!strcmp(name, "pipeline"))
        c->opt_pipeline = value != 0;
    else if (!strcmp(name, "fuse"))
        c->opt_fuse = value != 0;
    else if (!strcmp(name, "frame_pipeline"))
        c->opt_frame_pipeline = value != 0;
    else if (!strcmp(name, "fuse_late"))
        c->opt_fuse_late = value != 0;
    else if (!strcmp(name, "keep_streams"))
        c->opt_keep_streams = value != 0;
    else if (!strcmp(name, "fuse_demod"))
        c->opt_fuse_demod = value != 0;
    else if (!strcmp(name, "tail_in_levels"))
        c->opt_tail_in_levels = value != 0;
    else if (!strcmp(name, "meter"))
        c->opt_meter = value != 0;
    else if (!strcmp(name, "squelch"))
        c->opt_squelch = value != 0;
    else if (!strcmp(name, "preroll"))
        c->opt_preroll = value != 0;
    else if (!strcmp(name, "squelch_auto"))
        c->opt_squelch_auto = value != 0;
    else if (!strcmp(name, "park"))
        c->opt_park = value != 0;
    else if (!strcmp(name, "watch"))
        c->opt_watch = value != 0;
    else if (!strcmp(name, "catchup"))
        c->opt_catchup = value != 0;
    else if (!strcmp(name, "agc"))
        c->opt_agc = value != 0;
    else if (!strcmp(name, "wake"))
        c->opt_wake = value != 0;
    else if (!strcmp(name, "adc_meter"))
        c->opt_adc_meter = value != 0;
    else
        return fail(c, SDRX_EINVAL, "unknown option '%s'", name);
    return SDRX_OK;
}

int sdrx_add_vfo(sdrx_ctx *c, const sdrx_vfo_desc *d, int *id_out)
{
    if (!c || !d)
        return SDRX_EINVAL;
    if (c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_add_vfo after sdrx_finalize");
    const int id = (int)c->nodes.size();
    if (d->parent_id >= id || d->parent_id < -1)
        return fail(c, SDRX_EINVAL, "vfo %d: parent_id %d must name an earlier vfo or be -1", id, d->parent_id);
    if (d->decimate_count < 0 || d->decimate_count > kMaxStages)
        return fail(c, SDRX_EINVAL, "vfo %d: decimate_count %d outside 0..8 (vfo.h:63)", id, d->decimate_count);
    if (d->fs <= 0 || d->samples_per_buffer <= 0)
        return fail(c, SDRX_EINVAL, "vfo %d: fs and samples_per_buffer must be positive", id);
    if (d->late_decimate < 0 || d->late_decimate == 1)
        return fail(c, SDRX_EINVAL, "vfo %d: late_decimate must be 0 or >= 2 (the reference uses 5 and 6)", id);
    if (d->parent_id >= 0 && c->nodes[(size_t)d->parent_id].d.demod_usb)
        return fail(c, SDRX_EINVAL, "vfo %d: parent %d is a USB leaf", id, d->parent_id);
    Node n;
    n.d = *d;
    c->nodes.push_back(n);
    if (d->parent_id >= 0)
        c->nodes[(size_t)d->parent_id].children.push_back(id);
    if (id_out)
        *id_out = id;
    return SDRX_OK;
}

int sdrx_check_vfo(const sdrx_vfo_desc *d, char *msg, size_t cap)
{
    auto say = [&](int code, const char *fmt, ...) {
        if (msg && cap) {
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(msg, cap, fmt, ap);
            va_end(ap);
        }
        return code;
    };
    if (!d)
        return SDRX_EINVAL;
    if (msg && cap)
        msg[0] = 0;
    if (d->decimate_count < 0 || d->decimate_count > kMaxStages)
        return say(SDRX_EINVAL, "decimate_count %d outside 0..8 (vfo.h:63)", d->decimate_count);
    if (d->fs <= 0 || d->samples_per_buffer <= 0)
        return say(SDRX_EINVAL, "fs and samples_per_buffer must be positive");
    if (d->late_decimate < 0 || d->late_decimate == 1)
        return say(SDRX_EINVAL, "late_decimate must be 0 or >= 2 (the reference uses 5 and 6)");
    // the order of vfo::init (vfo.cpp:60-124): late-decimation low-pass first, then the audio low-pass
    int target = (int)(d->fs / std::pow(2, d->decimate_count));
    if (d->demod_usb && d->late_decimate > 0) {
        target /= d->late_decimate;
        if (const char *why = low_pass_rejection((double)target * d->late_decimate, (double)(target / 2), (double)target / (d->late_decimate - 1)))
            return say(SDRX_EFILTER, "%s", why);
    }
    if (d->filter_bw_hz > 0) // (vfo::init designs this filter for ANY vfo with filterbw > 0, vfo.cpp:106-124, USB or not)
        if (const char *why = low_pass_rejection((double)target, (double)d->filter_bw_hz, (double)d->filter_bw_hz / 4))
            return say(SDRX_EFILTER, "%s", why);
    if (d->fs % kRun || d->samples_per_buffer % kRun || d->fs < kChunk)
        return say(SDRX_EUNSUPPORTED, "fs (%d) and samples_per_buffer (%d) must be multiples of 16 and fs >= 1024", d->fs, d->samples_per_buffer);
    if (d->samples_per_buffer % (1 << d->decimate_count))
        return say(SDRX_EUNSUPPORTED, "samples_per_buffer %d not a multiple of 2^%d", d->samples_per_buffer, d->decimate_count);
    return SDRX_OK;
}

int sdrx_set_publish_callback(sdrx_ctx *c, sdrx_publish_fn fn, void *user)
{
    if (!c)
        return SDRX_EINVAL;
    c->cb = fn;
    c->cb_user = user;
    return SDRX_OK;
}

} // extern "C"


extern "C" {

int sdrx_finalize(sdrx_ctx *c)
{
    if (!c)
        return SDRX_EINVAL;
    if (c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_finalize called twice");
    if (c->nodes.empty())
        return fail(c, SDRX_ESTATE, "sdrx_finalize: no VFOs");
    HIPCHK(c, hipSetDevice(c->device));
    const int asked_squelch = c->opt_squelch, asked_meter = c->opt_meter, asked_preroll = c->opt_preroll, asked_park = c->opt_park;
    const int asked_watch = c->opt_watch;
    if (c->opt_wake) // the device parks and unparks the leaves the watch measures
        c->opt_park = c->opt_watch = 1;
    if (c->opt_catchup) // the caught-up frame of an unparked leaf leaves through the pre-roll path
        c->opt_park = c->opt_preroll = 1;
    if (c->opt_preroll || c->opt_squelch_auto) // the pre-roll and the floor tracking are the gate's
        c->opt_squelch = 1;
    if (c->opt_squelch || c->opt_agc) // the gate and the gain step read the meter records
        c->opt_meter = 1;
    const int rc = finalize_impl(c);
    if (rc != SDRX_OK) { // nothing of a half-built tree stays behind: a later call starts clean -- with the options as they
                         // were SET, not as this attempt implied them (the caller may switch "preroll" off and try again)
        (void)hipStreamSynchronize(c->st.stream);
        free_device_state(c);
        c->l1.clear();
        c->lb.clear();
        c->publish_order.clear();
        c->opt_squelch = asked_squelch;
        c->opt_meter = asked_meter;
        c->opt_preroll = asked_preroll;
        c->opt_park = asked_park;
        c->opt_watch = asked_watch;
    }
    return rc;
}

namespace {
// The descriptors of the enabled spectra, uploaded whenever what they point at changes (sdrx_set_spectrum, the taps): the VFO
// spectra whose stream exists -- where sdrx_get_stream finds it, by tree level -- then the raw one.  Synchronous: never inside
// a frame call.
int spectrum_rebuild(sdrx_ctx *c)
{
    if (c->spec.slots.empty())
        return SDRX_OK;
    const int N = (int)c->nodes.size();
    std::vector<SpecDesc> d;
    c->spec.level_begin.assign((size_t)c->n_levels + 1, 0);
    for (int lv = 0; lv < c->n_levels; ++lv) {
        c->spec.level_begin[(size_t)lv] = (int)d.size();
        for (int id = 0; id < N; ++id) {
            const Node &n = c->nodes[(size_t)id];
            const auto tap = c->taps.find(id);
            if (n.level != lv || !c->spec.slots[(size_t)id].on || (!n.has_stream && tap == c->taps.end()))
                continue;
            if (leaf_parked_at(c, id, c->frame_no)) // a parked leaf writes no stream: no update (its display state stays)
                continue;
            SpecDesc e;
            memset(&e, 0, sizeof e);
            for (int p = 0; p < 2; ++p) {
                if (!n.has_stream)
                    e.src[p] = tap->second.buf[p];
                else if (n.leaf)
                    e.src[p] = reinterpret_cast<const float2 *>(c->arena + n.off_stream[p]) + n.Hx;
                else
                    e.src[p] = reinterpret_cast<const float2 *>(c->arena + n.off_stream[p]);
            }
            e.kind = n.has_stream && !n.leaf ? kSpecTiled : kSpecNatural;
            e.n_in = std::min(n.n_f, kSpecN);
            e.level = std::min(lv, kMaxLevels - 1); // (only the frame pipeline, at most kMaxLevels deep, has frames per level)
            e.pwr = c->spec.slots[(size_t)id].pwr;
            e.bins = reinterpret_cast<float2 *>(e.pwr + kSpecN);
            e.rec = c->spec.d_rec + id;
            d.push_back(e);
        }
    }
    c->spec.level_begin[(size_t)c->n_levels] = (int)d.size();
    c->spec.n_desc = (int)d.size();
    c->spec.raw_on = c->spec.slots[(size_t)N].on;
    if (c->spec.raw_on) {
        SpecDesc e;
        memset(&e, 0, sizeof e);
        e.kind = kSpecRaw;
        e.n_in = std::min(c->root_frame, kSpecN);
        e.pwr = c->spec.slots[(size_t)N].pwr;
        e.bins = reinterpret_cast<float2 *>(e.pwr + kSpecN);
        e.rec = c->spec.d_rec + N;
        d.push_back(e);
    }
    if (!d.empty())
        HIPCHK(c, hipMemcpy(c->spec.d_desc, d.data(), sizeof(SpecDesc) * d.size(), hipMemcpyHostToDevice));
    return SDRX_OK;
}
} // namespace

// The reference's fftVFOSlot(topic) (vfo.cpp:492-509): from the next frame on, decimate[decimateCount] of node `id` is what
// sdrx_get_stream serves.  Every VFO keeps that stream in HBM anyway -- except a leaf whose late decimation runs inside the
// mix wave (it writes only the decimated stream): for such a leaf this call makes the wave keep decimate[0] as well.
// sdrx_set_tap REPLACES the selection (id = -1: none), sdrx_add_tap adds to it: fftVFOSlot sets emitFFT on every VFO whose
// topic equals the selected string, so two VFOs with one topic are two taps.
static int tap_change_impl(sdrx_ctx *c, int id, bool replace, const char *what);
static int tap_change(sdrx_ctx *c, int id, bool replace, const char *what)
{
    const int rc = tap_change_impl(c, id, replace, what);
    const int rc2 = c && c->finalized ? spectrum_rebuild(c) : SDRX_OK; // a fused leaf's spectrum follows its tap buffer
    return rc ? rc : rc2;
}
static int tap_change_impl(sdrx_ctx *c, int id, bool replace, const char *what)
{
    if (!c)
        return SDRX_EINVAL;
    if (!c->finalized)
        return fail(c, SDRX_ESTATE, "%s before sdrx_finalize", what);
    if (id < (replace ? -1 : 0) || id >= (int)c->nodes.size())
        return fail(c, SDRX_EINVAL, "bad vfo id %d", id);
    if (c->in_flight > 0)
        return fail(c, SDRX_ESTATE, "%s: %d submitted frame(s) not yet delivered -- call sdrx_wait first", what, c->in_flight);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c)) // frames inside the software pipeline run to their end with the taps they were queued under
        return rc;
    auto point = [&](int node, float2 *b0, float2 *b1) -> hipError_t { // K1Vfo::tap of `node` (synchronous: the pointers live on this stack)
        float2 *ptrs[2] = {b0, b1};
        return hipMemcpy(c->arena + c->off_k1vfo + sizeof(K1Vfo) * (size_t)node + offsetof(K1Vfo, tap), ptrs, sizeof ptrs, hipMemcpyHostToDevice);
    };
    if (replace) {
        for (auto it = c->taps.begin(); it != c->taps.end();) {
            if (it->first == id) { // stays what it is (and keeps serving the frames it has)
                ++it;
                continue;
            }
            HIPCHK(c, point(it->first, nullptr, nullptr));
            it = c->taps.erase(it);
        }
    }
    if (id < 0 || c->nodes[(size_t)id].has_stream || c->taps.count(id))
        return SDRX_OK; // every other node keeps decimate[d] in HBM anyway
    sdrx_ctx::TapBuf t;
    t.since = c->frame_no;
    bool arena_free = c->tap_len > 0;
    for (const auto &kv : c->taps)
        arena_free = arena_free && kv.second.own[0];
    if (arena_free) {
        for (int p = 0; p < 2; ++p)
            t.buf[p] = reinterpret_cast<float2 *>(c->arena + c->off_tapbuf[p]);
    } else {
        for (int p = 0; p < 2; ++p) {
            if (t.own[p].alloc((size_t)c->nodes[(size_t)id].n_f) != hipSuccess)
                return fail(c, SDRX_ENOMEM, "%s: no device memory for another tap buffer", what);
            t.buf[p] = t.own[p];
        }
    }
    HIPCHK(c, point(id, t.buf[0], t.buf[1]));
    c->taps.emplace(id, std::move(t));
    return SDRX_OK;
}

int sdrx_set_tap(sdrx_ctx *c, int id) { return tap_change(c, id, true, "sdrx_set_tap"); }
int sdrx_add_tap(sdrx_ctx *c, int id) { return tap_change(c, id, false, "sdrx_add_tap"); }

} // extern "C"

namespace {

// The checks of sdrx_set_mixer_freqs / sdrx_set_gains: the whole list before anything changes.
// Returns SDRX_OK or SDRX_EINVAL with the reason in `msg`.
int check_vfo_list(int n_nodes, const int *ids, const void *vals, bool dbl, int n, std::string &msg)
{
    char buf[160];
    if (n < 0 || (n > 0 && (!ids || !vals))) {
        snprintf(buf, sizeof buf, "bad list (n = %d)", n);
        msg = buf;
        return SDRX_EINVAL;
    }
    std::vector<char> seen((size_t)n_nodes, 0);
    for (int k = 0; k < n; ++k) {
        const int id = ids[k];
        const double v = dbl ? static_cast<const double *>(vals)[k] : (double)static_cast<const float *>(vals)[k];
        buf[0] = 0;
        if (id < 0 || id >= n_nodes)
            snprintf(buf, sizeof buf, "bad vfo id %d (entry %d)", id, k);
        else if (seen[(size_t)id]++)
            snprintf(buf, sizeof buf, "vfo %d listed twice", id);
        else if (!std::isfinite(v))
            snprintf(buf, sizeof buf, "vfo %d: value is not finite", id);
        if (buf[0]) {
            msg = buf;
            return SDRX_EINVAL;
        }
    }
    return SDRX_OK;
}

// Applies a checked list: drain the software pipeline (frames queued earlier finish with the old values), then one upload of
// the job list and one k_vfo_retune launch.  The host copies of every node follow.
int apply_vfo_jobs(sdrx_ctx *c, const int *ids, const double *freqs, const float *gains, int n)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    std::vector<RetuneJob> jobs;
    jobs.reserve((size_t)n * 2);
    K1Vfo *k1 = reinterpret_cast<K1Vfo *>(c->arena + c->off_k1vfo);
    for (int k = 0; k < n; ++k) {
        const Node &nd = c->nodes[(size_t)ids[k]];
        RetuneJob J;
        memset(&J, 0, sizeof J);
        if (freqs) {
            J.kind = kJobRetune;
            J.vfo = k1 + ids[k];
            nco_rotation((double)nd.d.fs, freqs[k], J.rot_re, J.rot_im);
            nco_powers(J.rot_re, J.rot_im, J.rk);
            J.origin = c->frame_no;
            jobs.push_back(J);
            continue;
        }
        J.kind = kJobGain;
        J.value = gains[k];
        if (nd.d2_index >= 0) {
            J.gain = &(reinterpret_cast<K2Vfo *>(c->arena + c->off_k2) + nd.d2_index)->gain;
            jobs.push_back(J);
        }
        if (nd.d4_index >= 0) {
            J.gain = &(reinterpret_cast<K4Vfo *>(c->arena + c->off_k4) + nd.d4_index)->gain;
            jobs.push_back(J);
        }
        if (nd.d5_index >= 0) {
            J.gain = &(reinterpret_cast<K5Vfo *>(c->arena + c->off_k5) + nd.d5_index)->gain;
            jobs.push_back(J);
        }
    }
    if (!jobs.empty()) {
        if (int rc = upload_jobs(c, c->d_jobs, jobs.data(), jobs.size()))
            return rc;
        const int nj = (int)jobs.size();
        hipLaunchKernelGGL(k_vfo_retune, dim3((nj + 63) / 64), dim3(64), 0, c->st.stream, c->d_jobs, nj);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->st.stream)); // (`jobs` lives on this stack)
    }
    for (int k = 0; k < n; ++k) {
        Node &nd = c->nodes[(size_t)ids[k]];
        if (freqs) {
            nd.d.mixer_freq_hz = freqs[k];
            nco_rotation((double)nd.d.fs, freqs[k], nd.rot_re, nd.rot_im);
        } else {
            nd.d.gain = gains[k];
        }
    }
    return freqs ? watch_retuned(c, ids, n) : SDRX_OK; // (a watched leaf's band follows its mixer)
}

int set_vfo_values(sdrx_ctx *c, const int *ids, const double *freqs, const float *gains, int n, const char *what)
{
    if (!c)
        return SDRX_EINVAL;
    if (!c->finalized)
        return fail(c, SDRX_ESTATE, "%s before sdrx_finalize", what);
    std::string msg;
    if (check_vfo_list((int)c->nodes.size(), ids, freqs ? (const void *)freqs : (const void *)gains, freqs != nullptr, n, msg))
        return fail(c, SDRX_EINVAL, "%s: %s", what, msg.c_str());
    if (c->in_flight > 0)
        return fail(c, SDRX_ESTATE, "%s: %d submitted frame(s) not yet delivered -- call sdrx_wait first", what, c->in_flight);
    if (n == 0)
        return SDRX_OK;
    return apply_vfo_jobs(c, ids, freqs, gains, n);
}

} // namespace

extern "C" {

int sdrx_set_mixer_freqs(sdrx_ctx *c, const int *ids, const double *mixer_freq_hz, int n)
{
    return set_vfo_values(c, ids, mixer_freq_hz, nullptr, n, "sdrx_set_mixer_freqs");
}

int sdrx_set_gains(sdrx_ctx *c, const int *ids, const float *gains, int n)
{
    return set_vfo_values(c, ids, nullptr, gains, n, "sdrx_set_gains");
}

} // extern "C"

namespace {

// sdrx_set_active on a checked list: the entries that change a leaf's state become fill jobs (FillJob: its flag words; for a
// leaf that is unparked also zeros over every filter-state region of both frame parities and the gate state of sdrx_finalize)
// and, for an unparked leaf, one retune job with the rotation it has (a fresh Oscillator from the next frame on).  The
// software pipeline is drained first; one upload, k_vfo_reset and k_vfo_retune, one synchronisation.
// Option catchup: a leaf with a parent that was parked in frame K-1 (K = the next frame, K >= 1) starts at K-1 instead -- its
// oscillator's origin is K-1 and prev_open = 0 -- and runs that frame behind the two launches: its own mix items in one
// k_mix_decimate launch per tree level, then its own blocks of every block kernel, the sub-lists uploaded with the jobs.  They
// read the parent's decimate[d] of K-1 where it lies (parity (K-1) & 1: untouched until frame K+1) and write the leaf's
// ordinary buffers of that parity; the gate of K then pre-rolls the payload (pre = open && !prev_open).  The leaf's meter
// records of K-1 come back before the call returns (sdrx_get_catchup).
int apply_active(sdrx_ctx *c, const int *ids, const int32_t *active, int n)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    sdrx_ctx::Park &K = c->park;
    std::vector<FillJob> fills;
    std::vector<RetuneJob> tunes;
    auto fill = [&](void *ptr, size_t words, unsigned value) {
        if (words)
            fills.push_back(FillJob{static_cast<unsigned *>(ptr), (unsigned)words, value});
    };
    K1Vfo *k1 = reinterpret_cast<K1Vfo *>(c->arena + c->off_k1vfo);
    bool any_spectrum = false;
    std::vector<int> caught; // option catchup: the leaves that start one frame back
    for (int k = 0; k < n; ++k) {
        const int id = ids[k];
        const Node &nd = c->nodes[(size_t)id];
        if (K.leaf[(size_t)id].active == active[k]) // already there: no reset
            continue;
        const bool catch_up = c->opt_catchup && active[k] && nd.d.parent_id >= 0 && c->frame_no >= 1 && K.parked_at(id, c->frame_no - 1);
        if (catch_up)
            caught.push_back(id);
        // the leaf's flag words; for a leaf that is unparked also what makes it a new vfo (caught up: no gate ran on K-1, and
        // the gate of K finds the leaf "closed before")
        leaf_regions(c, id, catch_up ? 0u : 1u, [&](void *ptr, size_t words, unsigned v_on, unsigned v_off, bool wake_only) {
            if (active[k])
                fill(ptr, words, v_on);
            else if (!wake_only)
                fill(ptr, words, v_off);
        });
        any_spectrum |= !c->spec.slots.empty() && c->spec.slots[(size_t)id].on;
        if (!active[k])
            continue;
        RetuneJob J;
        memset(&J, 0, sizeof J);
        J.kind = kJobRetune;
        J.vfo = k1 + id;
        J.rot_re = nd.rot_re;
        J.rot_im = nd.rot_im;
        nco_powers(J.rot_re, J.rot_im, J.rk);
        J.origin = catch_up ? c->frame_no - 1 : c->frame_no;
        tunes.push_back(J);
    }
    // the sub-lists of the catch-up, behind the jobs: K1Work[] per tree level, then per block kernel BlockWork[] (k_lpf_long
    // with option meter: and its blocks' record offsets)
    struct Sub {
        size_t off = 0, off_mrel = 0;
        int n = 0;
    };
    std::vector<Sub> sub_mix((size_t)c->n_levels), sub_blk(c->lb.size());
    std::vector<unsigned char> lists;
    auto append = [&](const void *src, size_t bytes) {
        const size_t o = align_up(lists.size(), 16);
        lists.resize(o + bytes);
        memcpy(lists.data() + o, src, bytes);
        return o;
    };
    if (!caught.empty()) {
        for (int lv = 1; lv < c->n_levels; ++lv) {
            std::vector<K1Work> w;
            for (int id : caught)
                if (c->nodes[(size_t)id].level == lv)
                    w.insert(w.end(), c->cu.leaf[(size_t)id].mix.begin(), c->cu.leaf[(size_t)id].mix.end());
            sub_mix[(size_t)lv].n = (int)w.size();
            if (!w.empty())
                sub_mix[(size_t)lv].off = append(w.data(), sizeof(K1Work) * w.size());
        }
        for (size_t q = 0; q < c->lb.size(); ++q) {
            const int slot = sdrx_ctx::Catchup::slot(c->lb[q].kind);
            std::vector<BlockWork> w;
            std::vector<int> mrel;
            for (int id : caught) {
                const sdrx_ctx::Catchup::Leaf &L = c->cu.leaf[(size_t)id];
                w.insert(w.end(), L.blk[slot].begin(), L.blk[slot].end());
                if (slot == 2)
                    mrel.insert(mrel.end(), L.mrel.begin(), L.mrel.end());
            }
            sub_blk[q].n = (int)w.size();
            if (!w.empty())
                sub_blk[q].off = append(w.data(), sizeof(BlockWork) * w.size());
            if (!mrel.empty())
                sub_blk[q].off_mrel = append(mrel.data(), sizeof(int) * mrel.size());
        }
    }
    if (!fills.empty()) {
        const size_t fb = sizeof(FillJob) * fills.size(), jb = align_up(fb + sizeof(RetuneJob) * tunes.size(), 16), bytes = jb + lists.size();
        std::vector<unsigned char> host(bytes);
        memcpy(host.data(), fills.data(), fb);
        if (!tunes.empty())
            memcpy(host.data() + fb, tunes.data(), sizeof(RetuneJob) * tunes.size());
        if (!lists.empty())
            memcpy(host.data() + jb, lists.data(), lists.size());
        if (int rc = upload_jobs(c, K.d_jobs, host.data(), bytes))
            return rc;
        hipLaunchKernelGGL(k_vfo_reset, dim3((unsigned)fills.size()), dim3(256), 0, c->st.stream, reinterpret_cast<const FillJob *>(K.d_jobs.get()));
        if (!tunes.empty()) {
            const int nj = (int)tunes.size();
            hipLaunchKernelGGL(k_vfo_retune, dim3((nj + 63) / 64), dim3(64), 0, c->st.stream, reinterpret_cast<const RetuneJob *>(K.d_jobs + fb), nj);
        }
        if (!caught.empty()) { // frame K-1 of the caught-up leaves: the levels, then the leaf tail, as a frame's own sequence
            const unsigned long long f = c->frame_no - 1;
            for (const Launch1 &L : c->l1)
                if (sub_mix[(size_t)L.level].n > 0)
                    launch_mix_list(c, L, f, reinterpret_cast<const K1Work *>(K.d_jobs + jb + sub_mix[(size_t)L.level].off), sub_mix[(size_t)L.level].n, nullptr,
                                    kRawTiled);
            for (size_t q = 0; q < c->lb.size(); ++q)
                if (sub_blk[q].n > 0)
                    launch_block_list(c, c->lb[q], c->st.stream, f, reinterpret_cast<const BlockWork *>(K.d_jobs + jb + sub_blk[q].off),
                                      c->opt_meter ? reinterpret_cast<const int *>(K.d_jobs + jb + sub_blk[q].off_mrel) : nullptr, sub_blk[q].n);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->st.stream)); // (`host` lives on this stack)
    }
    if (!caught.empty()) { // the caught-up frame's meter records: one copy of the span that holds them
        int lo = c->meter_slots, hi = 0;
        for (int id : caught) {
            lo = std::min(lo, c->nodes[(size_t)id].meter_first);
            hi = std::max(hi, c->nodes[(size_t)id].meter_first + c->nodes[(size_t)id].meter_n);
        }
        std::vector<unsigned char> rec(16 * (size_t)(hi - lo));
        HIPCHK(c, hipMemcpy(rec.data(), c->d_pay[(c->frame_no - 1) & 1ull] + c->meter_off + 16 * (size_t)lo, rec.size(), hipMemcpyDeviceToHost));
        for (int id : caught) {
            const Node &nd = c->nodes[(size_t)id];
            sdrx_ctx::Catchup::Leaf &U = c->cu.leaf[(size_t)id];
            U.frame = (long long)c->frame_no - 1;
            const MeterFold F = fold_meter_records(rec.data(), nd.meter_first - lo, nd.meter_n); // (as sdrx_get_meters folds them)
            U.sum_sq = F.sum_sq;
            U.clipped = F.clipped;
            U.peak = F.peak;
        }
    }
    for (int k = 0; k < n; ++k) {
        sdrx_ctx::Park::Leaf &L = K.leaf[(size_t)ids[k]];
        if (L.active == active[k])
            continue;
        if (c->opt_catchup && std::find(caught.begin(), caught.end(), ids[k]) == caught.end())
            c->cu.leaf[(size_t)ids[k]].frame = -1; // parked (a catch-up is discarded), or started at K as without the option
        if (L.since != c->frame_no) // (a second change before the same frame: the frames before it ran in the state they ran in)
            L.was_active = L.active;
        L.active = active[k];
        L.since = c->frame_no;
        if (active[k] && c->opt_squelch)
            c->sq.hang[(size_t)c->sq.index[(size_t)ids[k]]] = 0;
    }
    return any_spectrum ? spectrum_rebuild(c) : SDRX_OK; // (an enabled spectrum of a parked leaf leaves the launch list)
}

} // namespace

extern "C" {

int sdrx_set_active(sdrx_ctx *c, const int *ids, const int32_t *active, int n)
{
    const int rc = leaf_call(c, "sdrx_set_active", &sdrx_ctx::opt_park, "park", ids, active != nullptr, n, kBetweenFrames, [&](int k) {
        const char *why = bad_if_controlled(c, ids[k]);
        return why ? why : bad_switch(active[k]);
    });
    return rc || n == 0 ? rc : apply_active(c, ids, active, n);
}

int sdrx_get_active(sdrx_ctx *c, const int *ids, int n, sdrx_active_state *out)
{
    if (int rc = leaf_call(c, "sdrx_get_active", nullptr, nullptr, ids, out != nullptr, n, kAnyTime)) // (no option: every leaf is active without "park")
        return rc;
    for (int k = 0; k < n; ++k) {
        sdrx_active_state s;
        memset(&s, 0, sizeof s);
        s.active = 1;
        if (!c->park.leaf.empty()) {
            s.active = c->park.leaf[(size_t)ids[k]].active;
            s.since_frame = (int64_t)c->park.leaf[(size_t)ids[k]].since;
        }
        // a leaf under wake control: the state its newest frame ran in is a device result -- of the last frame, or with frames
        // in flight of the delivered one
        WakeRecord r;
        if (c->wake.controlled(ids[k]) && c->frame_no > 0) {
            bool have = false;
            if (c->in_flight > 0)
                have = c->host_slot >= 0 && wake_record(c, ids[k], c->host_frame, &r);
            else if (hipSetDevice(c->device) == hipSuccess && drain(c) == SDRX_OK)
                have = wake_record(c, ids[k], c->frame_no - 1, &r);
            if (have) {
                s.active = r.active;
                s.since_frame = r.since_frame;
            }
        }
        out[k] = s;
    }
    return SDRX_OK;
}

int sdrx_get_catchup(sdrx_ctx *c, const int *ids, int n, sdrx_meter *out)
{
    if (int rc = leaf_call(c, "sdrx_get_catchup", &sdrx_ctx::opt_catchup, "catchup", ids, out != nullptr, n, kAnyTime))
        return rc;
    for (int k = 0; k < n; ++k) {
        const Node &nd = c->nodes[(size_t)ids[k]];
        const sdrx_ctx::Catchup::Leaf &U = c->cu.leaf[(size_t)ids[k]];
        sdrx_meter m;
        memset(&m, 0, sizeof m);
        m.frame = -1;
        if (U.frame >= 0) {
            m.frame = (int64_t)U.frame;
            m.sum_sq = U.sum_sq;
            m.n_values = meter_n_values(nd);
            m.clipped = U.clipped;
            memcpy(&m.peak, &U.peak, 4);
        }
        out[k] = m;
    }
    return SDRX_OK;
}

int sdrx_set_stream(sdrx_ctx *c, void *s)
{
    if (!c)
        return SDRX_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = drain(c);
    if (rc)
        return rc;
    c->st.stream = s ? reinterpret_cast<hipStream_t>(s) : c->st.own_stream;
    return SDRX_OK;
}

} // extern "C"

extern "C" {

int sdrx_get_raw(sdrx_ctx *c, float *out, int max_complex, int *n_ret)
{
    if (!c || !out)
        return SDRX_EINVAL;
    if (!c->finalized || c->frame_no == 0)
        return fail(c, SDRX_ESTATE, "sdrx_get_raw: no frame processed yet");
    if (c->in_flight > 0)
        return fail(c, SDRX_ESTATE, "sdrx_get_raw: %d submitted frame(s) not yet delivered -- call sdrx_wait first", c->in_flight);
    if (c->last_raw < 0)
        return fail(c, SDRX_ESTATE, "sdrx_get_raw: the last frame was caller-owned device memory (sdrx_process_device)");
    HIPCHK(c, hipSetDevice(c->device));
    const int n = std::min(max_complex, c->root_frame);
    if (int rc = drain(c))
        return rc;
    if (c->last_raw == kRawF32) {
        HIPCHK(c, hipMemcpy(out, c->d_raw[(c->frame_no - 1) & 1ull], (size_t)n * sizeof(float2), hipMemcpyDeviceToHost));
    } else if (c->last_raw == kRawU8) { // floats[b] = b - 127, jonti/sdr.cpp:43-49
        std::vector<uint8_t> b((size_t)n * 2);
        HIPCHK(c, hipMemcpy(b.data(), c->d_raw_u8[(c->frame_no - 1) & 1ull], b.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < b.size(); ++i)
            out[i] = (float)((int)b[i] - 127);
    } else { // tile layout (the DC-bias kernels wrote it)
        const size_t total = align_up((size_t)c->root_frame, kChunk);
        std::vector<float2> t(total);
        HIPCHK(c, hipMemcpy(t.data(), c->d_raw_tiled, total * sizeof(float2), hipMemcpyDeviceToHost));
        untile(t.data(), out, n);
    }
    if (n_ret)
        *n_ret = n;
    return SDRX_OK;
}

// ---- Resampler (include/sdrx.h; sdrx_resample.h has the ratio, the frame lengths and the design) ------------------------------
static void resampler_info(const ResamplePlan &P, double passband_hz, sdrx_resampler_info *info)
{
    memset(info, 0, sizeof *info);
    info->fs_in = P.fs_in, info->fs_out = P.fs_out;
    info->L = P.L, info->M = P.M, info->taps_per_phase = P.T;
    info->in_frame = P.n_in, info->out_frame = P.n_out;
    info->delay_out_samples = resample_delay(P);
    info->passband_hz = passband_hz;
}

int sdrx_resampler_design(int32_t fs_in, int32_t fs_out, int32_t taps_per_phase, double atten_db, float *taps, int32_t cap, sdrx_resampler_info *info)
{
    ResamplePlan P;
    if (fs_in <= 0 || fs_out <= 0)
        return fail(nullptr, SDRX_EINVAL, "sdrx_resampler_design: sample rates must be positive");
    if (const char *why = resample_ratio(fs_in, fs_out, taps_per_phase, P))
        return fail(nullptr, SDRX_EUNSUPPORTED, "sdrx_resampler_design %d -> %d S/s: %s", fs_in, fs_out, why);
    if (taps && cap < P.L * P.T)
        return fail(nullptr, SDRX_EINVAL, "sdrx_resampler_design: room for %d taps, the prototype has L * T = %d", cap, P.L * P.T);
    double pass = 0;
    const int rc = resample_design(P, atten_db, taps, &pass);
    if (rc == 1)
        return fail(nullptr, SDRX_EINVAL, "sdrx_resampler_design: atten_db must be above 50 and at most 120");
    if (rc == 2)
        return fail(nullptr, SDRX_EFILTER, "sdrx_resampler_design %d -> %d S/s: with %d taps per phase the transition is wider than the band", fs_in, fs_out,
                    taps_per_phase);
    if (info)
        resampler_info(P, pass, info);
    return SDRX_OK;
}

int sdrx_set_resampler(sdrx_ctx *c, int32_t fs_in, const float *taps, int32_t taps_per_phase)
{
    if (!c)
        return SDRX_EINVAL;
    if (c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_set_resampler after sdrx_finalize");
    if (fs_in == 0) {
        static_cast<sdrx_ctx::Resampler &>(c->rs) = sdrx_ctx::Resampler();
        return SDRX_OK;
    }
    if (fs_in < 0 || !taps || taps_per_phase <= 0)
        return fail(c, SDRX_EINVAL, "sdrx_set_resampler: fs_in and taps_per_phase must be positive and taps not null");
    int fs_out = 0;
    for (const Node &n : c->nodes)
        if (n.d.parent_id < 0 && !fs_out)
            fs_out = n.d.fs;
    if (!fs_out)
        return fail(c, SDRX_ESTATE, "sdrx_set_resampler before the first parent-less VFO was added: its fs is the output rate");
    sdrx_ctx::Resampler R;
    R.on = true;
    if (const char *why = resample_ratio(fs_in, fs_out, taps_per_phase, R.plan))
        R.refused = why; // (sdrx_finalize says so: SDRX_EUNSUPPORTED)
    else
        R.taps.assign(taps, taps + (size_t)R.plan.L * R.plan.T);
    static_cast<sdrx_ctx::Resampler &>(c->rs) = std::move(R);
    return SDRX_OK;
}

int sdrx_get_resampler(sdrx_ctx *c, sdrx_resampler_info *info, float *taps, int32_t cap)
{
    if (!c)
        return SDRX_EINVAL;
    if (!c->rs.on)
        return fail(c, SDRX_ESTATE, "sdrx_get_resampler: no resampler set (sdrx_set_resampler)");
    if (!info || (taps && cap < 0))
        return fail(c, SDRX_EINVAL, "sdrx_get_resampler: null info or negative cap");
    resampler_info(c->rs.plan, c->rs.passband_hz, info);
    if (!c->finalized)
        info->in_frame = info->out_frame = 0;
    if (taps)
        std::copy(c->rs.taps.begin(), c->rs.taps.begin() + std::min((size_t)cap, c->rs.taps.size()), taps);
    return SDRX_OK;
}

int sdrx_get_resampler_input(sdrx_ctx *c, float *out, int32_t cap_complex)
{
    if (!c || !out)
        return SDRX_EINVAL;
    if (!c->rs.on)
        return fail(c, SDRX_ESTATE, "sdrx_get_resampler_input: no resampler set (sdrx_set_resampler)");
    if (!c->finalized || c->frame_no == 0)
        return fail(c, SDRX_ESTATE, "sdrx_get_resampler_input: no frame processed yet");
    if (c->in_flight > 0)
        return fail(c, SDRX_ESTATE, "sdrx_get_resampler_input: %d submitted frame(s) not yet delivered -- call sdrx_wait first", c->in_flight);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    const int n_in = c->rs.plan.n_in; // (not c->in_frame: a front stage in front of the resampler takes a longer frame)
    const int n = std::min((int)cap_complex, n_in);
    const size_t total = align_up((size_t)n_in, kChunk);
    std::vector<float2> t(total);
    HIPCHK(c, hipMemcpy(t.data(), c->rs.d_stage, total * sizeof(float2), hipMemcpyDeviceToHost));
    untile(t.data(), out, std::max(n, 0));
    return SDRX_OK;
}

// ---- Front stage (include/sdrx.h; sdrx_front.h has the frame lengths, the windows and the design) ------------------------------
static void front_info(const FrontPlan &P, double tw, sdrx_front_info *info)
{
    memset(info, 0, sizeof *info);
    info->real_input = P.real, info->stages = P.stages, info->K = P.K, info->N = front_taps(P.K);
    info->in_frame = P.in_frame, info->out_frame = P.n0;
    info->tw = tw;
    info->alias_free = tw > 0 ? 1.0 - 2.0 * tw : 0.0;
}

static int front_design_checked(sdrx_ctx *c, const char *what, int K, double atten_db, float *taps, double *tw)
{
    const int rc = front_design(K, atten_db, taps, tw);
    if (rc == 1)
        return fail(c, SDRX_EINVAL, "%s: atten_db must be above 50 and at most 120", what);
    if (rc == 2)
        return fail(c, SDRX_EFILTER, "%s: with K = %d (N = %d taps) at %g dB the transition is wider than the band", what, K, front_taps(K), atten_db);
    return SDRX_OK;
}

int sdrx_front_design(int32_t K, double atten_db, float *taps, int32_t cap, sdrx_front_info *info)
{
    if (K < kFrMinK || K > kFrMaxK)
        return fail(nullptr, SDRX_EINVAL, "sdrx_front_design: K must be in 2 .. 31 (N = 4 K + 3 taps)");
    if (taps && cap < front_taps(K))
        return fail(nullptr, SDRX_EINVAL, "sdrx_front_design: room for %d taps, the prototype has N = %d", cap, front_taps(K));
    double tw = 0;
    if (int rc = front_design_checked(nullptr, "sdrx_front_design", K, atten_db, taps, &tw))
        return rc;
    if (info) {
        FrontPlan P;
        P.K = K;
        front_info(P, tw, info);
    }
    return SDRX_OK;
}

int sdrx_set_front(sdrx_ctx *c, int32_t real_input, int32_t stages, const float *taps, int32_t K, double atten_db)
{
    if (!c)
        return SDRX_EINVAL;
    if (c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_set_front after sdrx_finalize");
    if (stages == 0) {
        static_cast<sdrx_ctx::Front &>(c->fr) = sdrx_ctx::Front();
        return SDRX_OK;
    }
    bool root = false;
    for (const Node &n : c->nodes)
        root = root || n.d.parent_id < 0;
    if (!root)
        return fail(c, SDRX_ESTATE, "sdrx_set_front before the first parent-less VFO was added");
    if (const char *why = front_args(real_input, stages, K))
        return fail(c, SDRX_EINVAL, "sdrx_set_front: %s", why);
    sdrx_ctx::Front F;
    F.on = true;
    F.plan.real = real_input, F.plan.stages = stages, F.plan.K = K;
    F.taps.resize((size_t)front_taps(K));
    if (taps) {
        const int bad = front_bad_tap(taps, K);
        if (bad >= 0)
            return fail(c, SDRX_EINVAL, "sdrx_set_front: h[%d] must be +0.0f (every odd k but the centre %d is a zero of the half-band)", bad, front_centre(K));
        std::copy(taps, taps + F.taps.size(), F.taps.begin());
    } else if (int rc = front_design_checked(c, "sdrx_set_front", K, atten_db, F.taps.data(), &F.tw)) {
        return rc;
    }
    static_cast<sdrx_ctx::Front &>(c->fr) = std::move(F);
    return SDRX_OK;
}

int sdrx_get_front(sdrx_ctx *c, sdrx_front_info *info, float *taps, int32_t cap)
{
    if (!c)
        return SDRX_EINVAL;
    if (!c->fr.on)
        return fail(c, SDRX_ESTATE, "sdrx_get_front: no front stage set (sdrx_set_front)");
    if (!info || (taps && cap < 0))
        return fail(c, SDRX_EINVAL, "sdrx_get_front: null info or negative cap");
    front_info(c->fr.plan, c->fr.tw, info);
    if (!c->finalized)
        info->in_frame = info->out_frame = 0;
    if (taps)
        std::copy(c->fr.taps.begin(), c->fr.taps.begin() + std::min((size_t)cap, c->fr.taps.size()), taps);
    return SDRX_OK;
}

// ---- Impulse blanker (include/sdrx.h; sdrx_blank.h has the rules) ----------------------------------------------------------------
int sdrx_set_blanker(sdrx_ctx *c, const sdrx_blanker_cfg *cfg)
{
    if (int rc = stage_set_entry(c, &sdrx_ctx::bl, cfg, "sdrx_set_blanker", "blanker"))
        return rc == kStageOff ? SDRX_OK : rc;
    if (const char *why = blank_args(cfg->ratio, cfg->floor, cfg->rank_q16, cfg->guard))
        return fail(c, SDRX_EINVAL, "sdrx_set_blanker: %s", why);
    if (c->finalized)
        if (int rc = stage_set_between_frames(c, "sdrx_set_blanker"))
            return rc;
    c->bl.on = true;
    c->bl.cfg = BlankCfg{cfg->ratio, cfg->floor, cfg->rank_q16, cfg->guard, {0, 0, 0, 0}};
    return SDRX_OK;
}

int sdrx_get_blanker(sdrx_ctx *c, sdrx_blanker_cfg *cfg_out, sdrx_blanker_record *out)
{
    return stage_get<BlankRecord>(c, &sdrx_ctx::bl, cfg_out, out, "sdrx_get_blanker", "blanker", false,
                                  [](const sdrx_blanker_record &r) { return r.measured != 0; });
}

int sdrx_get_blanker_input(sdrx_ctx *c, float *out, int32_t cap_complex)
{
    if (!c || !out)
        return SDRX_EINVAL;
    if (!c->bl.on)
        return fail(c, SDRX_ESTATE, "sdrx_get_blanker_input: no blanker set (sdrx_set_blanker)");
    if (!c->finalized || c->frame_no == 0)
        return fail(c, SDRX_ESTATE, "sdrx_get_blanker_input: no frame processed yet");
    if (c->in_flight > 0)
        return fail(c, SDRX_ESTATE, "sdrx_get_blanker_input: %d submitted frame(s) not yet delivered -- call sdrx_wait first", c->in_flight);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    const int n = std::min((int)cap_complex, c->in_frame);
    const size_t total = align_up((size_t)c->in_frame, kChunk);
    std::vector<float2> t(total);
    HIPCHK(c, hipMemcpy(t.data(), c->bl.d_stage, total * sizeof(float2), hipMemcpyDeviceToHost));
    untile(t.data(), out, std::max(n, 0));
    return SDRX_OK;
}

// ---- IQ balance correction (include/sdrx.h; sdrx_iqbal.h has the rules) ---------------------------------------------------------
int sdrx_set_iq_balance(sdrx_ctx *c, const sdrx_iq_cfg *cfg)
{
    if (int rc = stage_set_entry(c, &sdrx_ctx::iq, cfg, "sdrx_set_iq_balance", "IQ balance correction"))
        return rc == kStageOff ? SDRX_OK : rc;
    if (const char *why = iq_args(cfg->mu, cfg->min_power, cfg->c0, cfg->d0, cfg->flags, cfg->reserved))
        return fail(c, SDRX_EINVAL, "sdrx_set_iq_balance: %s", why);
    if (c->finalized) {
        if (int rc = stage_set_between_frames(c, "sdrx_set_iq_balance"))
            return rc;
        if (cfg->flags & SDRX_IQ_LOAD) // the pair of the next frame, in stream order
            hipLaunchKernelGGL(k_iqbal_load, dim3(1), dim3(64), 0, c->st.stream, c->iq.d_state.get(), cfg->c0, cfg->d0);
    }
    const bool keep = c->finalized && !(cfg->flags & SDRX_IQ_LOAD); // (c0, d0 stay what was last written into the state)
    c->iq.cfg = IqCfg{cfg->mu, cfg->min_power, keep ? c->iq.cfg.c0 : cfg->c0, keep ? c->iq.cfg.d0 : cfg->d0, cfg->flags, {0, 0, 0}};
    c->iq.on = true;
    return SDRX_OK;
}

int sdrx_get_iq_balance(sdrx_ctx *c, sdrx_iq_cfg *cfg_out, sdrx_iq_record *out)
{
    return stage_get<IqRecord>(c, &sdrx_ctx::iq, cfg_out, out, "sdrx_get_iq_balance", "IQ balance correction", false,
                               [](const sdrx_iq_record &r) { return r.n_complex != 0; });
}

// ---- Frequency shift (include/sdrx.h; sdrx_shift.h has the rules) ------------------------------------------------------------------
int sdrx_set_shift(sdrx_ctx *c, const sdrx_shift_cfg *cfg)
{
    if (int rc = stage_set_entry(c, &sdrx_ctx::sh, cfg, "sdrx_set_shift", "frequency shift"))
        return rc == kStageOff ? SDRX_OK : rc;
    if (const char *why = shift_args(cfg->flags, cfg->reserved))
        return fail(c, SDRX_EINVAL, "sdrx_set_shift: %s", why);
    const bool load = (cfg->flags & SDRX_SHIFT_LOAD_PHASE) != 0;
    if (c->finalized) {
        if (int rc = stage_set_between_frames(c, "sdrx_set_shift"))
            return rc;
        // the increment of the next frame, in stream order; the phase carries on unless the caller loads one
        hipLaunchKernelGGL(k_shift_load, dim3(1), dim3(64), 0, c->st.stream, c->sh.d_state.get(), cfg->inc, cfg->phase0, load ? 1 : 0);
    }
    const bool keep = c->finalized && !load; // (phase0 stays what was last written into the state)
    c->sh.cfg = ShiftCfg{cfg->inc, keep ? c->sh.cfg.phase0 : cfg->phase0, cfg->flags, {0, 0, 0, 0, 0}};
    c->sh.on = true;
    return SDRX_OK;
}

int sdrx_get_shift(sdrx_ctx *c, sdrx_shift_cfg *cfg_out, sdrx_shift_record *out)
{
    return stage_get<ShiftRecord>(c, &sdrx_ctx::sh, cfg_out, out, "sdrx_get_shift", "frequency shift", false,
                                  [](const sdrx_shift_record &r) { return r.n_complex != 0; });
}

void sdrx_shift_tables(float *out)
{
    if (out)
        shift_tables(out);
}

int sdrx_shift_inc(double fs_tree, double hz, uint32_t *inc)
{
    uint32_t v = 0;
    if (!inc || !shift_inc(fs_tree, hz, &v))
        return SDRX_EINVAL;
    *inc = v;
    return SDRX_OK;
}

double sdrx_shift_hz(double fs_tree, uint32_t inc) { return shift_hz(fs_tree, inc); }

// ---- Detector leaves (include/sdrx.h; sdrx_detect.h has the rules) -----------------------------------------------------------------
int sdrx_set_detector(sdrx_ctx *c, int id, const sdrx_detect_cfg *cfg)
{
    if (!c)
        return SDRX_EINVAL;
    if (c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_set_detector after sdrx_finalize");
    if (!cfg || id < 0 || id >= (int)c->nodes.size())
        return fail(c, SDRX_EINVAL, "sdrx_set_detector: bad vfo id %d or null settings", id);
    DetectCfg d;
    memcpy(&d, cfg, sizeof d);
    if (const char *why = detect_args(d))
        return fail(c, SDRX_EINVAL, "sdrx_set_detector: vfo %d: %s", id, why);
    Node &n = c->nodes[(size_t)id];
    if (n.d.demod_usb)
        return fail(c, SDRX_EINVAL, "sdrx_set_detector: vfo %d has demod_usb set: a USB leaf has its detector", id);
    n.detector = d.kind;
    return SDRX_OK;
}

int sdrx_get_detector(sdrx_ctx *c, int id, sdrx_detect_cfg *cfg_out)
{
    if (!c)
        return SDRX_EINVAL;
    if (!cfg_out || id < 0 || id >= (int)c->nodes.size())
        return fail(c, SDRX_EINVAL, "sdrx_get_detector: bad vfo id %d or null output", id);
    memset(cfg_out, 0, sizeof *cfg_out);
    cfg_out->kind = c->nodes[(size_t)id].detector;
    return SDRX_OK;
}

// ---- Post-detection filter (include/sdrx.h; sdrx_postdet.h has the rules and the design) -------------------------------------------
int sdrx_set_postfilter(sdrx_ctx *c, int id, const sdrx_postfilter_cfg *cfg, const float *taps)
{
    if (!c)
        return SDRX_EINVAL;
    if (c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_set_postfilter after sdrx_finalize");
    if (!cfg || id < 0 || id >= (int)c->nodes.size())
        return fail(c, SDRX_EINVAL, "sdrx_set_postfilter: bad vfo id %d or null settings", id);
    PostCfg p;
    memcpy(&p, cfg, sizeof p);
    if (const char *why = postdet_args(p))
        return fail(c, SDRX_EINVAL, "sdrx_set_postfilter: vfo %d: %s", id, why);
    if (p.ntaps > 0 && !taps)
        return fail(c, SDRX_EINVAL, "sdrx_set_postfilter: vfo %d: null taps", id);
    Node &n = c->nodes[(size_t)id];
    if (p.ntaps == 0) {
        n.post_taps.clear();
        n.post_decim = 1;
    } else {
        n.post_taps.assign(taps, taps + p.ntaps);
        n.post_decim = p.decim;
    }
    return SDRX_OK;
}

int sdrx_get_postfilter(sdrx_ctx *c, int id, sdrx_postfilter_info *info, float *taps, int32_t cap)
{
    if (!c)
        return SDRX_EINVAL;
    if (!info || id < 0 || id >= (int)c->nodes.size())
        return fail(c, SDRX_EINVAL, "sdrx_get_postfilter: bad vfo id %d or null output", id);
    const Node &n = c->nodes[(size_t)id];
    if (n.post_taps.empty())
        return fail(c, SDRX_ESTATE, "sdrx_get_postfilter: vfo %d has no post-detection filter", id);
    memset(info, 0, sizeof *info);
    info->decim = n.post_decim;
    info->ntaps = (int32_t)n.post_taps.size();
    info->out_len = c->finalized ? detect_out(n) : 0;
    info->delay_samples = ((double)n.post_taps.size() - 1) / 2.0;
    if (taps && cap > 0)
        memcpy(taps, n.post_taps.data(), sizeof(float) * std::min((size_t)cap, n.post_taps.size()));
    return SDRX_OK;
}

int sdrx_postfilter_design(double fs, double cutoff_hz, int32_t ntaps, double atten_db, float *taps, int32_t cap, sdrx_postfilter_info *info)
{
    if (taps && cap < ntaps)
        return fail(nullptr, SDRX_EINVAL, "sdrx_postfilter_design: room for %d taps, %d asked for", cap, ntaps);
    double pass = 0, stop = 0;
    const int rc = postdet_design(fs, cutoff_hz, ntaps, atten_db, taps, &pass, &stop);
    if (rc == 1)
        return fail(nullptr, SDRX_EINVAL, "sdrx_postfilter_design: atten_db must be above 50 and at most 120, ntaps in 1 .. 256, fs and cutoff_hz positive");
    if (rc == 2)
        return fail(nullptr, SDRX_EFILTER, "sdrx_postfilter_design: %d taps at %g dB: the transition around %g Hz does not fit into 0 .. %g Hz", ntaps, atten_db,
                    cutoff_hz, fs / 2);
    if (info) {
        memset(info, 0, sizeof *info);
        info->ntaps = ntaps;
        info->delay_samples = ((double)ntaps - 1) / 2.0;
        info->pass_hz = pass, info->stop_hz = stop;
    }
    return SDRX_OK;
}

// ---- Spur canceller (include/sdrx.h; sdrx_notch.h has the rules) -------------------------------------------------------------------
int sdrx_set_notch(sdrx_ctx *c, const sdrx_notch_cfg *cfg)
{
    if (int rc = stage_set_entry(c, &sdrx_ctx::nt, cfg, "sdrx_set_notch", "spur canceller"))
        return rc == kStageOff ? SDRX_OK : rc;
    NotchCfg N;
    memcpy(&N, cfg, sizeof N);
    if (const char *why = notch_args(N))
        return fail(c, SDRX_EINVAL, "sdrx_set_notch: %s", why);
    if (c->finalized) {
        if (int rc = stage_set_between_frames(c, "sdrx_set_notch"))
            return rc;
        // the tone list of the next frame, in stream order: a slot whose inc0 stays keeps phase, increment and amplitude
        NotchLoad a;
        memcpy(a.inc0, N.inc0, sizeof a.inc0);
        a.restart = notch_restart_mask(c->nt.cfg, N);
        if (a.restart)
            hipLaunchKernelGGL(k_notch_load, dim3(1), dim3(64), 0, c->st.stream, c->nt.d_state.get(), a);
    } else if (N.n_tones == 0) { // no tones before sdrx_finalize: off
        c->nt.on = false;
        return SDRX_OK;
    }
    c->nt.cfg = N;
    c->nt.on = true;
    return SDRX_OK;
}

int sdrx_get_notch(sdrx_ctx *c, sdrx_notch_cfg *cfg_out, sdrx_notch_record *out)
{
    return stage_get<NotchRecord>(c, &sdrx_ctx::nt, cfg_out, out, "sdrx_get_notch", "spur canceller", true, // (the settings as last written)
                                  [](const sdrx_notch_record &r) { return r.n_complex != 0; });
}

int sdrx_get_stream(sdrx_ctx *c, int id, float *out, int max_complex, int *n_ret)
{
    if (!c || id < 0 || id >= (int)c->nodes.size())
        return fail(c, SDRX_EINVAL, "bad vfo id %d", id);
    if (!c->finalized || c->frame_no == 0)
        return fail(c, SDRX_ESTATE, "sdrx_get_stream: no frame processed yet");
    if (c->in_flight > 0) // the stream buffers already belong to the newest submitted frame, not to the last delivered one
        return fail(c, SDRX_ESTATE, "sdrx_get_stream: %d submitted frame(s) not yet delivered -- call sdrx_wait first", c->in_flight);
    const Node &n = c->nodes[(size_t)id];
    const int par = (int)((c->frame_no - 1) & 1ull);
    const int cnt = std::min(max_complex, n.n_f);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    if (leaf_parked_at(c, id, c->frame_no - 1))
        return fail(c, SDRX_ENOSTREAM, "sdrx_get_stream: vfo %d was parked in frame %llu (sdrx_set_active)", id, c->frame_no - 1);
    const auto tap = c->taps.find(id);
    if (!n.has_stream && !(tap != c->taps.end() && c->frame_no > tap->second.since))
        return fail(c, SDRX_ENOSTREAM,
                    "sdrx_get_stream: vfo %d %s inside the mix wave and keeps no decimate[%d] -- select it with sdrx_set_tap / "
                    "sdrx_add_tap before the frame (the reference's fftVFOSlot), or set option keep_streams=1 / %s=0",
                    id, n.fused_late ? "decimates by 5 / 6" : "demodulates", n.d.decimate_count, n.fused_late ? "fuse_late" : "fuse_demod");
    if (out && cnt > 0) {
        if (!n.has_stream) {
            HIPCHK(c, hipMemcpy(out, tap->second.buf[par], sizeof(float2) * (size_t)cnt, hipMemcpyDeviceToHost));
        } else if (n.leaf) {
            HIPCHK(c, hipMemcpy(out, c->arena + n.off_stream[par] + sizeof(float2) * (size_t)n.Hx, sizeof(float2) * (size_t)cnt,
                                hipMemcpyDeviceToHost));
        } else {
            // tile layout on the device: undo it for the caller (fftData carries natural order)
            const size_t total = align_up((size_t)n.n_f, kChunk);
            std::vector<float2> tmp(total);
            HIPCHK(c, hipMemcpy(tmp.data(), c->arena + n.off_stream[par], sizeof(float2) * total, hipMemcpyDeviceToHost));
            untile(tmp.data(), out, cnt);
        }
    }
    if (n_ret)
        *n_ret = n.n_f;
    return SDRX_OK;
}

// the first spectrum: tables (the reference's own double expressions) and per-slot records
static int spectrum_first_use(sdrx_ctx *c)
{
    const size_t slots = c->nodes.size() + 1;
    const std::vector<float2> tab = spectrum_tables();
    HIPCHK(c, c->spec.d_tw.alloc(tab.size()));
    HIPCHK(c, hipMemcpy(c->spec.d_tw, tab.data(), sizeof(float2) * tab.size(), hipMemcpyHostToDevice));
    HIPCHK(c, c->spec.d_rec.alloc(slots));
    HIPCHK(c, hipMemsetAsync(c->spec.d_rec, 0, sizeof(SpecRecord) * slots, c->st.stream));
    HIPCHK(c, c->spec.d_desc.alloc(slots));
    c->spec.slots.resize(slots);
    return SDRX_OK;
}

int sdrx_set_spectrum(sdrx_ctx *c, int id, int enable)
{
    if (!c)
        return SDRX_EINVAL;
    if (!c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_set_spectrum before sdrx_finalize");
    const int N = (int)c->nodes.size();
    if (id != SDRX_SPECTRUM_RAW && (id < 0 || id >= N))
        return fail(c, SDRX_EINVAL, "sdrx_set_spectrum: bad vfo id %d", id);
    if (c->in_flight > 0)
        return fail(c, SDRX_ESTATE, "sdrx_set_spectrum: %d submitted frame(s) not yet delivered -- call sdrx_wait first", c->in_flight);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c)) // frames inside the software pipeline finish under the spectra they were queued with
        return rc;
    if (enable && id >= 0 && c->wake.controlled(id))
        return fail(c, SDRX_EINVAL, "sdrx_set_spectrum: vfo %d is under the device's wake control (sdrx_set_wake)", id);
    const int slot = id < 0 ? N : id;
    if (c->spec.slots.empty()) {
        if (int rc = spectrum_first_use(c)) {
            c->spec = sdrx_ctx::Spectrum();
            return rc;
        }
    }
    sdrx_ctx::SpecState &S = c->spec.slots[(size_t)slot];
    if (enable) {
        if (!S.pwr && S.pwr.alloc(2 * (size_t)kSpecN) != hipSuccess)
            return fail(c, SDRX_ENOMEM, "sdrx_set_spectrum: no device memory for the spectrum of vfo %d", id);
        // the combo-box reset (mainwindow.cpp:539-549): pwr and the window input zeroed, sdrj's count = 0
        HIPCHK(c, hipMemsetAsync(S.pwr, 0, S.pwr.bytes(), c->st.stream));
        HIPCHK(c, hipStreamSynchronize(c->st.stream)); // (the context's streams do not synchronise with the null stream)
        SpecRecord r;
        memset(&r, 0, sizeof r);
        r.n_in = std::min(id < 0 ? c->root_frame : c->nodes[(size_t)id].n_f, kSpecN);
        HIPCHK(c, hipMemcpy(c->spec.d_rec + slot, &r, sizeof r, hipMemcpyHostToDevice));
        S.on = true;
        if (id < 0)
            c->spec.raw_count = 0;
    } else {
        S.pwr.reset();
        S.on = false;
    }
    return spectrum_rebuild(c);
}

static int spectrum_call(sdrx_ctx *c, const char *what, const int *ids, int n)
{
    if (!c->finalized)
        return fail(c, SDRX_ESTATE, "%s before sdrx_finalize", what);
    const int N = (int)c->nodes.size();
    for (int k = 0; k < n; ++k) {
        const int id = ids[k];
        if (id != SDRX_SPECTRUM_RAW && (id < 0 || id >= N))
            return fail(c, SDRX_EINVAL, "%s: bad vfo id %d", what, id);
        if (c->spec.slots.empty() || !c->spec.slots[(size_t)(id < 0 ? N : id)].on)
            return fail(c, SDRX_ESTATE, "%s: the spectrum of vfo %d is not enabled (sdrx_set_spectrum)", what, id);
    }
    if (c->in_flight > 0)
        return fail(c, SDRX_ESTATE, "%s: %d submitted frame(s) not yet delivered -- call sdrx_wait first", what, c->in_flight);
    HIPCHK(c, hipSetDevice(c->device));
    return drain(c);
}

int sdrx_get_spectrum(sdrx_ctx *c, int id, sdrx_spectrum_info *info, double *pwr, double *smooth, float *bins_iq)
{
    if (!c)
        return SDRX_EINVAL;
    if (int rc = spectrum_call(c, "sdrx_get_spectrum", &id, 1))
        return rc;
    const int slot = id < 0 ? (int)c->nodes.size() : id;
    const double *d_pwr = c->spec.slots[(size_t)slot].pwr;
    if (info)
        HIPCHK(c, hipMemcpy(info, c->spec.d_rec + slot, sizeof *info, hipMemcpyDeviceToHost));
    if (bins_iq)
        HIPCHK(c, hipMemcpy(bins_iq, d_pwr + kSpecN, sizeof(float2) * kSpecN, hipMemcpyDeviceToHost));
    if (pwr || smooth) {
        std::vector<double> tmp;
        double *p = pwr;
        if (!p) {
            tmp.resize(kSpecN);
            p = tmp.data();
        }
        HIPCHK(c, hipMemcpy(p, d_pwr, sizeof(double) * kSpecN, hipMemcpyDeviceToHost));
        if (smooth) // mainwindow.cpp:454-458
            for (int i = 0; i < kSpecN - 10; ++i)
                smooth[i] = (p[i + 4] + p[i + 3] + p[i + 2] + p[i + 1] + p[i]) / 5;
    }
    return SDRX_OK;
}

int sdrx_get_spectrum_levels(sdrx_ctx *c, const int *ids, int n, double *maxval, double *aveval, int64_t *updates)
{
    if (!c)
        return SDRX_EINVAL;
    if (n < 0 || (n > 0 && !ids))
        return fail(c, SDRX_EINVAL, "sdrx_get_spectrum_levels: bad id list");
    if (int rc = spectrum_call(c, "sdrx_get_spectrum_levels", ids, n))
        return rc;
    if (n == 0)
        return SDRX_OK;
    const int N = (int)c->nodes.size();
    std::vector<SpecRecord> r((size_t)N + 1);
    HIPCHK(c, hipMemcpy(r.data(), c->spec.d_rec, sizeof(SpecRecord) * r.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < n; ++k) {
        const SpecRecord &e = r[(size_t)(ids[k] < 0 ? N : ids[k])];
        if (maxval)
            maxval[k] = e.maxval;
        if (aveval)
            aveval[k] = e.aveval;
        if (updates)
            updates[k] = e.updates;
    }
    return SDRX_OK;
}

int sdrx_get_prequant(sdrx_ctx *c, int id, float *out, int max, int *n_ret)
{
    if (!c || id < 0 || id >= (int)c->nodes.size())
        return fail(c, SDRX_EINVAL, "bad vfo id %d", id);
    const Node &n = c->nodes[(size_t)id];
    if (!c->finalized || !c->opt_prequant || !n.leaf || !n.d.demod_usb)
        return fail(c, SDRX_ESTATE, "sdrx_get_prequant: set option keep_prequant=1 before finalize; USB leaves only");
    if (c->in_flight > 0)
        return fail(c, SDRX_ESTATE, "sdrx_get_prequant: %d submitted frame(s) not yet delivered -- call sdrx_wait first", c->in_flight);
    const int cnt = std::min(max, n.n_out);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    if (c->frame_no > 0 && leaf_parked_at(c, id, c->frame_no - 1))
        return fail(c, SDRX_ENOSTREAM, "sdrx_get_prequant: vfo %d was parked in frame %llu (sdrx_set_active)", id, c->frame_no - 1);
    if (out && cnt > 0)
        HIPCHK(c, hipMemcpy(out, c->arena + n.off_preq, sizeof(float) * (size_t)cnt, hipMemcpyDeviceToHost));
    if (n_ret)
        *n_ret = n.n_out;
    return SDRX_OK;
}

int sdrx_get_taps(sdrx_ctx *c, int id, int which, float *out, int max, int *n_ret)
{
    if (!c || id < 0 || id >= (int)c->nodes.size())
        return fail(c, SDRX_EINVAL, "bad vfo id %d", id);
    if (!c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_get_taps before sdrx_finalize");
    const Node &n = c->nodes[(size_t)id];
    const std::vector<float> *t = which == 0 ? &n.lpf : which == 1 ? &n.dec : which == 2 ? &n.hilbert : nullptr;
    if (!t)
        return fail(c, SDRX_EINVAL, "which must be 0, 1 or 2");
    // read back what the kernels actually use (device copy), not the host vector
    const size_t off = which == 0 ? n.off_lpf + (n.long_lpf ? 0 : 3 * sizeof(float)) : which == 1 ? n.off_dec : n.off_hilbert;
    const int cnt = std::min(max, (int)t->size());
    HIPCHK(c, hipSetDevice(c->device));
    if (out && cnt > 0)
        HIPCHK(c, hipMemcpy(out, c->arena + off, sizeof(float) * (size_t)cnt, hipMemcpyDeviceToHost));
    if (n_ret)
        *n_ret = (int)t->size();
    return SDRX_OK;
}

int sdrx_get_nco(sdrx_ctx *c, int id, long first, long count, float *out)
{
    if (!c || id < 0 || id >= (int)c->nodes.size())
        return fail(c, SDRX_EINVAL, "bad vfo id %d", id);
    if (!c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_get_nco before sdrx_finalize");
    const Node &n = c->nodes[(size_t)id];
    if (first < 0 || count < 0 || first + count > n.d.fs)
        return fail(c, SDRX_EINVAL, "table range [%ld,%ld) outside 0..%d", first, first + count, n.d.fs);
    if (count == 0)
        return SDRX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<float2> tmp;
    HIPCHK(c, tmp.alloc((size_t)count));
    hipLaunchKernelGGL(k_nco_dump, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->st.stream,
                       reinterpret_cast<const float2 *>(c->arena + n.off_cp), n.rot_re, n.rot_im, first, count, tmp);
    hipError_t e = hipStreamSynchronize(c->st.stream);
    if (e == hipSuccess)
        e = hipMemcpy(out, tmp, sizeof(float2) * (size_t)count, hipMemcpyDeviceToHost);
    tmp.reset();
    if (e != hipSuccess)
        return fail(c, SDRX_EHIP, "sdrx_get_nco: %s", hipGetErrorString(e));
    return SDRX_OK;
}

int sdrx_get_stats(sdrx_ctx *c, sdrx_stats *s)
{
    if (!c || !s)
        return SDRX_EINVAL;
    memset(s, 0, sizeof *s);
    s->n_vfos = (int)c->nodes.size();
    for (const Node &n : c->nodes)
        s->n_leaves += n.children.empty();
    s->n_levels = c->n_levels;
    s->exact = c->opt_exact;
    s->algorithmic_bytes_per_frame = c->alg_bytes;
    s->vfo_samples_per_frame = c->vfo_samples;
    const size_t raw_bytes = c->d_raw[0].bytes() + c->d_raw_u8[0].bytes(); // (ONE parity of the host-fed frames' buffers: kept for compatibility)
    s->device_bytes = (int64_t)(c->arena_bytes + 2 * c->pay_bytes + raw_bytes + c->sq.bytes() + c->park.d_act.bytes() + c->watch.bytes() + c->drift.bytes() + c->scan.bytes() + c->agc.bytes() + c->wake.bytes() + c->adc.bytes() + c->rs.bytes() + c->fr.bytes() + c->bl.bytes() + c->iq.bytes() + c->sh.bytes() + c->nt.bytes());
    s->frames = (int64_t)c->frame_no;
    s->mix_chunks_per_frame = c->mix_chunks;
    if (c->dc.d_counters) { // (waits for what is queued: a measurement call)
        unsigned long long h[3] = {0, 0, 0};
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->st.stream));
        HIPCHK(c, hipMemcpy(h, c->dc.d_counters, sizeof h, hipMemcpyDeviceToHost));
        s->dc_blocks = (int64_t)h[0];
        s->dc_fallback_blocks = (int64_t)h[1];
        s->dc_retried_blocks = (int64_t)h[2];
    }
    return SDRX_OK;
}

int sdrx_enable_kernel_timing(sdrx_ctx *c, int enable)
{
    if (!c)
        return SDRX_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    c->tm.on = enable != 0;
    for (int k = 0; k < SDRX_NKERNELS; ++k) {
        c->tm.ms[k] = 0;
        c->tm.n[k] = 0;
        c->tm.bytes[k] = 0;
    }
    return SDRX_OK;
}

int sdrx_get_kernel_times(sdrx_ctx *c, double ms[SDRX_NKERNELS], int64_t launches[SDRX_NKERNELS],
                          int64_t alg_bytes[SDRX_NKERNELS])
{
    if (!c)
        return SDRX_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    for (int k = 0; k < SDRX_NKERNELS; ++k) {
        if (ms)
            ms[k] = c->tm.ms[k];
        if (launches)
            launches[k] = c->tm.n[k];
        if (alg_bytes)
            alg_bytes[k] = c->tm.bytes[k];
    }
    return SDRX_OK;
}

} // extern "C"

#include "sdrx_group.hip"
