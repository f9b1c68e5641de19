// host/sdrx_host.hpp -- C++ host layer over the C ABI (include/sdrx.h), Qt-free, header-only.
//
// The reference's host is Qt/C++.  This header gives a C++ host the reference's own interface for
// the path, minus Qt:
//   sdrx_host::vfo   -- setters / init / setVFOs of `class vfo`           (vfo.h:16-49)
//   sdrx_host::sdrj  -- setVFOs / setDCCorrection / demodData of `sdrj`   (sdrj.h, sdrj.cpp:266-305)
//   sdrx_host::load_profile -- the INI -> VFO tree rules of MainWindow    (mainwindow.cpp:27-233)
// A Qt front-end wraps these; tests drive them through host/demo.cpp.
#pragma once
#include <algorithm>
#include <cctype>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../include/sdrx.h"

namespace sdrx_host {

// ------------------------------------------------------------------------------------------ vfo
class vfo {
public:
    vfo()
    {
        std::memset(&d, 0, sizeof d);
        d.gain = 0.01f;   // vfo.cpp:9
        d.demod_usb = 1;  // vfo.cpp:15
        d.scalecomp = 1;  // vfo.cpp:24
        d.parent_id = -1;
    }
    void setFs(int samplerate) { d.fs = samplerate; }
    void setDecimationCount(int count) { d.decimate_count = count; }
    void setMixerFreq(double freq) { d.mixer_freq_hz = freq; }
    double getMixerFreq() const { return d.mixer_freq_hz; }
    int getOutRate() const { return (int)(d.fs / std::pow(2, d.decimate_count)); } // vfo.cpp:212-217
    void setFilterBandwidth(double bw) { d.filter_bw_hz = (int)bw; }
    void setGain(float g) { d.gain = g; }
    void setDemodUSB(bool usb) { d.demod_usb = usb ? 1 : 0; }
    bool getDemodUSB() const { return d.demod_usb != 0; }
    void setCompressonStyle(int st) { d.cstyle = st; } // sic, vfo.h:36
    // no counterpart in vfo.h: a leaf with setDemodUSB(false) leaves as an AM envelope (SDRX_DETECT_AM) or an FM discriminator
    // (SDRX_DETECT_FM) in int16 instead of compress()'s bytes (include/sdrx.h "Detector leaves"); a single context only
    void setDetector(int kind) { detector = kind; }
    int getDetector() const { return detector; }
    // no counterpart in vfo.h either: a detector leaf leaves through a FIR of `taps` over the detector's floats, decimated by
    // `decim` (include/sdrx.h "Post-detection filter"); no taps take it away; a single context only
    void setPostFilter(const std::vector<float> &taps, int decim)
    {
        postTaps = taps;
        postDecim = taps.empty() ? 1 : decim;
    }
    const std::vector<float> &getPostTaps() const { return postTaps; }
    int getPostDecim() const { return postDecim; }
    void setScaleComp(int scale) { d.scalecomp = scale; }
    void setZmqTopic(const std::string &t)
    {
        topic = t;
        std::memset(d.topic, 0, sizeof d.topic);
        std::memcpy(d.topic, t.data(), std::min<size_t>(t.size(), sizeof(d.topic) - 1));
    }
    void setZmqAddress(const std::string &a) { zmqAddress = a; } // the socket stays on the host side
    void init(int samplesPerBuffer, bool /*bind*/, int lateDecimate = 0)
    {
        d.samples_per_buffer = samplesPerBuffer;
        d.late_decimate = lateDecimate;
        initialised = true;
    }
    void setVFOs(std::vector<vfo *> *pVFOs) { mpVFOs = pVFOs; }
    // vfo.cpp:492-509: decimate[decimateCount] goes to fftData after every frame while the selected
    // topic is this VFO's own (the Qt signal of vfo.h:46 is a plain callback here)
    void fftVFOSlot(const std::string &t) { emitFFT = t == topic; }
    std::function<void(const std::vector<std::complex<float>> &)> fftData;
    bool emitFFT = false;

    sdrx_vfo_desc d;
    std::string topic, zmqAddress;
    std::vector<vfo *> *mpVFOs = nullptr;
    int id = -1;
    int detector = SDRX_DETECT_NONE;
    std::vector<float> postTaps;
    int postDecim = 1;
    bool initialised = false;
};

// ------------------------------------------------------------------------------------------ sdrj
// publish(topic5, rate, payload, len): what vfo::transmitData hands to ZmqPublisher::publish.
using publish_fn = std::function<void(const char topic[5], uint32_t rate, const void *buf, uint32_t len)>;

// ------------------------------------------------------------------------------------------ ADC meter
// What an sdrx_adc_meter record (library option "adc_meter" = 1, sdrj::adcMeter below) says about the front end, in the chain's
// units -- CS16 codes times 2^-8, the 8-bit codes as they are; full scale is 128 for every format.  The arithmetic of
// sdrreceiver_amd.ingest.adc_levels, operation for operation: the variances and the covariance from exact integers,
// var_i = (n sum_sq_i - sum_i^2) / n^2, cov = (n sum_iq - sum_i sum_q) / n^2, each numerator converted to double once.
struct adc_levels_t {
    double dc_i = 0, dc_q = 0;  // means
    double rms = 0;             // of the components, I and Q together, DC included
    double peak = 0;            // largest |code|
    double headroom_db = 0;     // 20 log10(128 / peak); +inf for an all-zero frame
    double clip_share = 0;      // components at a rail / 2 n
    uint32_t longest_rail_run = 0;
    int bits_used = 0;          // the highest non-empty bin of bits[]
    double gain_imbalance = 0;  // sqrt(var_i / var_q); NaN when an arm is constant
    double phase_error = 0;     // asin(cov / sqrt(var_i var_q)), radians; NaN likewise
};
inline adc_levels_t adc_levels(const sdrx_adc_meter &r)
{
    if (!r.measured)
        throw std::invalid_argument("adc_levels: the frame was not measured (it did not arrive as integer samples)");
    typedef __int128 wide;
    // (a record of real samples, SDRX_FMT_RS16 / RU12, holds the even samples in arm i and the odd ones in arm q: the levels are per
    // arm as for I/Q; sdrreceiver_amd.ingest.adc_levels merges them)
    const double s = r.fmt == SDRX_FMT_CS16 || r.fmt == SDRX_FMT_RS16 ? 0.00390625 : r.fmt == SDRX_FMT_RU12 ? 0.0625 : 1.0, n = (double)r.n_complex, nn = n * n;
    const wide N = (wide)r.n_complex;
    const double var_i = (double)(N * (wide)r.i.sum_sq - (wide)r.i.sum * (wide)r.i.sum) / nn * s * s;
    const double var_q = (double)(N * (wide)r.q.sum_sq - (wide)r.q.sum * (wide)r.q.sum) / nn * s * s;
    const double cov = (double)(N * (wide)r.sum_iq - (wide)r.i.sum * (wide)r.q.sum) / nn * s * s;
    auto mag = [](int32_t v) { return v < 0 ? -(int64_t)v : (int64_t)v; };
    adc_levels_t L;
    L.dc_i = (double)r.i.sum / n * s;
    L.dc_q = (double)r.q.sum / n * s;
    L.rms = std::sqrt((double)(r.i.sum_sq + r.q.sum_sq) / (2.0 * n)) * s;
    L.peak = (double)std::max(std::max(mag(r.i.min), mag(r.i.max)), std::max(mag(r.q.min), mag(r.q.max))) * s;
    L.headroom_db = L.peak > 0.0 ? 20.0 * std::log10(128.0 / L.peak) : HUGE_VAL;
    L.clip_share = (double)((uint64_t)r.i.at_lo + r.i.at_hi + r.q.at_lo + r.q.at_hi) / (2.0 * n);
    L.longest_rail_run = std::max(r.i.longest_rail_run, r.q.longest_rail_run);
    for (int k = 0; k < 17; ++k)
        if (r.bits[k])
            L.bits_used = k;
    const bool ok = var_i > 0.0 && var_q > 0.0;
    L.gain_imbalance = ok ? std::sqrt(var_i / var_q) : NAN;
    L.phase_error = ok ? std::asin(std::min(1.0, std::max(-1.0, cov / std::sqrt(var_i * var_q)))) : NAN;
    return L;
}

class sdrj {
public:
    explicit sdrj(int device = 0) : devices_(1, device) {}
    // One tree on several GPUs of the node (sdrx_group_*): sub VFOs block-partitioned per main VFO, the raw
    // frame fanned out from the first device over xGMI.  A device may be named twice (two shards on one GPU).
    explicit sdrj(std::vector<int> devices) : devices_(std::move(devices))
    {
        if (devices_.empty())
            devices_.push_back(0);
    }
    ~sdrj()
    {
        if (ctx_)
            sdrx_destroy(ctx_);
        if (grp_)
            sdrx_group_destroy(grp_);
    }
    sdrj(const sdrj &) = delete;
    sdrj &operator=(const sdrj &) = delete;

    void setVFOs(std::vector<vfo *> *vfos) { mpVFOs = vfos; }
    void setDCCorrection(bool dc) { correctDC = dc; }
    void setPublisher(publish_fn f) { publish_ = std::move(f); }
    void setOption(const std::string &name, int value) { options_[name] = value; }
    // The front end's sample rate where it is not the main VFOs' Fs (Airspy at 10, 6, 3 or 2.5 MS/s, an RTL dongle at 2.4 or
    // 2.048 MS/s; no counterpart in the reference): before the first frame.  Every frame handed to demodData / demodBytes /
    // demodSamples then has resampler().in_frame samples at that rate, and a rational resampler on the device -- the library's
    // own Kaiser design with `taps_per_phase` taps per phase and `atten_db` of stop band -- makes the tree's frame from it
    // (include/sdrx.h "Resampler").  0: off.  One device only.
    void setInputRate(int fs_in, int taps_per_phase = 32, double atten_db = 80.0)
    {
        if (started())
            throw std::runtime_error("sdrj::setInputRate after the first frame");
        input_rate_ = fs_in, rs_taps_ = taps_per_phase, rs_atten_ = atten_db;
    }
    // ... and what it is once the tree is committed (start()): ratio, frame lengths, delay and pass band
    sdrx_resampler_info resampler()
    {
        if (!ctx_ || !input_rate_)
            throw std::runtime_error("sdrj::resampler: no input rate set, or not started");
        sdrx_resampler_info info;
        check(sdrx_get_resampler(ctx_, &info, nullptr, 0), "sdrx_get_resampler");
        info.passband_hz = rs_passband_;
        return info;
    }
    // A half-band front stage on the device in front of the resampler or of the main VFOs (include/sdrx.h "Front stage"; no
    // counterpart in the reference): before the first frame.  `stages` (1 .. 3) decimations by 2 with the library's own Kaiser
    // half-band of N = 4 K + 3 taps and `atten_db` of stop band; every frame then has front().in_frame samples.  real_input: the
    // front end delivers REAL samples of an IF (Airspy R2 / Mini) -- demodSamples with SDRX_FMT_RS16 or SDRX_FMT_RU12, the count
    // in real samples -- and the first stage makes I/Q of them (tuned centre fs_r / 4).  stages = 0: off.  One device only.
    void setFront(int stages, bool real_input = false, int K = 15, double atten_db = 80.0)
    {
        if (started())
            throw std::runtime_error("sdrj::setFront after the first frame");
        fr_stages_ = stages, fr_real_ = real_input, fr_K_ = K, fr_atten_ = atten_db;
    }
    // ... and what it is once the tree is committed (start()): stages, taps, frame lengths, transition width
    sdrx_front_info front()
    {
        if (!ctx_ || !fr_stages_)
            throw std::runtime_error("sdrj::front: no front stage set, or not started");
        sdrx_front_info info;
        check(sdrx_get_front(ctx_, &info, nullptr, 0), "sdrx_get_front");
        return info;
    }
    // The impulse blanker on the device (include/sdrx.h "Impulse blanker"; no counterpart in the reference): samples whose power
    // exceeds `ratio` times the rank `rank_q16` (32768: the median) of the previous frame's powers, and `floor`, become zero with
    // `guard` samples on either side, behind the format conversion and the DC removal and in front of everything else.  Before
    // the first frame it switches the stage on; afterwards it changes the four settings between two frames.  One device only.
    void setBlanker(float ratio, int guard, float floor = 0.0f, int rank_q16 = 32768)
    {
        if (grp_)
            throw std::runtime_error("sdrj: the blanker (setBlanker) is not offered on several devices");
        bl_cfg_ = sdrx_blanker_cfg{ratio, floor, rank_q16, guard, {0, 0, 0, 0}};
        if (ctx_)
            check(sdrx_set_blanker(ctx_, &bl_cfg_), "sdrx_set_blanker");
        bl_on_ = true;
    }
    // ... and its record of the last delivered frame: threshold, reference bins, hits / blanked / runs / carry_in
    sdrx_blanker_record blanker()
    {
        if (!ctx_ || !bl_on_)
            throw std::runtime_error("sdrj::blanker: no blanker set, or not started");
        sdrx_blanker_record r;
        check(sdrx_get_blanker(ctx_, nullptr, &r), "sdrx_get_blanker");
        return r;
    }
    // The IQ balance correction on the device (include/sdrx.h "IQ balance"; no counterpart in the reference): Q' = c I + d Q behind
    // the format conversion and the DC removal, the pair moved by `mu` times a Newton step once per frame that holds at least
    // `min_power` (mu = 0: held).  Before the first frame it switches the stage on, starting from (c0, d0); afterwards it changes
    // mu and min_power between two frames, and with load = true writes (c0, d0) as the pair of the next frame.  One device only.
    void setIqBalance(float mu, float min_power, float c0 = 0.0f, float d0 = 1.0f, bool load = false)
    {
        if (grp_)
            throw std::runtime_error("sdrj: the IQ balance correction (setIqBalance) is not offered on several devices");
        iq_cfg_ = sdrx_iq_cfg{mu, min_power, c0, d0, load ? SDRX_IQ_LOAD : 0u, {0, 0, 0}};
        if (ctx_)
            check(sdrx_set_iq_balance(ctx_, &iq_cfg_), "sdrx_set_iq_balance");
        iq_on_ = true;
    }
    // ... and its record of the last delivered frame: measured / adapted / rejected, the pair used, the next one, the five sums
    sdrx_iq_record iqBalance()
    {
        if (!ctx_ || !iq_on_)
            throw std::runtime_error("sdrj::iqBalance: no IQ balance correction set, or not started");
        sdrx_iq_record r;
        check(sdrx_get_iq_balance(ctx_, nullptr, &r), "sdrx_get_iq_balance");
        return r;
    }
    // The frequency shift on the device (include/sdrx.h "Frequency shift"; the reference's mix_offset, README "tune ALL VFO's up or
    // down by a number of Hz", as one stage): the tree's raw frame times exp(+j 2 pi hz t), `hz` at the parent-less VFOs' rate.
    // Before the first frame it switches the stage on; afterwards it changes the shift between two frames, phase-continuous in
    // every channel.  One device only.
    void setShift(double hz)
    {
        if (grp_)
            throw std::runtime_error("sdrj: the frequency shift (setShift) is not offered on several devices");
        shift_hz_ = hz;
        if (ctx_) {
            const sdrx_shift_cfg cfg = shift_cfg();
            check(sdrx_set_shift(ctx_, &cfg), "sdrx_set_shift");
        }
        sh_on_ = true;
    }
    // ... and its record of the last delivered frame: the phase and the increment it used, and what it left behind
    sdrx_shift_record shift()
    {
        if (!ctx_ || !sh_on_)
            throw std::runtime_error("sdrj::shift: no frequency shift set, or not started");
        sdrx_shift_record r;
        check(sdrx_get_shift(ctx_, nullptr, &r), "sdrx_get_shift");
        return r;
    }
    // Closing the loop on the host: the shift that follows a drift estimate (drift_hz of the raw frame's source: a band that sits D
    // Hz high peaks at +D and is corrected by a shift of -D), clamped to +-fs_tree / 2
    static double shift_follow(double hz_now, double drift_hz, double fs_tree, double gain = 1.0)
    {
        const double hz = hz_now - gain * drift_hz;
        return hz > fs_tree / 2 ? fs_tree / 2 : hz < -fs_tree / 2 ? -fs_tree / 2 : hz;
    }
    // The spur canceller on the device (include/sdrx.h "Spur canceller"): up to SDRX_NOTCH_MAX steady carriers that are not signals,
    // given in Hz at the parent-less VFOs' rate to within tens of Hz, tracked and subtracted from the tree's raw frame in front of
    // the shift.  mu: the amplitude loop's gain; afc_gain: the frequency loop's (0 holds the frequencies); min_coherence: its gate;
    // max_pull_hz: how far a tone may move from where it was given.  Before the first frame it switches the stage on; afterwards
    // it changes the settings between two frames (a tone whose frequency is unchanged keeps its state).  One device only.
    void setNotch(const std::vector<double> &hz, float mu, float afc_gain, float min_coherence, double max_pull_hz)
    {
        if (grp_)
            throw std::runtime_error("sdrj: the spur canceller (setNotch) is not offered on several devices");
        if (hz.size() > SDRX_NOTCH_MAX)
            throw std::runtime_error("sdrj::setNotch: at most SDRX_NOTCH_MAX tones");
        nt_hz_ = hz, nt_mu_ = mu, nt_afc_ = afc_gain, nt_coh_ = min_coherence, nt_pull_hz_ = max_pull_hz;
        if (ctx_) {
            const sdrx_notch_cfg cfg = notch_cfg();
            check(sdrx_set_notch(ctx_, &cfg), "sdrx_set_notch");
        }
        nt_on_ = true;
    }
    // ... and its record of the last delivered frame: per tone the increment used and the next one, the amplitude, the flags, S, P, E
    sdrx_notch_record notch()
    {
        if (!ctx_ || !nt_on_)
            throw std::runtime_error("sdrj::notch: no spur canceller set, or not started");
        sdrx_notch_record r;
        check(sdrx_get_notch(ctx_, nullptr, &r), "sdrx_get_notch");
        return r;
    }
    // the frequency a tone of that record is tracked at, in Hz at the parent-less VFOs' rate
    double notchHz(const sdrx_notch_record &r, int k) const { return sdrx_shift_hz((double)(*mpVFOs)[0]->d.fs, r.tone[k].inc_next); }
    // sdrj.cpp:84-101: the raw spectrum is selected by the topic "Main"; any selection restarts
    // the every-4th-call counter of demodData (sdrj.cpp:296-303)
    void fftVFOSlot(const std::string &topic)
    {
        emitFFT = topic == "Main";
        count = 0;
    }
    std::function<void(const std::vector<std::complex<float>> &)> fftData; // signal of sdrj.h:40

    // Commit the tree to the GPU (== all vfo::init work).  Called by the first demodData.
    void start()
    {
        if (!mpVFOs || mpVFOs->empty())
            throw std::runtime_error("sdrj: no main VFOs");
        if (devices_.size() > 1 && input_rate_)
            throw std::runtime_error("sdrj: the resampler (setInputRate) is not offered on several devices");
        if (devices_.size() > 1 && fr_stages_)
            throw std::runtime_error("sdrj: the front stage (setFront) is not offered on several devices");
        if (devices_.size() > 1 && bl_on_)
            throw std::runtime_error("sdrj: the blanker (setBlanker) is not offered on several devices");
        if (devices_.size() > 1 && iq_on_)
            throw std::runtime_error("sdrj: the IQ balance correction (setIqBalance) is not offered on several devices");
        if (devices_.size() > 1 && sh_on_)
            throw std::runtime_error("sdrj: the frequency shift (setShift) is not offered on several devices");
        if (devices_.size() > 1 && nt_on_)
            throw std::runtime_error("sdrj: the spur canceller (setNotch) is not offered on several devices");
        if (devices_.size() > 1) {
            check(sdrx_group_create(&grp_, devices_.data(), (int)devices_.size()), "sdrx_group_create");
            for (auto &kv : options_)
                check(sdrx_group_set_option(grp_, kv.first.c_str(), kv.second), "sdrx_group_set_option");
            for (vfo *m : *mpVFOs)
                add(m, -1);
            check(sdrx_group_set_publish_callback(grp_, &sdrj::trampoline, this), "sdrx_group_set_publish_callback");
            check(sdrx_group_finalize(grp_), "sdrx_group_finalize");
            return;
        }
        check(sdrx_create(&ctx_, devices_[0]), "sdrx_create");
        for (auto &kv : options_)
            check(sdrx_set_option(ctx_, kv.first.c_str(), kv.second), "sdrx_set_option");
        for (vfo *m : *mpVFOs)
            add(m, -1); // parents first: ids are creation order = the reference's publish order
        if (input_rate_) { // (behind the VFOs: the first main's Fs is the output rate)
            std::vector<float> taps(32768);
            sdrx_resampler_info info;
            if (sdrx_resampler_design(input_rate_, (*mpVFOs)[0]->d.fs, rs_taps_, rs_atten_, taps.data(), (int)taps.size(), &info) != SDRX_OK)
                throw std::runtime_error(std::string("sdrx_resampler_design: ") + sdrx_last_error(nullptr));
            rs_passband_ = info.passband_hz;
            check(sdrx_set_resampler(ctx_, input_rate_, taps.data(), rs_taps_), "sdrx_set_resampler");
        }
        if (fr_stages_)
            check(sdrx_set_front(ctx_, fr_real_ ? 1 : 0, fr_stages_, nullptr, fr_K_, fr_atten_), "sdrx_set_front");
        if (bl_on_)
            check(sdrx_set_blanker(ctx_, &bl_cfg_), "sdrx_set_blanker");
        if (iq_on_)
            check(sdrx_set_iq_balance(ctx_, &iq_cfg_), "sdrx_set_iq_balance");
        if (sh_on_) {
            const sdrx_shift_cfg cfg = shift_cfg();
            check(sdrx_set_shift(ctx_, &cfg), "sdrx_set_shift");
        }
        if (nt_on_) {
            const sdrx_notch_cfg cfg = notch_cfg();
            check(sdrx_set_notch(ctx_, &cfg), "sdrx_set_notch");
        }
        check(sdrx_set_publish_callback(ctx_, &sdrj::trampoline, this), "sdrx_set_publish_callback");
        check(sdrx_finalize(ctx_), "sdrx_finalize");
    }

    // sdrj::demodData(const float*, int) (sdrj.cpp:266-305): `len` floats, interleaved I/Q.
    void demodData(const float *data, int len)
    {
        if (!started())
            start();
        const float *in = data;
        if (correctDC || (grp_ && emitFFT)) // (a group keeps the host's copy for the raw spectrum tap)
            samples_.assign(data, data + len);
        if (correctDC) { // sdrj.cpp:271-286, on the host exactly where the reference has it
            dc_correct(samples_);
            in = samples_.data();
        }
        select_tap();
        call("process", sdrx_group_process, sdrx_process, in, len / 2);
        after_frame(len / 2);
    }
    // rtl_tcp / dongle bytes (sdrj.cpp:149-165): LUT and DC correction on the device.  On several devices
    // the bytes themselves are fanned out (a quarter of the traffic); with the DC-bias IIR on, every device runs
    // the recurrence itself on the whole frame (same bytes, same start state: the same estimate everywhere).
    void demodBytes(const uint8_t *bytes, int n_complex)
    {
        if (!started())
            start();
        select_tap();
        if (!grp_) {
            check(sdrx_process_u8(ctx_, bytes, n_complex, correctDC ? 1 : 0), "sdrx_process_u8");
        } else {
            if (emitFFT && !correctDC) { // the raw spectrum tap of a group without DC removal: the LUT, here
                samples_.resize((size_t)2 * n_complex);
                for (size_t i = 0; i < samples_.size(); ++i)
                    samples_[i] = (float)((int)bytes[i] - 127); // jonti/sdr.cpp:43-49
            } else {
                samples_.clear();
            }
            check(sdrx_group_process_u8(grp_, bytes, n_complex, correctDC ? 1 : 0), "sdrx_group_process_u8");
        }
        after_frame(n_complex);
    }
    // Integer samples of a front end in format `fmt` (SDRX_FMT_CU8 / CS8 / CS16, include/sdrx.h; with setFront(.., true) the real
    // formats SDRX_FMT_RS16 / RU12, n_complex then counting real samples): conversion to the reference's
    // units and DC correction on the device.  SDRX_FMT_CU8 is demodBytes.  On several devices the integers themselves are
    // fanned out; the raw spectrum tap of a group is then served by the first member that holds VFOs, which keeps the
    // converted frame with or without DC removal.
    void demodSamples(const void *samples, int n_complex, int fmt)
    {
        if (fmt == SDRX_FMT_CU8)
            return demodBytes(static_cast<const uint8_t *>(samples), n_complex);
        if (!started())
            start();
        select_tap();
        samples_.clear();
        if (!grp_)
            check(sdrx_process_fmt(ctx_, samples, n_complex, fmt, correctDC ? 1 : 0), "sdrx_process_fmt");
        else
            check(sdrx_group_process_fmt(grp_, samples, n_complex, fmt, correctDC ? 1 : 0), "sdrx_group_process_fmt");
        after_frame(n_complex);
    }
    sdrx_ctx *context() { return ctx_; }
    sdrx_group *group() { return grp_; }
    // ADC meter (library option "adc_meter" = 1, setOption before the first frame; no counterpart in the reference): the exact
    // integer statistics of the last delivered frame's integer samples as they arrived -- demodBytes / demodSamples frames;
    // measured = 0 after demodData.  adc_levels() above turns the record into levels, headroom and IQ balance.
    sdrx_adc_meter adcMeter()
    {
        sdrx_adc_meter r;
        call("get_adc_meter", sdrx_group_get_adc_meter, sdrx_get_adc_meter, &r);
        return r;
    }
    // Squelch-gated egress (library option "squelch" = 1, no counterpart in the reference): leaf ids[k] -- vfo::id after
    // start() -- opens when its meter sum_sq reaches thr_sum_sq[k] and stays open hang_frames[k] frames; between two frames.
    void set_squelch(const std::vector<int> &ids, const std::vector<uint64_t> &thr_sum_sq, const std::vector<uint32_t> &hang_frames)
    {
        if (ids.size() != thr_sum_sq.size() || ids.size() != hang_frames.size())
            throw std::invalid_argument("set_squelch: lists of different length");
        call("set_squelch", sdrx_group_set_squelch, sdrx_set_squelch, ids.data(), thr_sum_sq.data(), hang_frames.data(), (int)ids.size());
    }
    // Auto-squelch (library option "squelch_auto" = 1): leaf ids[k]'s threshold becomes max(thr_sum_sq, floor * ratio_q8[k] / 256),
    // the floor being the smallest sum_sq of its last window_frames[k] .. 2 * window_frames[k] - 1 frames; ratio_q8 0 = off for
    // the leaf; between two frames.  Restarts the named leaves' floor.
    void set_squelch_auto(const std::vector<int> &ids, const std::vector<uint32_t> &ratio_q8, const std::vector<uint32_t> &window_frames)
    {
        if (ids.size() != ratio_q8.size() || ids.size() != window_frames.size())
            throw std::invalid_argument("set_squelch_auto: lists of different length");
        call("set_squelch_auto", sdrx_group_set_squelch_auto, sdrx_set_squelch_auto, ids.data(), ratio_q8.data(), window_frames.data(), (int)ids.size());
    }
    // Device-side AGC (library option "agc" = 1): USB leaf ids[k]'s gain follows its output meter between frames by the rule of
    // sdrx.h (cfgs[k].hi_ms 0 = off for the leaf); between two frames.  Restarts the named leaves' quiet_run.  agc(): what the
    // step did behind the last delivered frame -- and how a host reads a gain the device steps.
    void set_agc(const std::vector<int> &ids, const std::vector<sdrx_agc_cfg> &cfgs)
    {
        if (ids.size() != cfgs.size())
            throw std::invalid_argument("set_agc: lists of different length");
        call("set_agc", sdrx_group_set_agc, sdrx_set_agc, ids.data(), cfgs.data(), (int)ids.size());
    }
    std::vector<sdrx_agc_state> agc(const std::vector<int> &ids)
    {
        std::vector<sdrx_agc_state> out(ids.size());
        call("get_agc", sdrx_group_get_agc, sdrx_get_agc, ids.data(), (int)ids.size(), out.data());
        return out;
    }
    // Parking (library option "park" = 1): leaf ids[k] is parked (active[k] 0: no arithmetic, delivered like a closed leaf) or
    // unparked (1: a new vfo from the next frame on -- fresh oscillator, zero filter state); between two frames.
    void set_active(const std::vector<int> &ids, const std::vector<int32_t> &active)
    {
        if (ids.size() != active.size())
            throw std::invalid_argument("set_active: lists of different length");
        call("set_active", sdrx_group_set_active, sdrx_set_active, ids.data(), active.data(), (int)ids.size());
    }
    std::vector<sdrx_active_state> active(const std::vector<int> &ids)
    {
        std::vector<sdrx_active_state> out(ids.size());
        call("get_active", sdrx_group_get_active, sdrx_get_active, ids.data(), (int)ids.size(), out.data());
        return out;
    }
    // channel watch (option "watch"): band power of a leaf from its source's spectrum, active or parked
    void set_watch(const std::vector<int> &ids, const std::vector<int32_t> &on)
    {
        if (ids.size() != on.size())
            throw std::invalid_argument("set_watch: lists of different length");
        call("set_watch", sdrx_group_set_watch, sdrx_set_watch, ids.data(), on.data(), (int)ids.size());
    }
    std::vector<sdrx_watch_level> watch(const std::vector<int> &ids)
    {
        std::vector<sdrx_watch_level> out(ids.size());
        call("get_watch", sdrx_group_get_watch, sdrx_get_watch, ids.data(), (int)ids.size(), out.data());
        return out;
    }
    std::vector<double> watch_psd(int leaf_id, int64_t *frame = nullptr)
    {
        std::vector<double> psd(SDRX_SPECTRUM_BINS);
        call("get_watch_psd", sdrx_group_get_watch_psd, sdrx_get_watch_psd, leaf_id, psd.data(), frame);
        return psd;
    }
    // device-side wake (library option "wake" = 1): watched leaf ids[k] is parked and unparked by the device itself, inside the
    // frame, by the rule of sdrx.h on its watch figures (cfgs[k].on 0 releases it); between two frames.  Resets the named
    // leaves' hold_left.  wake(): the decision of the last delivered frame.
    void set_wake(const std::vector<int> &ids, const std::vector<sdrx_wake_cfg> &cfgs)
    {
        if (ids.size() != cfgs.size())
            throw std::invalid_argument("set_wake: lists of different length");
        call("set_wake", sdrx_group_set_wake, sdrx_set_wake, ids.data(), cfgs.data(), (int)ids.size());
    }
    std::vector<sdrx_wake_state> wake(const std::vector<int> &ids)
    {
        std::vector<sdrx_wake_state> out(ids.size());
        call("get_wake", sdrx_group_get_wake, sdrx_get_wake, ids.data(), (int)ids.size(), out.data());
        return out;
    }
    // drift estimate (part of option "watch"): the spectrum of the source of watched leaf `leaf_id` registered against a
    // template over the shifts -max_shift .. max_shift (0: off); templ == nullptr: the next measured frame's spectrum is
    // captured on the device.  drift(): the record of the last delivered frame; drift_hz() turns it into Hz.
    void set_drift(int leaf_id, const double *templ, int max_shift)
    {
        call("set_drift", sdrx_group_set_drift, sdrx_set_drift, leaf_id, templ, max_shift);
    }
    sdrx_drift_level drift(int leaf_id)
    {
        sdrx_drift_level out;
        call("get_drift", sdrx_group_get_drift, sdrx_get_drift, leaf_id, &out);
        return out;
    }
    std::vector<double> drift_profile(int leaf_id, int max_shift, int64_t *frame = nullptr)
    {
        std::vector<double> profile((size_t)(2 * max_shift + 1));
        call("get_drift_profile", sdrx_group_get_drift_profile, sdrx_get_drift_profile, leaf_id, profile.data(), frame);
        return profile;
    }
    // sdrx.h "Drift estimate": the parabola through the peak and its neighbours; plain shift at the window's edge
    static double drift_bins(const sdrx_drift_level &r)
    {
        const double den = r.left - 2.0 * r.peak + r.right;
        if (r.shift >= r.max_shift || r.shift <= -r.max_shift || den == 0.0)
            return (double)r.shift;
        return r.shift + 0.5 * (r.left - r.right) / den;
    }
    static double drift_hz(const sdrx_drift_level &r, double fs_source) { return drift_bins(r) * fs_source / SDRX_SPECTRUM_BINS; }
    // band scan (part of option "watch"): the carriers in the integrated spectrum of the source of watched leaf `leaf_id`
    // (cfg == nullptr or cell_bins 0: off).  scan(): the record of the last delivered frame; scan_hits() / scan_cells(): the
    // last completed evaluation; scan_hit_hz / scan_mixer_for / scan_unassigned: what a host does with a hit (sdrx.h "Band scan").
    void set_scan(int leaf_id, const sdrx_scan_cfg *cfg) { call("set_scan", sdrx_group_set_scan, sdrx_set_scan, leaf_id, cfg); }
    sdrx_scan_level scan(int leaf_id)
    {
        sdrx_scan_level out;
        call("get_scan", sdrx_group_get_scan, sdrx_get_scan, leaf_id, &out);
        return out;
    }
    std::vector<sdrx_scan_hit> scan_hits(int leaf_id, int64_t *frame = nullptr)
    {
        std::vector<sdrx_scan_hit> hits(SDRX_SCAN_MAX_HITS);
        int n = 0;
        call("get_scan_hits", sdrx_group_get_scan_hits, sdrx_get_scan_hits, leaf_id, hits.data(), (int)hits.size(), &n, frame);
        hits.resize((size_t)n);
        return hits;
    }
    std::vector<double> scan_cells(int leaf_id, int cell_bins, int64_t *frame = nullptr)
    {
        std::vector<double> cells((size_t)(SDRX_SPECTRUM_BINS / cell_bins));
        call("get_scan_cells", sdrx_group_get_scan_cells, sdrx_get_scan_cells, leaf_id, cells.data(), frame);
        return cells;
    }
    struct scan_hz {
        double lo, hi, peak;
    };
    static scan_hz scan_hit_hz(const sdrx_scan_hit &h, int cell_bins, double fs_source)
    {
        const double hz = fs_source / SDRX_SPECTRUM_BINS;
        const int w = cell_bins, half = SDRX_SPECTRUM_BINS / 2;
        return scan_hz{(h.first_cell * w - half) * hz, ((h.first_cell + h.n_cells) * w - 1 - half) * hz, (h.peak_cell * w + (w - 1) / 2.0 - half) * hz};
    }
    // the integer mixer frequency that puts `hz` (of the source) in the middle of the leaf's watch band
    static long long scan_mixer_for(const sdrx_vfo_desc &d, double hz)
    {
        if (!d.demod_usb)
            return std::llrint(-hz);
        const double R = (double)d.fs / (double)(1 << d.decimate_count);
        const double R_out = d.late_decimate == 5 || d.late_decimate == 6 ? R / (double)d.late_decimate : R;
        double B = d.filter_bw_hz > 0 ? (double)d.filter_bw_hz : R_out / 2;
        if (B > R_out / 2)
            B = R_out / 2;
        return std::llrint(B / 2 - hz);
    }
    // the hits whose [lo, hi] overlaps none of the leaf bands `bands` ([lo, hi] pairs in Hz of the source)
    static std::vector<sdrx_scan_hit> scan_unassigned(const std::vector<sdrx_scan_hit> &hits, int cell_bins, double fs_source,
                                                      const std::vector<std::pair<double, double>> &bands)
    {
        std::vector<sdrx_scan_hit> out;
        for (const sdrx_scan_hit &h : hits) {
            const scan_hz z = scan_hit_hz(h, cell_bins, fs_source);
            bool taken = false;
            for (const auto &b : bands)
                taken = taken || (z.lo <= b.second && b.first <= z.hi);
            if (!taken)
                out.push_back(h);
        }
        return out;
    }

private:
    bool started() const { return ctx_ || grp_; }
    void dc_correct(std::vector<float> &x)
    {
        const float keep = 1.0f - 0.000001f, k = 0.000001f;
        for (size_t i = 0; i + 1 < x.size(); i += 2) {
            avept_[0] = avept_[0] * keep + k * x[i];
            avept_[1] = avept_[1] * keep + k * x[i + 1];
            x[i] -= avept_[0];
            x[i + 1] -= avept_[1];
        }
    }
    // the context that holds VFO `id` and its id there
    sdrx_ctx *locate(int id, int *local)
    {
        if (!grp_) {
            *local = id;
            return ctx_;
        }
        int member = -1;
        sdrx_ctx *c = nullptr;
        check(sdrx_group_locate(grp_, id, &member, local), "sdrx_group_locate");
        check(sdrx_group_member(grp_, member, &c, nullptr), "sdrx_group_member");
        return c;
    }
    // fftVFOSlot selected VFOs (vfo.cpp:492-509: EVERY VFO whose topic equals the selected string): tell the library before the
    // frame runs -- a leaf whose late decimation is fused into the mix wave keeps decimate[0] only while it is a tap
    // (sdrx_set_tap replaces the selection of a context, sdrx_add_tap adds to it)
    void select_tap()
    {
        std::vector<vfo *> want;
        for (vfo *v : all_)
            if (v->emitFFT && v->fftData)
                want.push_back(v);
        if (want == taps_)
            return;
        for (sdrx_ctx *c : tap_ctxs_)
            check_ctx(c, sdrx_set_tap(c, -1), "sdrx_set_tap");
        tap_ctxs_.clear();
        for (vfo *v : want) {
            int lid = -1;
            sdrx_ctx *c = locate(v->id, &lid);
            check_ctx(c, sdrx_add_tap(c, lid), "sdrx_add_tap");
            if (std::find(tap_ctxs_.begin(), tap_ctxs_.end(), c) == tap_ctxs_.end())
                tap_ctxs_.push_back(c);
        }
        taps_ = want;
    }
    // vfo::process ends with `if (emitFFT) emit fftData(decimate[decimateCount])` (vfo.cpp:290-293);
    // demodData with `if (count == 4 && emitFFT) { emit fftData(samples); count = 0; } count++`.
    void after_frame(int n_complex)
    {
        for (vfo *v : all_)
            if (v->emitFFT && v->fftData) {
                int n = 0, lid = -1;
                sdrx_ctx *c = locate(v->id, &lid);
                check_ctx(c, sdrx_get_stream(c, lid, nullptr, 0, &n), "sdrx_get_stream");
                tap_.resize((size_t)n);
                check_ctx(c, sdrx_get_stream(c, lid, reinterpret_cast<float *>(tap_.data()), n, &n), "sdrx_get_stream");
                v->fftData(tap_);
            }
        if (count == 4 && emitFFT) {
            if (fftData) {
                int n = 0;
                tap_.resize((size_t)n_complex);
                if (grp_) { // the frame as the host handed it over (after its own LUT / DC removal) ...
                    if (samples_.size() == (size_t)2 * n_complex) {
                        std::memcpy(static_cast<void *>(tap_.data()), samples_.data(), sizeof(float) * samples_.size());
                    } else { // ... or, bytes with the DC removal done on the devices, as the first one holding VFOs kept it
                        sdrx_ctx *c = nullptr;
                        for (int k = 0; k < sdrx_group_size(grp_) && !c; ++k)
                            check(sdrx_group_member(grp_, k, &c, nullptr), "sdrx_group_member");
                        if (c && sdrx_get_raw(c, reinterpret_cast<float *>(tap_.data()), n_complex, &n) == SDRX_OK)
                            tap_.resize((size_t)n);
                        else
                            tap_.clear();
                    }
                } else {
                    check(sdrx_get_raw(ctx_, reinterpret_cast<float *>(tap_.data()), n_complex, &n), "sdrx_get_raw");
                    tap_.resize((size_t)n);
                }
                if (!tap_.empty())
                    fftData(tap_);
            }
            count = 0;
        }
        count++;
    }
    void add(vfo *v, int parent)
    {
        all_.push_back(v);
        if (!v->initialised)
            throw std::runtime_error("vfo::init was not called");
        v->d.parent_id = parent;
        call("add_vfo", sdrx_group_add_vfo, sdrx_add_vfo, &v->d, &v->id);
        if (v->detector != SDRX_DETECT_NONE) {
            if (grp_)
                throw std::runtime_error("vfo::setDetector: groups do not offer detector leaves (include/sdrx.h \"Detector leaves\")");
            sdrx_detect_cfg cfg;
            std::memset(&cfg, 0, sizeof cfg);
            cfg.kind = v->detector;
            check(sdrx_set_detector(ctx_, v->id, &cfg), "sdrx_set_detector");
        }
        if (!v->postTaps.empty()) {
            if (grp_)
                throw std::runtime_error("vfo::setPostFilter: groups do not offer the post-detection filter (include/sdrx.h \"Post-detection filter\")");
            sdrx_postfilter_cfg cfg;
            std::memset(&cfg, 0, sizeof cfg);
            cfg.decim = v->postDecim;
            cfg.ntaps = (int32_t)v->postTaps.size();
            check(sdrx_set_postfilter(ctx_, v->id, &cfg, v->postTaps.data()), "sdrx_set_postfilter");
        }
        if (v->mpVFOs)
            for (vfo *c : *v->mpVFOs)
                add(c, v->id);
    }
    // the call `name` of the ABI on whichever this host runs on: sdrx_group_<name>(grp_, ...) or sdrx_<name>(ctx_, ...)
    template <class GroupFn, class CtxFn, class... Args>
    void call(const char *name, GroupFn group_fn, CtxFn ctx_fn, Args... args)
    {
        const int rc = grp_ ? group_fn(grp_, args...) : ctx_fn(ctx_, args...);
        if (rc != SDRX_OK)
            check(rc, (std::string(grp_ ? "sdrx_group_" : "sdrx_") + name).c_str());
    }
    void check(int rc, const char *what)
    {
        if (rc != SDRX_OK)
            throw std::runtime_error(std::string(what) + ": " + (grp_ ? sdrx_group_last_error(grp_) : sdrx_last_error(ctx_)));
    }
    static void check_ctx(sdrx_ctx *c, int rc, const char *what)
    {
        if (rc != SDRX_OK)
            throw std::runtime_error(std::string(what) + ": " + sdrx_last_error(c));
    }
    static void trampoline(void *user, const char topic[5], uint32_t rate, const void *buf, uint32_t len)
    {
        sdrj *self = static_cast<sdrj *>(user);
        if (self->publish_)
            self->publish_(topic, rate, buf, len);
    }
    std::vector<int> devices_;
    sdrx_ctx *ctx_ = nullptr;
    sdrx_group *grp_ = nullptr;
    std::vector<vfo *> *mpVFOs = nullptr;
    bool correctDC = false;
    bool emitFFT = false;
    int count = 0;
    std::vector<vfo *> all_;
    std::vector<std::complex<float>> tap_;
    std::vector<vfo *> taps_;          // the VFOs the library was last told about (sdrx_add_tap) ...
    std::vector<sdrx_ctx *> tap_ctxs_; // ... and the contexts that hold them
    float avept_[2] = {0.f, 0.f};
    std::vector<float> samples_;
    publish_fn publish_;
    std::map<std::string, int> options_;
    int input_rate_ = 0, rs_taps_ = 32; // setInputRate
    double rs_atten_ = 80.0, rs_passband_ = 0;
    int fr_stages_ = 0, fr_K_ = 15; // setFront
    bool fr_real_ = false;
    double fr_atten_ = 80.0;
    bool bl_on_ = false; // setBlanker
    sdrx_blanker_cfg bl_cfg_{};
    bool iq_on_ = false; // setIqBalance
    sdrx_iq_cfg iq_cfg_{};
    bool sh_on_ = false; // setShift
    double shift_hz_ = 0.0;
    sdrx_shift_cfg shift_cfg() const // shift_hz_ at the first main's rate
    {
        sdrx_shift_cfg cfg{};
        if (sdrx_shift_inc((double)(*mpVFOs)[0]->d.fs, shift_hz_, &cfg.inc) != SDRX_OK)
            throw std::runtime_error("sdrj::setShift: the shift must be finite and at most half the main VFOs' sample rate");
        return cfg;
    }
    bool nt_on_ = false; // setNotch
    std::vector<double> nt_hz_;
    float nt_mu_ = 0, nt_afc_ = 0, nt_coh_ = 0;
    double nt_pull_hz_ = 0.0;
    sdrx_notch_cfg notch_cfg() const // the tones and the pull at the first main's rate
    {
        sdrx_notch_cfg cfg{};
        const double fs = (double)(*mpVFOs)[0]->d.fs;
        cfg.n_tones = (uint32_t)nt_hz_.size();
        cfg.mu = nt_mu_, cfg.afc_gain = nt_afc_, cfg.min_coherence = nt_coh_;
        bool ok = nt_pull_hz_ >= 0 && sdrx_shift_inc(fs, nt_pull_hz_, &cfg.max_pull) == SDRX_OK;
        for (size_t k = 0; ok && k < nt_hz_.size(); ++k)
            ok = sdrx_shift_inc(fs, nt_hz_[k], &cfg.inc0[k]) == SDRX_OK;
        if (!ok)
            throw std::runtime_error("sdrj::setNotch: the tones and the pull must be finite and at most half the main VFOs' sample rate");
        return cfg;
    }
};

// ------------------------------------------------------------------------------------------ INI
// The subset of QSettings::IniFormat the shipped profiles use: [section] headers, key=value with
// blanks trimmed, `N\key` array members (backslash = group separator), top-level keys before any
// section, ';' comment lines.  A leading '#' is NOT a comment for QSettings: such a line defines a
// key nobody reads (sdr_25E.ini:5-9).
inline std::map<std::string, std::string> parse_ini(std::istream &in)
{
    auto trim = [](std::string s) {
        size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
        return a == std::string::npos ? std::string() : s.substr(a, b - a + 1);
    };
    std::map<std::string, std::string> kv;
    std::string line, section;
    while (std::getline(in, line)) {
        line = trim(line);
        if (line.empty() || line[0] == ';')
            continue;
        if (line.front() == '[' && line.back() == ']') {
            section = trim(line.substr(1, line.size() - 2));
            std::string low = section;
            std::transform(low.begin(), low.end(), low.begin(), ::tolower);
            if (low == "general")
                section.clear();
            continue;
        }
        size_t eq = line.find('=');
        if (eq == std::string::npos)
            continue;
        std::string k = trim(line.substr(0, eq)), v = trim(line.substr(eq + 1));
        std::replace(k.begin(), k.end(), '\\', '/');
        if (v.size() >= 2 && v.front() == '"' && v.back() == '"')
            v = v.substr(1, v.size() - 2);
        kv[(section.empty() ? "" : section + "/") + k] = v;
    }
    return kv;
}

// A whole receiver profile: owns the vfo objects; `mains` is what sdrj::setVFOs receives.
struct Profile {
    int fs = 0, frame = 0, bufsplit = 4, center_frequency = 0;
    bool correct_dc = false;
    std::string zmq_address;
    std::vector<std::unique_ptr<vfo>> all; // creation order: mains, then subs in INI order
    std::vector<vfo *> mains;
    std::vector<std::vector<vfo *>> subs; // per main (VFOsub[i], mainwindow.h:82)
};

// ---- the INI front door ----------------------------------------------------------
// The rules by which the reference turns its settings file into a VFO tree (mainwindow.cpp:27-233), restated as
// three small pure steps -- settings access, frame geometry, sub-VFO placement -- and an instantiation step.

// QSettings' view of the parsed file: missing or malformed numbers read as 0 (QVariant::toInt / toFloat).
class Settings {
public:
    explicit Settings(std::map<std::string, std::string> kv) : kv_(std::move(kv)) {}
    std::string text(const std::string &key) const
    {
        auto it = kv_.find(key);
        return it == kv_.end() ? std::string() : it->second;
    }
    int integer(const std::string &key) const
    {
        const std::string s = text(key);
        if (s.empty())
            return 0;
        char *end = nullptr;
        const long long v = std::strtoll(s.c_str(), &end, 10);
        return (*end != 0 || v < INT32_MIN || v > INT32_MAX) ? 0 : (int)v;
    }
    float real(const std::string &key) const
    {
        const std::string s = text(key);
        char *end = nullptr;
        const float v = std::strtof(s.c_str(), &end);
        return (s.empty() || *end != 0) ? 0.0f : v;
    }
    // `N\\key` array members of QSettings::beginReadArray(group): "<group>/<i>/<key>", i = 1 .. size
    std::string item(const std::string &group, int i, const char *key) const { return group + "/" + std::to_string(i) + "/" + key; }

private:
    std::map<std::string, std::string> kv_;
};

// How many floats the ingest delivers per callback: a quarter of a second of I/Q, or a fifth where a quarter
// is not a multiple of 512 floats (288 kS/s) -- mainwindow.cpp:65-80.
struct FrameGeometry {
    int floats_per_callback, callbacks_per_second;
    int complex_per_frame() const { return floats_per_callback / 2; }
};
inline FrameGeometry frame_geometry(int sample_rate)
{
    const int quarter = 2 * sample_rate / 4;
    if (quarter % 512 == 0)
        return {quarter, 4};
    return {2 * sample_rate / 5, 5};
}

// Where a sub VFO hangs and how it decimates, decided from the mains already configured
// (mainwindow.cpp:179-216): the first IQ main whose output band covers the channel; below a 240 k / 288 k main
// the last step to 48 k is the /5 or /6 FIR ("late decimation"), the half-bands do the rest.
struct SubPlacement {
    int main_index = 0, input_rate = 0, parent_mixer = 0, halfband_stages = 0, late_decimate = 0;
};
inline SubPlacement place_sub(const std::vector<vfo *> &mains, int receiver_rate, int center, int channel_freq, int out_rate)
{
    SubPlacement pl;
    pl.input_rate = receiver_rate;
    for (size_t a = 0; a < mains.size(); ++a) {
        vfo &m = *mains[a];
        const int main_centre = center - (int)m.getMixerFreq();
        if (std::abs(main_centre - channel_freq) < m.getOutRate() && !m.getDemodUSB()) {
            pl.main_index = (int)a;
            pl.parent_mixer = (int)m.getMixerFreq();
            pl.input_rate = m.getOutRate();
            break;
        }
    }
    const int fir_step = pl.input_rate / 48000; // 5 below a 240 k main, 6 below a 288 k one
    if (fir_step == 5 || fir_step == 6) {
        pl.late_decimate = fir_step;
        pl.halfband_stages = (int)std::log2(pl.input_rate / (fir_step * out_rate));
    } else {
        pl.halfband_stages = (int)std::log2(receiver_rate / out_rate) - (int)std::log2(receiver_rate / pl.input_rate);
    }
    return pl;
}

inline std::unique_ptr<Profile> load_profile(std::istream &in)
{
    const Settings ini(parse_ini(in));
    auto prof = std::unique_ptr<Profile>(new Profile());
    Profile &P = *prof;
    P.fs = ini.integer("sample_rate");
    if (P.fs == 0)
        throw std::runtime_error("sample_rate ini file key not found or equal to zero"); // mainwindow.cpp:31-37
    if (P.fs != 288000 && P.fs != 1536000 && P.fs != 1920000)                            // mainwindow.h:29
        throw std::runtime_error("sample_rate " + std::to_string(P.fs) + " not supported");
    const FrameGeometry geo = frame_geometry(P.fs);
    P.frame = geo.complex_per_frame();
    P.bufsplit = geo.callbacks_per_second;
    P.center_frequency = ini.integer("center_frequency");
    P.zmq_address = ini.text("zmq_address");
    P.correct_dc = ini.text("correct_dc_bias") == "1";
    const int channel_offset = ini.integer("mix_offset");

    // main VFOs: IQ only, compress() style 1, fed by the raw stream (mainwindow.cpp:98-138)
    const int n_mains = std::max(0, ini.integer("main_vfos/size"));
    P.subs.resize((size_t)n_mains);
    for (int i = 1; i <= n_mains; ++i) {
        auto key = [&](const char *k) { return ini.item("main_vfos", i, k); };
        const int out_rate = ini.integer(key("out_rate"));
        if (out_rate <= 0)
            throw std::runtime_error(key("out_rate") + " missing");
        P.all.emplace_back(new vfo());
        vfo &m = *P.all.back();
        if (const int scale = ini.integer(key("compress_scale")))
            if (scale > 0)
                m.setScaleComp(scale);
        if (!ini.text(key("zmq_address")).empty() && !ini.text(key("zmq_topic")).empty()) {
            m.setZmqAddress(ini.text(key("zmq_address")));
            m.setZmqTopic(ini.text(key("zmq_topic")));
        }
        m.setFs(P.fs);
        m.setDecimationCount(P.fs / out_rate == 1 ? 0 : (int)std::log2(P.fs / out_rate));
        m.setMixerFreq(P.center_frequency - ini.integer(key("frequency")));
        m.setDemodUSB(false);
        m.setCompressonStyle(1);
        m.init(P.frame, false);
        m.setVFOs(&P.subs[(size_t)i - 1]);
        P.mains.push_back(&m);
    }

    // sub VFOs: USB audio leaves under the main that covers them (mainwindow.cpp:141-233)
    const int n_subs = ini.integer("vfos/size");
    for (int i = 1; i <= n_subs; ++i) {
        auto key = [&](const char *k) { return ini.item("vfos", i, k); };
        int out_rate = ini.integer(key("out_rate"));
        if (out_rate == 0) { // the older profiles give the data rate of the channel instead
            const int data_rate = ini.integer(key("data_rate"));
            if (data_rate > 0)
                out_rate = data_rate == 600 ? 12000 : data_rate == 1200 ? 24000 : 48000;
        }
        // `detector=am|fm` (no key of the reference, which ignores keys it does not know): the entry leaves as an AM envelope or an
        // FM discriminator in int16 and is placed as a 48 kS/s sub is
        std::string det = ini.text(key("detector"));
        for (char &ch : det)
            ch = (char)std::tolower((unsigned char)ch);
        if (!det.empty() && det != "am" && det != "fm")
            throw std::runtime_error(ini.item("vfos", i, "") + ": detector=" + det + ": only am and fm are offered");
        // `post_decim`, `post_taps`, `post_cutoff_hz`, `post_atten_db` (no keys of the reference): all four or none, on an entry with
        // `detector=` -- its post-detection filter, designed at the leaf's rate
        const char *post_keys[4] = {"post_decim", "post_taps", "post_cutoff_hz", "post_atten_db"};
        std::string post_val[4];
        int post_given = 0;
        for (int k = 0; k < 4; ++k) {
            post_val[k] = ini.text(key(post_keys[k]));
            post_given += !post_val[k].empty();
        }
        if (post_given != 0 && post_given != 4)
            throw std::runtime_error(ini.item("vfos", i, "") + ": the post-detection filter takes all four keys or none (post_decim, post_taps, "
                                                              "post_cutoff_hz, post_atten_db)");
        if (post_given && det.empty())
            throw std::runtime_error(ini.item("vfos", i, "") + ": post_decim, post_taps, post_cutoff_hz and post_atten_db belong to an entry with detector=am|fm");
        if (!det.empty() && out_rate == 0)
            out_rate = 48000;
        if (out_rate <= 0)
            throw std::runtime_error(ini.item("vfos", i, "") + ": neither out_rate nor data_rate given");
        if (P.mains.empty())
            throw std::runtime_error("profile has sub VFOs but no main VFO");
        const int channel = ini.integer(key("frequency")) + channel_offset;
        const SubPlacement pl = place_sub(P.mains, P.fs, P.center_frequency, channel, out_rate);
        P.all.emplace_back(new vfo());
        vfo &v = *P.all.back();
        v.setZmqTopic(ini.text(key("topic")));
        v.setZmqAddress(P.zmq_address);
        v.setDecimationCount(pl.halfband_stages);
        v.setFilterBandwidth(ini.integer(key("filter_bandwidth")));
        v.setGain(ini.real(key("gain")) / 100);
        v.setMixerFreq((P.center_frequency - pl.parent_mixer) - channel);
        v.setFs(pl.input_rate);
        v.setCompressonStyle(1);
        if (!det.empty()) {
            if (pl.late_decimate)
                throw std::runtime_error(ini.item("vfos", i, "") + ": detector=" + det + " below a main VFO of " + std::to_string(pl.input_rate) +
                                         " S/s would need the late decimation by " + std::to_string(pl.late_decimate) +
                                         ", which runs in front of the USB demodulation only: give the entry a main VFO whose out_rate is a "
                                         "power of two times its own");
            v.setDemodUSB(false);
            v.setFilterBandwidth(0);
            v.setCompressonStyle(0);
            v.setDetector(det == "am" ? SDRX_DETECT_AM : SDRX_DETECT_FM);
            if (post_given) {
                const int R = std::atoi(post_val[0].c_str()), T = std::atoi(post_val[1].c_str());
                const int n = (pl.input_rate / P.bufsplit) >> v.d.decimate_count;
                const double rate = (double)(pl.input_rate >> v.d.decimate_count);
                const std::string where = ini.item("vfos", i, "") + ": post-detection filter: ";
                if (T < 1 || T > SDRX_POSTFILTER_MAX_TAPS)
                    throw std::runtime_error(where + "ntaps must be 1 .. 256");
                if (R < 1 || R > SDRX_POSTFILTER_MAX_DECIM)
                    throw std::runtime_error(where + "decim must be 1 .. 16");
                if (n % R)
                    throw std::runtime_error(where + "the leaf's samples per frame are not a multiple of decim");
                std::vector<float> taps((size_t)T);
                const int rc = sdrx_postfilter_design(rate, std::atof(post_val[2].c_str()), T, std::atof(post_val[3].c_str()), taps.data(), T, nullptr);
                if (rc != SDRX_OK)
                    throw std::runtime_error(where + sdrx_last_error(nullptr));
                v.setPostFilter(taps, R);
            }
        }
        v.init(pl.input_rate / P.bufsplit, true, pl.late_decimate);
        P.subs[(size_t)pl.main_index].push_back(&v);
    }
    return prof;
}

inline std::unique_ptr<Profile> load_profile_file(const std::string &path)
{
    std::ifstream f(path);
    if (!f)
        throw std::runtime_error("Given settings ini file doesn't exist: " + path); // mainwindow.cpp:20-25
    return load_profile(f);
}

} // namespace sdrx_host
