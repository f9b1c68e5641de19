// host/demo.cpp -- drives the C++ host layer (host/sdrx_host.hpp) the way the reference's
// MainWindow + sdrj do: read a profile INI, build the VFO tree through the vfo setters, feed
// frames to sdrj::demodData, receive every leaf's payload through the publish hook.
//
//   sdrx_demo <profile.ini> --dump              descriptors as JSON lines (no GPU needed)
//                                               (a [vfos] entry with detector=am|fm is a detector leaf: int16 messages at 48 kS/s,
//                                               or at 48 kS/s / post_decim behind post_decim, post_taps, post_cutoff_hz, post_atten_db)
//   sdrx_demo <profile.ini> --frames N [--u8] [--format cu8|cs8|cs16|rs16|ru12] [--adc] [--input-rate HZ]
//                                   [--front-stages N [--front-real] [--front-taps K]] [--blanker RATIO,GUARD[,FLOOR[,RANK]]]
//                                   [--iq-balance MU,MINPOWER[,C0,D0]] [--shift HZ] [--notch HZ[,HZ...]:MU[,AFC,COH,PULLHZ]]
//                                   [--fft TOPIC] [--devices 0,1,...]
//                                               N synthetic LCG frames; one line per published
//                                               message: frame topic rate bytes fnv1a64(payload)
//                                               --u8 feeds them as dongle bytes, --format as integer samples of that
//                                               format (the same sample values in each: the same messages); neither: floats
//                                               --adc (library option adc_meter): one more line per frame behind its messages,
//                                               adc frame fmt n sum_i sum_q sum_sq_i sum_sq_q sum_iq min_i max_i min_q max_q
//                                               at_rail longest_rail_run bits_used | peak headroom_db dc_i dc_q rms
//                                               (adc frame unmeasured for a frame of floats)
//                                               --input-rate HZ: the frames are at HZ, not at the profile's sample rate, and
//                                               the library's resampler makes the tree's frames from them; first line
//                                               resampler fs_in fs_out L M taps_per_phase in_frame out_frame delay passband_hz
//                                               --front-stages N: N half-band decimations by 2 on the device in front of that (or
//                                               of the tree), the library's design with 4 K + 3 taps (--front-taps K, default 15);
//                                               the frames have 2^N times the samples.  --front-real: they are REAL samples,
//                                               --format rs16 (int16) or ru12 (12-bit offset codes in uint16).  Next line
//                                               front real_input stages K N in_frame out_frame tw alias_free
//                                               --blanker RATIO,GUARD[,FLOOR[,RANK]]: the impulse blanker on the device (FLOOR 0,
//                                               RANK 32768 -- the median -- unless given); one more line per frame behind its
//                                               messages (in front of the adc line),
//                                               blanker frame thr_bits ref_bin next_ref_bin hits blanked runs carry_in
//                                               --iq-balance MU,MINPOWER[,C0,D0]: the IQ balance correction on the device (C0 0,
//                                               D0 1 unless given); one more line per frame behind its messages (in front of
//                                               the blanker line),
//                                               iq frame measured adapted rejected c_bits d_bits next_c_bits next_d_bits
//                                                  sum_i sum_q sum_iq sum_ii sum_qq
//                                               --shift HZ: the frequency shift on the device, HZ at the main VFOs' rate; one
//                                               more line per frame behind its messages (in front of the iq line),
//                                               shift frame phase inc next_phase next_inc      (8 hex digits each)
//                                               --notch HZ[,HZ...]:MU[,AFC,COH,PULLHZ]: the spur canceller on the device, up to eight
//                                               tones in HZ at the main VFOs' rate (AFC 1, COH 0.5, PULLHZ 100 unless given); one
//                                               more line per frame behind its messages (in front of the shift line),
//                                               notch frame blocks then per tone: tracked_hz inc inc_next a_re_bits a_im_bits
//                                                  coherent adapted clamped rejected
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>

#include "sdrx_host.hpp"

using namespace sdrx_host;

static uint64_t fnv1a(const void *p, size_t n)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) {
        h ^= b[i];
        h *= 1099511628211ull;
    }
    return h;
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s profile.ini --dump | --frames N [--u8] [--format cu8|cs8|cs16|rs16|ru12] [--adc] [--input-rate HZ] [--front-stages N [--front-real] [--front-taps K]] [--blanker RATIO,GUARD[,FLOOR[,RANK]]] [--iq-balance MU,MINPOWER[,C0,D0]] [--shift HZ] [--notch HZ[,HZ...]:MU[,AFC,COH,PULLHZ]] [--fft TOPIC] [--devices 0,1,...]\n", argv[0]);
        return 2;
    }
    try {
        auto P = load_profile_file(argv[1]);
        const std::string mode = argv[2];
        if (mode == "--dump") {
            std::printf("{\"fs\": %d, \"frame\": %d, \"bufsplit\": %d, \"correct_dc\": %d, \"n\": %zu}\n", P->fs, P->frame, P->bufsplit,
                        (int)P->correct_dc, P->all.size());
            // creation order with parents resolved: mains, then each main's subs
            for (size_t m = 0; m < P->mains.size(); ++m) {
                const sdrx_vfo_desc &d = P->mains[m]->d;
                std::printf("{\"main\": %zu, \"fs\": %d, \"d\": %d, \"mixer\": %.1f, \"usb\": %d, \"spb\": %d, \"scalecomp\": %d}\n", m, d.fs,
                            d.decimate_count, d.mixer_freq_hz, d.demod_usb, d.samples_per_buffer, d.scalecomp);
            }
            for (size_t m = 0; m < P->subs.size(); ++m)
                for (vfo *v : P->subs[m]) {
                    const sdrx_vfo_desc &d = v->d;
                    std::printf("{\"sub_of\": %zu, \"topic\": \"%s\", \"fs\": %d, \"d\": %d, \"late\": %d, \"mixer\": %.1f, \"bw\": %d, "
                                "\"gain\": %.9g, \"spb\": %d, \"usb\": %d, \"detector\": %d, \"post_decim\": %d, \"post_taps\": [",
                                m, v->topic.c_str(), d.fs, d.decimate_count, d.late_decimate, d.mixer_freq_hz, d.filter_bw_hz, (double)d.gain,
                                d.samples_per_buffer, d.demod_usb, v->getDetector(), v->getPostDecim());
                    for (size_t t = 0; t < v->getPostTaps().size(); ++t)
                        std::printf("%s%.9g", t ? ", " : "", (double)v->getPostTaps()[t]);
                    std::printf("]}\n");
                }
            return 0;
        }
        if (mode != "--frames" || argc < 4)
            throw std::runtime_error("bad arguments");
        const int frames = std::atoi(argv[3]);
        bool u8 = false, adc = false;
        int fmt = SDRX_FMT_CU8, input_rate = 0, front_stages = 0, front_K = 15;
        bool front_real = false, blanker = false;
        float bl_ratio = 0, bl_floor = 0;
        int bl_guard = 0, bl_rank = 32768;
        bool iq_balance = false;
        float iq_mu = 0, iq_min_power = 0, iq_c0 = 0, iq_d0 = 1;
        bool shift = false;
        double shift_hz = 0;
        bool notch = false;
        std::vector<double> notch_hz;
        float notch_mu = 0, notch_afc = 1.0f, notch_coh = 0.5f;
        double notch_pull = 100.0;
        std::string fft_topic;
        std::vector<int> devices;
        for (int a = 4; a < argc; ++a) {
            if (std::string(argv[a]) == "--u8")
                u8 = true;
            else if (std::string(argv[a]) == "--format" && a + 1 < argc) {
                const std::string f = argv[++a];
                if (f != "cu8" && f != "cs8" && f != "cs16" && f != "rs16" && f != "ru12")
                    throw std::runtime_error("--format takes cu8, cs8 or cs16, or with --front-real rs16 or ru12");
                fmt = f == "cu8" ? SDRX_FMT_CU8 : f == "cs8" ? SDRX_FMT_CS8 : f == "cs16" ? SDRX_FMT_CS16 : f == "rs16" ? SDRX_FMT_RS16 : SDRX_FMT_RU12;
                u8 = true;
            } else if (std::string(argv[a]) == "--adc")
                adc = true;
            else if (std::string(argv[a]) == "--input-rate" && a + 1 < argc)
                input_rate = std::atoi(argv[++a]);
            else if (std::string(argv[a]) == "--front-stages" && a + 1 < argc)
                front_stages = std::atoi(argv[++a]);
            else if (std::string(argv[a]) == "--front-taps" && a + 1 < argc)
                front_K = std::atoi(argv[++a]);
            else if (std::string(argv[a]) == "--front-real")
                front_real = true;
            else if (std::string(argv[a]) == "--blanker" && a + 1 < argc) {
                const int got = std::sscanf(argv[++a], "%f,%d,%f,%d", &bl_ratio, &bl_guard, &bl_floor, &bl_rank);
                if (got < 2)
                    throw std::runtime_error("--blanker takes RATIO,GUARD[,FLOOR[,RANK]]");
                blanker = true;
            } else if (std::string(argv[a]) == "--iq-balance" && a + 1 < argc) {
                const int got = std::sscanf(argv[++a], "%f,%f,%f,%f", &iq_mu, &iq_min_power, &iq_c0, &iq_d0);
                if (got != 2 && got != 4)
                    throw std::runtime_error("--iq-balance takes MU,MINPOWER[,C0,D0]");
                iq_balance = true;
            } else if (std::string(argv[a]) == "--shift" && a + 1 < argc) {
                if (std::sscanf(argv[++a], "%lf", &shift_hz) != 1)
                    throw std::runtime_error("--shift takes HZ");
                shift = true;
            } else if (std::string(argv[a]) == "--notch" && a + 1 < argc) {
                const std::string spec = argv[++a];
                const size_t colon = spec.find(':');
                if (colon == std::string::npos)
                    throw std::runtime_error("--notch takes HZ[,HZ...]:MU[,AFC,COH,PULLHZ]");
                std::stringstream tones(spec.substr(0, colon));
                for (std::string item; std::getline(tones, item, ',');) {
                    double v = 0;
                    if (std::sscanf(item.c_str(), "%lf", &v) != 1)
                        throw std::runtime_error("--notch: a tone is a number of Hz");
                    notch_hz.push_back(v);
                }
                const int got = std::sscanf(spec.c_str() + colon + 1, "%f,%f,%f,%lf", &notch_mu, &notch_afc, &notch_coh, &notch_pull);
                if ((got != 1 && got != 4) || notch_hz.empty())
                    throw std::runtime_error("--notch takes HZ[,HZ...]:MU[,AFC,COH,PULLHZ]");
                notch = true;
            } else if (std::string(argv[a]) == "--fft" && a + 1 < argc)
                fft_topic = argv[++a];
            else if (std::string(argv[a]) == "--devices" && a + 1 < argc) { // one tree sharded over several GPUs
                std::stringstream ss(argv[++a]);
                std::string tok;
                while (std::getline(ss, tok, ','))
                    devices.push_back(std::atoi(tok.c_str()));
            }
        }
        if (devices.empty())
            devices.push_back(0);
        sdrj radio(devices);
        radio.setVFOs(&P->mains);
        radio.setDCCorrection(P->correct_dc);
        if (adc)
            radio.setOption("adc_meter", 1);
        int frame_no = 0;
        radio.setPublisher([&](const char topic[5], uint32_t rate, const void *buf, uint32_t len) {
            char t[6] = {0, 0, 0, 0, 0, 0};
            std::memcpy(t, topic, 5);
            std::printf("%d %s %u %u %016" PRIx64 "\n", frame_no, t, rate, len, fnv1a(buf, len));
        });
        // --fft TOPIC: what the GUI's spectrum selector does -- every vfo and the sdrj get fftVFOSlot(TOPIC)
        auto tap = [&](const char *who) {
            return [&frame_no, who](const std::vector<std::complex<float>> &d) {
                std::printf("fft %d %s %zu %016" PRIx64 "\n", frame_no, who, d.size(), fnv1a(d.data(), d.size() * sizeof(d[0])));
            };
        };
        if (!fft_topic.empty()) {
            for (auto &up : P->all) {
                vfo *v = up.get();
                v->fftData = tap(v->topic.c_str());
                v->fftVFOSlot(fft_topic);
            }
            radio.fftData = tap("Main");
            radio.fftVFOSlot(fft_topic);
        }
        const bool real_fmt = fmt == SDRX_FMT_RS16 || fmt == SDRX_FMT_RU12;
        if (real_fmt != front_real)
            throw std::runtime_error("--format rs16 / ru12 and --front-real (with --front-stages) go together");
        if (real_fmt)
            radio.setDCCorrection(false); // (the library removes no DC from real samples: it lands at the band's edge)
        int n_frame = P->frame; // samples of a frame as it is handed over
        if (input_rate > 0)
            radio.setInputRate(input_rate);
        if (front_stages > 0)
            radio.setFront(front_stages, front_real, front_K);
        if (blanker)
            radio.setBlanker(bl_ratio, bl_guard, bl_floor, bl_rank);
        if (iq_balance)
            radio.setIqBalance(iq_mu, iq_min_power, iq_c0, iq_d0);
        if (shift)
            radio.setShift(shift_hz);
        if (notch)
            radio.setNotch(notch_hz, notch_mu, notch_afc, notch_coh, notch_pull);
        if (input_rate > 0 || front_stages > 0)
            radio.start();
        if (input_rate > 0) {
            const sdrx_resampler_info R = radio.resampler();
            n_frame = R.in_frame;
            std::printf("resampler %d %d %d %d %d %d %d %.6f %.3f\n", R.fs_in, R.fs_out, R.L, R.M, R.taps_per_phase, R.in_frame, R.out_frame,
                        R.delay_out_samples, R.passband_hz);
        }
        if (front_stages > 0) {
            const sdrx_front_info F = radio.front();
            n_frame = F.in_frame;
            std::printf("front %d %d %d %d %d %d %.9f %.9f\n", F.real_input, F.stages, F.K, F.N, F.in_frame, F.out_frame, F.tw, F.alias_free);
        }
        // synthetic IQ of BASELINE.md: LCG x <- x*1664525 + 1013904223, component ((x >> 24) % 17) - 8
        uint32_t x = 1;
        std::vector<float> iq((size_t)2 * n_frame);
        std::vector<uint8_t> bytes((size_t)2 * n_frame);
        std::vector<int8_t> s8(fmt == SDRX_FMT_CS8 ? bytes.size() : 0);
        std::vector<int16_t> s16(fmt == SDRX_FMT_CS16 ? bytes.size() : 0);
        std::vector<uint16_t> r16(real_fmt ? (size_t)n_frame : 0); // real samples: one component a sample
        for (frame_no = 0; frame_no < frames; ++frame_no) {
            for (size_t i = 0; i < iq.size(); ++i) {
                x = x * 1664525u + 1013904223u;
                const int c = (int)((x >> 24) % 17u) - 8;
                iq[i] = (float)c;
                bytes[i] = (uint8_t)(c + 127);
                if (fmt == SDRX_FMT_CS8)
                    s8[i] = (int8_t)c;
                else if (fmt == SDRX_FMT_CS16)
                    s16[i] = (int16_t)(256 * c); // c * 2^8: the same sample value
                else if (real_fmt && i < r16.size())
                    r16[i] = fmt == SDRX_FMT_RS16 ? (uint16_t)(int16_t)(256 * c) : (uint16_t)(16 * c + 2048); // the same value in both
            }
            if (real_fmt)
                radio.demodSamples(r16.data(), n_frame, fmt);
            else if (fmt == SDRX_FMT_CS8)
                radio.demodSamples(s8.data(), n_frame, fmt);
            else if (fmt == SDRX_FMT_CS16)
                radio.demodSamples(s16.data(), n_frame, fmt);
            else if (u8)
                radio.demodBytes(bytes.data(), n_frame);
            else
                radio.demodData(iq.data(), (int)iq.size());
            if (notch) {
                const sdrx_notch_record r = radio.notch();
                std::printf("notch %d %u", frame_no, r.blocks);
                for (uint32_t k = 0; k < r.n_tones; ++k)
                    std::printf(" %.3f %08x %08x %08x %08x %u %u %u %u", radio.notchHz(r, (int)k), r.tone[k].inc, r.tone[k].inc_next, r.tone[k].a_re_bits,
                                r.tone[k].a_im_bits, r.tone[k].coherent, r.tone[k].adapted, r.tone[k].clamped, r.tone[k].rejected);
                std::printf("\n");
            }
            if (shift) {
                const sdrx_shift_record s = radio.shift();
                std::printf("shift %d %08x %08x %08x %08x\n", frame_no, s.phase, s.inc, s.next_phase, s.next_inc);
            }
            if (iq_balance) {
                const sdrx_iq_record q = radio.iqBalance();
                std::printf("iq %d %u %u %u %08x %08x %08x %08x %" PRId64 " %" PRId64 " %" PRId64 " %" PRIu64 " %" PRIu64 "\n", frame_no, q.measured, q.adapted,
                            q.rejected, q.c_bits, q.d_bits, q.next_c_bits, q.next_d_bits, q.sum_i, q.sum_q, q.sum_iq, q.sum_ii, q.sum_qq);
            }
            if (blanker) {
                const sdrx_blanker_record b = radio.blanker();
                std::printf("blanker %d %08x %d %d %u %u %u %u\n", frame_no, b.thr_bits, b.ref_bin, b.next_ref_bin, b.hits, b.blanked, b.runs, b.carry_in);
            }
            if (adc) {
                const sdrx_adc_meter r = radio.adcMeter();
                if (!r.measured) {
                    std::printf("adc %d unmeasured\n", frame_no);
                    continue;
                }
                const adc_levels_t L = adc_levels(r);
                std::printf("adc %d %s %u %" PRId64 " %" PRId64 " %" PRIu64 " %" PRIu64 " %" PRId64 " %d %d %d %d %u %u %d | %.6g %.3f %.6g %.6g %.6g\n", frame_no,
                            r.fmt == SDRX_FMT_CU8 ? "cu8" : r.fmt == SDRX_FMT_CS8 ? "cs8" : r.fmt == SDRX_FMT_CS16 ? "cs16" : r.fmt == SDRX_FMT_RS16 ? "rs16" : "ru12", r.n_complex, r.i.sum, r.q.sum, r.i.sum_sq, r.q.sum_sq,
                            r.sum_iq, r.i.min, r.i.max, r.q.min, r.q.max, r.i.at_lo + r.i.at_hi + r.q.at_lo + r.q.at_hi, L.longest_rail_run,
                            L.bits_used, L.peak, L.headroom_db, L.dc_i, L.dc_q, L.rms);
            }
        }
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "sdrx_demo: %s\n", e.what());
        return 1;
    }
}
