// oracle/ref/sdrj_harness.cpp -- TEST INFRASTRUCTURE, not product code.
//
// extern "C" driver around the UNMODIFIED reference classes `sdr` (jonti/sdr.cpp) and
// `sdrj` (sdrj.cpp), compiled from the sources where they lie (oracle/ref/Makefile) into
// oracle/_ref/libsdrjref.so (-O2) and libsdrjref_ofast.so (-Ofast, as shipped).  It pins
// the first two stages of the hot path to the real code: the byte -> float LUT of
// sdr::sdr (jonti/sdr.cpp:43-49, read through floats.at() exactly as rtlsdr_callback and
// sdrj::readyRead do) and the DC-bias IIR of sdrj::demodData (sdrj.cpp:266-305), with the
// every-4th-call raw spectrum signal and, optionally, real vfo roots behind it (built with
// the ref_vfo_* functions of harness.cpp, linked into the same library).
//
// ONE STREAM PER PROCESS.  demodData keeps its DC estimate `avept` in a function-static
// variable (sdrj.cpp:280): it is created once per loaded library, is shared by every sdrj
// object and cannot be reset.  A caller that needs a stream from the zero state must load
// the library in a fresh process (tests/sdrj_ref_worker.py does; oracle/binding.py
// sdrj_run starts it).
//
// librtlsdr is not part of this build: oracle/ref/rtl-sdr.h declares the entry points
// the two sources name, and the stubs at the end of this file fail every call.
//
// sdrj keeps `samples` private; as in harness.cpp the harness reads it by spelling
// `private` as `public` -- for sdrj.h only.  The std, Qt, jonti/sdr.h and vfo.h headers
// are included first, with their access untouched (libstdc++'s <sstream> does not
// compile with `private` redefined).
#include <cstdint>
#include <cstring>
#include <complex>
#include <sstream>
#include <string>
#include <vector>
#include <QObject>
#include <QString>
#include <QVector>
#include <QTcpSocket>
#include "jonti/sdr.h"
#include "vfo.h"

#define private public
#include "sdrj.h"
#undef private

namespace {

struct Handle {
    sdrj *s;
    QVector<vfo *> *roots;
    long calls = 0;                       // demodData calls since the last fftVFOSlot
    std::vector<long> fft_calls;          // 1-based call index of every fftData emission
    std::vector<std::vector<cpx_typef>> fft_data;
};

Handle *H(void *h) { return static_cast<Handle *>(h); }

} // namespace

extern "C" {

// sdrj's constructor leaves mpVFOs and emitFFT unset (sdrj.cpp:4-18): set both here.
// The vector stays empty unless sdrjh_add_root attaches vfo roots.
void *sdrjh_new()
{
    Handle *h = new Handle();
    h->s = new sdrj();
    h->roots = new QVector<vfo *>();
    h->s->setVFOs(h->roots);
    h->s->fftVFOSlot(QString("none"));
    QObject::connect(h->s, &sdrj::fftData, [h](const std::vector<cpx_typef> &d) {
        h->fft_calls.push_back(h->calls);
        h->fft_data.push_back(d);
    });
    return h;
}

// A root made by ref_vfo_new/ref_vfo_init of this library.  ~sdrj deletes the roots.
void sdrjh_add_root(void *h, void *v) { H(h)->roots->push_back(static_cast<vfo *>(v)); }

void sdrjh_set_dc_correction(void *h, int on) { H(h)->s->setDCCorrection(on != 0); }

void sdrjh_fft_vfo_slot(void *h, const char *topic)
{
    H(h)->calls = 0;
    H(h)->s->fftVFOSlot(QString::fromUtf8(topic));
}

// Bytes -> floats through the real LUT: `floats.at(buf[i])` (jonti/sdr.cpp:125, sdrj.cpp:158).
void sdrjh_bytes_to_floats(void *h, const unsigned char *b, long n, float *out)
{
    const sdr *base = H(h)->s;
    for (long i = 0; i < n; ++i)
        out[i] = base->floats.at(b[i]);
}

// One call of sdrj::demodData(data, len): `len` floats, i.e. len/2 complex samples.
void sdrjh_demod(void *h, const float *data, int len)
{
    ++H(h)->calls;
    H(h)->s->demodData(data, len);
}

// sdrj::samples after the last demodData, as interleaved floats; returns its length.
int sdrjh_get_samples(void *h, float *out, int max_complex)
{
    const std::vector<cpx_typef> &s = H(h)->s->samples;
    int n = (int)s.size() < max_complex ? (int)s.size() : max_complex;
    if (n > 0)
        std::memcpy(out, s.data(), sizeof(cpx_typef) * (size_t)n);
    return (int)s.size();
}

int sdrjh_fft_count(void *h) { return (int)H(h)->fft_calls.size(); }
long sdrjh_fft_call(void *h, int k) { return H(h)->fft_calls.at(k); }

int sdrjh_fft_get(void *h, int k, float *out, int max_complex)
{
    const std::vector<cpx_typef> &s = H(h)->fft_data.at(k);
    int n = (int)s.size() < max_complex ? (int)s.size() : max_complex;
    if (n > 0)
        std::memcpy(out, s.data(), sizeof(cpx_typef) * (size_t)n);
    return (int)s.size();
}

// ---------------------------------------------------------------- librtlsdr stubs
uint32_t rtlsdr_get_device_count(void) { return 0; }
const char *rtlsdr_get_device_name(uint32_t) { return ""; }
int rtlsdr_get_device_usb_strings(uint32_t, char *, char *, char *) { return -1; }
int rtlsdr_get_index_by_serial(const char *) { return -1; }
int rtlsdr_open(rtlsdr_dev_t **dev, uint32_t)
{
    if (dev)
        *dev = 0;
    return -1;
}
int rtlsdr_close(rtlsdr_dev_t *) { return -1; }
int rtlsdr_set_center_freq(rtlsdr_dev_t *, uint32_t) { return -1; }
int rtlsdr_set_tuner_gain_mode(rtlsdr_dev_t *, int) { return -1; }
int rtlsdr_set_tuner_gain(rtlsdr_dev_t *, int) { return -1; }
int rtlsdr_set_sample_rate(rtlsdr_dev_t *, uint32_t) { return -1; }
int rtlsdr_set_agc_mode(rtlsdr_dev_t *, int) { return -1; }
int rtlsdr_set_bias_tee(rtlsdr_dev_t *, int) { return -1; }
int rtlsdr_reset_buffer(rtlsdr_dev_t *) { return -1; }
int rtlsdr_read_async(rtlsdr_dev_t *, rtlsdr_read_async_cb_t, void *, uint32_t, uint32_t) { return -1; }
int rtlsdr_cancel_async(rtlsdr_dev_t *) { return -1; }

} // extern "C"
