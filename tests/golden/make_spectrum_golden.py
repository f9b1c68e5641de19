"""Developer-time generator of tests/golden/spectrum.npz: the spectrum display pinned to the REAL kiss_fft.

    python3 tests/golden/make_spectrum_golden.py /path/to/SDRReceiver

Compiles the reference's own kiss_fft130/kiss_fft.c, untouched, with gcc -O2 (no -march: what the reference's qmake build
gives it) and once more with -Ofast (for information), next to a small driver written here, in a temporary directory
outside the repository.  Never run by build(), the tests, smoke() or bench.py.

The driver, per input: the Hann table (mainwindow.cpp:284-287's double expression, stored as float), the windowed input
(complex<float> * float, zero-padded past the input's length), kiss_fft of 8192 points (kiss_fft_alloc + kiss_fft), and a C++
restatement of fftHandlerSlot's power step in the project's own words (float im*im + re*re, float sqrt, glibc log10 in
double, the reference's visiting order for maxval / aveval, the "< 10 dB" rule, the 5-point smooth).

The inputs are regenerated bit for bit by tests/spectrum_ref.py (integer LCG noise, float32 tone recurrences): the fixture
keeps their sha256, not the samples, and the FFT outputs as sha256 plus every 64th bin -- a bit-exact pin in a few KB.

Stored:
  hann                        the 8192-entry window (float32)
  case_names                  noise (dongle scale), tone (tone plus noise), carrier (1e4 carrier over 1e-2 noise), zeros,
                              short (3 000 samples, zero-padded)
  <case>_len, <case>_x_sha256 the input's length and the sha256 of its complex64 bytes
  <case>_inr_sha256           sha256 of the windowed input (complex64, 8192)
  <case>_out_sha256           sha256 of the -O2 build's FFT output (complex64, 8192); <case>_out_every64: bins 0, 64, ...
  <case>_ofast_maxdiff        max |bin| difference of the -Ofast build's output from the -O2 one (information only)
  seq_x_sha256                of the 8 frames of 6 000 samples (tone plus noise, fresh noise per frame)
  seq_pwr / seq_smooth        after update u (u = 0..7): pwr[u::8] (8 x 1024) / smooth[u::8][:1022] (8 x 1022)
  seq_pwr_last                the whole pwr after the 8th update
  seq_maxval / seq_aveval     after each update
  provenance                  compiler versions and flags, source file and its sha256
"""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import spectrum_ref as sr  # noqa: E402

DRIVER = r"""
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>
extern "C" {
#include "kiss_fft.h"
}
// spec_driver in.bin n_frames len out.bin: in = n_frames x len cf32; out per frame: inr (8192 cf32), out (8192 cf32),
// pwr (8192 f64), smooth (8182 f64), maxval, aveval (f64); the hann table (8192 f32) first.
int main(int argc, char **argv)
{
    const int N = 8192;
    const int frames = atoi(argv[2]), len = atoi(argv[3]);
    std::vector<std::complex<float>> x((size_t)frames * len);
    FILE *fi = fopen(argv[1], "rb");
    if (fread(x.data(), sizeof(x[0]), x.size(), fi) != x.size()) return 2;
    fclose(fi);
    std::vector<float> hann(N);
    for (int i = 0; i < N; i++) hann[i] = 0.5 * (1.0 - cos(2 * M_PI * ((float)i) / (N - 1.0)));
    kiss_fft_cfg cfg = kiss_fft_alloc(N, 0, NULL, NULL);
    std::vector<std::complex<float>> inr(N), out(N);
    std::vector<kiss_fft_cpx> kin(N), kout(N);
    std::vector<double> pwr(N, 0.0), smooth(N - 10);
    FILE *fo = fopen(argv[4], "wb");
    fwrite(hann.data(), sizeof(float), N, fo);
    for (int f = 0; f < frames; f++) {
        const std::complex<float> *d = x.data() + (size_t)f * len;
        for (int a = 0; a < N; a++) inr[a] = a < len ? d[a] * hann[a] : std::complex<float>(0, 0);
        for (int i = 0; i < N; i++) { kin[i].r = inr[i].real(); kin[i].i = inr[i].imag(); }
        kiss_fft(cfg, kin.data(), kout.data());
        for (int i = 0; i < N; i++) out[i] = std::complex<float>(kout[i].r, kout[i].i);
        double maxval = 0, aveval = 0;
        for (int i = 0; i < N; i++) {
            int b = i + N / 2;
            if (b >= N) b -= N;
            const float s = out[i].imag() * out[i].imag() + out[i].real() * out[i].real();
            const double val = std::sqrt(s);  // float sqrt, widened
            pwr[b] = pwr[b] * 0.95 + 0.05 * 10 * log10(fmax(100000.0 * std::fabs((1.0 / N) * val), 1));
            if (pwr[b] > maxval) maxval = pwr[b];
            aveval += pwr[b];
        }
        for (int i = 0; i < N - 10; i++) smooth[i] = (pwr[i + 4] + pwr[i + 3] + pwr[i + 2] + pwr[i + 1] + pwr[i]) / 5;
        aveval /= N;
        if ((maxval - aveval) < 10) maxval = aveval + 10.0;
        fwrite(inr.data(), sizeof(inr[0]), N, fo);
        fwrite(out.data(), sizeof(out[0]), N, fo);
        fwrite(pwr.data(), sizeof(double), N, fo);
        fwrite(smooth.data(), sizeof(double), N - 10, fo);
        fwrite(&maxval, sizeof maxval, 1, fo);
        fwrite(&aveval, sizeof aveval, 1, fo);
    }
    fclose(fo);
    free(cfg);
    return 0;
}
"""

N = 8192


def cases():
    return sr.fixture_cases()


def sequence():
    return sr.fixture_sequence()


def build(ref, tmp, opt):
    src = os.path.join(ref, "kiss_fft130", "kiss_fft.c")
    drv = os.path.join(tmp, "driver.cpp")
    open(drv, "w").write(DRIVER)
    exe = os.path.join(tmp, f"drv{opt}")
    obj = os.path.join(tmp, f"kiss{opt}.o")
    subprocess.check_call(["gcc", opt, "-c", src, "-I", os.path.dirname(src), "-o", obj])
    subprocess.check_call(["g++", opt, drv, obj, "-I", os.path.dirname(src), "-o", exe])
    return exe


def run(exe, tmp, x):
    x = np.ascontiguousarray(x, np.complex64)
    frames, length = (1, x.size) if x.ndim == 1 else x.shape
    fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    x.tofile(fi)
    subprocess.check_call([exe, fi, str(frames), str(length), fo])
    raw = open(fo, "rb").read()
    hann = np.frombuffer(raw[: 4 * N], np.float32)
    per = 8 * N + 8 * N + 8 * N + 8 * (N - 10) + 16
    out = []
    for f in range(frames):
        b = raw[4 * N + f * per: 4 * N + (f + 1) * per]
        inr = np.frombuffer(b[: 8 * N], np.complex64)
        fft = np.frombuffer(b[8 * N: 16 * N], np.complex64)
        pwr = np.frombuffer(b[16 * N: 24 * N], np.float64)
        smooth = np.frombuffer(b[24 * N: 24 * N + 8 * (N - 10)], np.float64)
        mx, av = np.frombuffer(b[24 * N + 8 * (N - 10):], np.float64)
        out.append((inr, fft, pwr, smooth, mx, av))
    return hann, out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SDRRECEIVER_REF", "")
    src = os.path.join(ref, "kiss_fft130", "kiss_fft.c")
    if not os.path.exists(src):
        sys.exit("usage: make_spectrum_golden.py /path/to/SDRReceiver (its kiss_fft130/kiss_fft.c)")
    d = {}
    with tempfile.TemporaryDirectory() as tmp:
        o2, ofast = build(ref, tmp, "-O2"), build(ref, tmp, "-Ofast")
        names = []
        for name, x in cases().items():
            hann, [(inr, out, *_)] = run(o2, tmp, x)
            _, [(_, out_fast, *_)] = run(ofast, tmp, x)
            d[f"{name}_len"], d[f"{name}_x_sha256"] = np.int64(x.size), np.array(sr.sha256(x))
            d[f"{name}_inr_sha256"], d[f"{name}_out_sha256"] = np.array(sr.sha256(inr)), np.array(sr.sha256(out))
            d[f"{name}_out_every64"] = out[::64].copy()
            d[f"{name}_ofast_maxdiff"] = np.float64(np.abs(out.astype(np.complex128) - out_fast).max())
            d["hann"] = hann
            names.append(name)
            same = np.array_equal(out.view(np.uint32), out_fast.view(np.uint32))
            print(f"{name}: {x.size} samples, -Ofast bins {'identical' if same else 'differ'} "
                  f"(max {d[f'{name}_ofast_maxdiff']:.3g}, max |bin| {np.abs(out).max():.3g})")
        d["case_names"] = np.array(names)
        seq = sequence()
        _, res = run(o2, tmp, seq)
        d["seq_x_sha256"] = np.array(sr.sha256(seq))
        d["seq_pwr"] = np.stack([r[2][u::8] for u, r in enumerate(res)])
        d["seq_smooth"] = np.stack([r[3][u::8][:1022] for u, r in enumerate(res)])
        d["seq_pwr_last"] = res[-1][2].copy()
        d["seq_maxval"] = np.array([r[4] for r in res])
        d["seq_aveval"] = np.array([r[5] for r in res])
    gcc = subprocess.check_output(["gcc", "--version"], text=True).splitlines()[0]
    d["provenance"] = np.array(f"kiss_fft130/kiss_fft.c sha256 {hashlib.sha256(open(src, 'rb').read()).hexdigest()}, "
                               f"unmodified, gcc -O2 (and -Ofast for *_ofast_maxdiff), {gcc}; power step: C++ restatement, "
                               f"glibc log10; generated by tests/golden/make_spectrum_golden.py")
    path = os.path.join(HERE, "spectrum.npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
