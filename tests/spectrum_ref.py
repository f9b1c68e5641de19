"""numpy restatement of the spectrum display (MainWindow::fftHandlerSlot, mainwindow.cpp:411-478) for the tests.

* :func:`hann`, :func:`twiddles` -- the reference's double expressions (glibc cos / sin through ``math``), stored as float32.
* :func:`kiss_fft` -- kf_work's recursion for nfft = 8192 (radices 4,4,4,4,4,4,2): the input in the digit-reversed order the
  recursion leaves it in, then kf_bfly2 and six kf_bfly4 stages, every butterfly of a stage at once as vectorised float32
  operations in kiss_fft's own order (C_MUL as 4 multiplies, no fused multiply-add anywhere in numpy's float32 ufuncs).
* :class:`Display` -- steps 3-4 in float64: the IIR on pwr, maxval / aveval and the "< 10 dB" rule, smooth.
* :func:`raw_update_calls` -- sdrj's every-4th-call cadence (sdrj.cpp:84-101, 296-303).
"""
from __future__ import annotations

import math

import numpy as np

N = 8192


def hann(n: int = N) -> np.ndarray:
    """hann[i] = 0.5*(1.0-cos(2*M_PI*((float)i)/(nFFT-1.0))), double, stored as float (mainwindow.cpp:284-287)."""
    return np.array([0.5 * (1.0 - math.cos(2 * math.pi * float(np.float32(i)) / (n - 1.0))) for i in range(n)], np.float32)


def twiddles(n: int = N) -> np.ndarray:
    """kiss_fft_alloc's forward twiddles: phase = -2*pi*i / nfft in double, (float)cos, (float)sin."""
    pi = 3.141592653589793238462643383279502884197169399375105820974944
    out = np.empty(n, np.complex64)
    for i in range(n):
        ph = -2 * pi * i / n
        out[i] = np.complex64(complex(np.float32(math.cos(ph)), np.float32(math.sin(ph))))
    return out


def digit_reversed_positions(n: int = N) -> np.ndarray:
    """pos[a]: where kf_work's recursion stores input a before the first butterfly (factors 4,4,4,4,4,4,2)."""
    a = np.arange(n)
    pos = np.zeros(n, np.int64)
    rest = a.copy()
    for k in range(6):
        pos += (rest & 3) << (2 * (5 - k) + 1)
        rest >>= 2
    return pos + rest


_TW = None
_POS = None
_HANN = None


def _cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def kiss_fft(x: np.ndarray) -> np.ndarray:
    """Forward kiss_fft of 8192 complex64 values, bit for bit."""
    global _TW, _POS
    if _TW is None:
        _TW = twiddles()
        _POS = digit_reversed_positions()
    x = np.asarray(x, np.complex64)
    assert x.shape == (N,)
    F = np.empty(N, np.complex64)
    F[_POS] = x
    re = F.real.astype(np.float32).copy()
    im = F.imag.astype(np.float32).copy()
    twr = _TW.real.astype(np.float32)
    twi = _TW.imag.astype(np.float32)
    # kf_bfly2, m = 1: t = Fout2 * tw[0]; Fout2 = Fout - t; Fout += t
    r0, i0, r1, i1 = re[0::2].copy(), im[0::2].copy(), re[1::2].copy(), im[1::2].copy()
    tr, ti = _cmul(r1, i1, twr[0], twi[0])
    re[1::2], im[1::2] = r0 - tr, i0 - ti
    re[0::2], im[0::2] = r0 + tr, i0 + ti
    m = 2
    while m < N:
        fs = N // (4 * m)
        blocks = N // (4 * m)
        R = re.reshape(blocks, 4, m)
        I = im.reshape(blocks, 4, m)
        k = np.arange(m)
        w1r, w1i = twr[k * fs], twi[k * fs]
        w2r, w2i = twr[2 * k * fs], twi[2 * k * fs]
        w3r, w3i = twr[3 * k * fs], twi[3 * k * fs]
        f0r, f0i = R[:, 0].copy(), I[:, 0].copy()
        s0r, s0i = _cmul(R[:, 1], I[:, 1], w1r, w1i)
        s1r, s1i = _cmul(R[:, 2], I[:, 2], w2r, w2i)
        s2r, s2i = _cmul(R[:, 3], I[:, 3], w3r, w3i)
        s5r, s5i = f0r - s1r, f0i - s1i
        f0r, f0i = f0r + s1r, f0i + s1i
        s3r, s3i = s0r + s2r, s0i + s2i
        s4r, s4i = s0r - s2r, s0i - s2i
        R[:, 2], I[:, 2] = f0r - s3r, f0i - s3i
        R[:, 0], I[:, 0] = f0r + s3r, f0i + s3i
        R[:, 1], I[:, 1] = s5r + s4i, s5i - s4r
        R[:, 3], I[:, 3] = s5r - s4i, s5i + s4r
        m *= 4
    out = np.empty(N, np.complex64)
    out.real, out.imag = re, im
    return out


def windowed(x: np.ndarray) -> np.ndarray:
    """inr: the first min(len, 8192) samples times the window (complex<float> * float), zero-padded."""
    x = np.asarray(x, np.complex64).reshape(-1)
    global _HANN
    if _HANN is None:
        _HANN = hann()
    n = min(x.size, N)
    h = _HANN
    out = np.zeros(N, np.complex64)
    out.real[:n] = x.real[:n] * h[:n]
    out.imag[:n] = x.imag[:n] * h[:n]
    return out


class Display:
    """One display state: pwr starts zeroed (on_comboVFO_currentIndexChanged), updated by :meth:`update`."""

    def __init__(self):
        self.pwr = np.zeros(N, np.float64)
        self.maxval = 0.0
        self.aveval = 0.0
        self.updates = 0
        self.bins = np.zeros(N, np.complex64)

    def update(self, x: np.ndarray) -> None:
        out = kiss_fft(windowed(x))
        self.update_bins(out)

    def update_bins(self, out: np.ndarray) -> None:
        self.bins = out
        re, im = out.real.astype(np.float32), out.imag.astype(np.float32)
        val = np.sqrt(im * im + re * re).astype(np.float64)  # float sum, float sqrt, widened
        lvl = 0.05 * 10 * np.log10(np.fmax(100000.0 * np.abs((1.0 / N) * val), 1))
        b = (np.arange(N) + N // 2) % N
        self.pwr[b] = self.pwr[b] * 0.95 + lvl
        order = self.pwr[b]  # the reference's visiting order b = N/2 .. N-1, 0 .. N/2-1
        mx = 0.0
        m = float(order.max())
        if m > mx:
            mx = m
        ave = math.fsum(order) / N
        if mx - ave < 10:
            mx = ave + 10.0
        self.maxval, self.aveval = mx, ave
        self.updates += 1

    @property
    def smooth(self) -> np.ndarray:
        p = self.pwr
        k = N - 10
        return (p[4:k + 4] + p[3:k + 3] + p[2:k + 2] + p[1:k + 1] + p[:k]) / 5


def raw_update_calls(frames: int) -> list[int]:
    """1-based frame calls after enabling on which sdrj emits fftData: count = 0 on selection, then per frame
    ``if (count == 4) {emit; count = 0;} count++``."""
    count, calls = 0, []
    for call in range(1, frames + 1):
        if count == 4:
            calls.append(call)
            count = 0
        count += 1
    return calls


def lcg_complex(seed: int, n: int, scale: float) -> np.ndarray:
    """Seeded integer LCG (Knuth's MMIX constants): n complex64 samples uniform in [-scale, scale)."""
    state = np.uint64(seed)
    a, c = np.uint64(6364136223846793005), np.uint64(1442695040888963407)
    out = np.empty(2 * n, np.float64)
    with np.errstate(over="ignore"):
        seq = np.empty(2 * n, np.uint64)
        for i in range(2 * n):
            state = state * a + c
            seq[i] = state
    out = (seq >> np.uint64(40)).astype(np.float64) / float(1 << 24)  # [0, 1)
    v = ((out * 2 - 1) * scale).astype(np.float32)
    return v.view(np.complex64)


def tone(n: int, cos_w: float, sin_w: float, amp: float) -> np.ndarray:
    """amp * w^k, k < n, as a float32 recurrence z <- z * w with every product and sum rounded on its own (C_MUL's form):
    reproducible bit for bit on any IEEE machine, unlike a library exp / cos.  w is given as two float32 literals."""
    wr, wi = np.float32(cos_w), np.float32(sin_w)
    zr, zi = np.float32(amp), np.float32(0.0)
    out = np.empty(2 * n, np.float32)
    for k in range(n):
        out[2 * k], out[2 * k + 1] = zr, zi
        zr, zi = np.float32(np.float32(zr * wr) - np.float32(zi * wi)), np.float32(np.float32(zr * wi) + np.float32(zi * wr))
    return out.view(np.complex64)


def add32(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """complex64 a + b, component by component in float32."""
    out = np.empty(a.size, np.complex64)
    out.real = a.real.astype(np.float32) + b.real.astype(np.float32)
    out.imag = a.imag.astype(np.float32) + b.imag.astype(np.float32)
    return out


def fixture_cases() -> dict:
    """The inputs of tests/golden/spectrum.npz, regenerated (their sha256 is stored there): dongle-scale noise, a tone plus
    noise, a 1e4 carrier over 1e-2 noise, all zeros, and 3 000 samples (zero-padded by the window step)."""
    return {
        "noise": lcg_complex(11, N, 127.5),
        "tone": add32(tone(N, 0.7139301300048828, 0.7002169489860535, 50.0), lcg_complex(12, N, 4.0)),
        "carrier": add32(tone(N, -0.30901700258255005, -0.9510565400123596, 1e4), lcg_complex(13, N, 1e-2)),
        "zeros": np.zeros(N, np.complex64),
        "short": lcg_complex(14, 3000, 127.5),
    }


def fixture_sequence() -> np.ndarray:
    """The 8 frames of 6 000 samples of the fixture's power sequence: a tone plus fresh noise per frame."""
    t = tone(6000, 0.9510565400123596, 0.30901700258255005, 30.0)
    return np.stack([add32(t, lcg_complex(100 + f, 6000, 8.0)) for f in range(8)])


def sha256(a: np.ndarray) -> str:
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
