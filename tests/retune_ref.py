"""numpy restatement of ONE VFO node's chain for the retune tests, frame by frame, with retunes and gain changes between frames.

A retune of a node to `f` before frame K is the reference's own primitive at that point, `delete osc_mix; osc_mix = new
Oscillator(Fs, f)`: the oscillator starts again (sample 0 of frame K takes the new table's entry L-1, then entries 1, 2, ...:
oscillator.cpp:20-50) and every filter state is carried over.  A gain change is vfo::setGain between two vfo::process calls.
The liborc oracle cannot express either (its oscillator is built once, in init), hence this model.  Every step is float32
in the order the reference evaluates it (numpy's float32 ufuncs round every operation and never fuse a multiply-add); the
FIRs vectorise over their outputs with one pass per tap, so the running sum per output keeps the reference's order:

* :func:`mix` -- the table mixer, x = (a c - b d, a d + b c) (vfo.cpp:237-245).  The table is the oracle's orc_osc_table (the
  recurrence is a serial chain of Fs steps; it is pinned to the reference by tests/test_oracle_vs_reference.py).
* :func:`halfband` -- one 11-tap half-band /2 stage over [11 history | frame], symmetric pairs left to right, then `0 + s`;
  the history kept is the 11 samples ending one before the frame's last (halfbanddecimator.cpp:43-72, dsp.cpp:137-173).
* late /5 | /6 (vfo.cpp:334-387): every sample enters the decimating low-pass, the frame-local samples 0, L, 2L, ... give an
  output over the N samples before the newest (the (N+1)-slot ring, dsp.cpp:59-71).
* the demodulation (vfo.cpp:300-332): 62-sample delay minus the 125-tap Hilbert (newest included, float sum, as double),
  rounded to float; the audio low-pass (newest excluded); `short(usb*gain*32768.0)` with x86-64's cvttsd2si.
* :func:`compress` -- vfo.cpp:389-424.
"""
from __future__ import annotations

import numpy as np

from oracle import binding as ob

HB0 = np.float32(0.0060431029837374152)
HB2 = np.float32(-0.049372515458761493)
HB4 = np.float32(0.29332944952052842)
HB5 = np.float32(0.5)
HILBERT = 125
DELAY = 62

_tables: dict[tuple[int, float], np.ndarray] = {}


def table(fs: int, f: float) -> np.ndarray:
    key = (int(fs), float(f))
    if key not in _tables:
        _tables[key] = ob.osc_table("port", int(fs), float(f))
    return _tables[key]


def mix(tab: np.ndarray, k0: int, x: np.ndarray) -> np.ndarray:
    """Samples k0 .. k0 + n of an oscillator that started at k = 0 times x (complex64)."""
    L = tab.size
    k = np.arange(k0, k0 + x.size, dtype=np.int64)
    idx = np.where(k == 0, L - 1, k % L)
    t = tab[idx]
    a, b = t.real, t.imag
    c, d = x.real, x.imag
    out = np.empty(x.size, np.complex64)
    out.real = a * c - b * d
    out.imag = a * d + b * c
    return out


def halfband(hist: np.ndarray, x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """One stage on a complex frame; hist = the 11 queue entries in front of it.  Returns (output, next hist)."""
    q = np.concatenate([hist, x])
    n = x.size
    out = np.empty(n // 2, np.complex64)
    for comp in ("real", "imag"):
        c = getattr(q, comp)
        w = [c[1 + j: 1 + j + n: 2][: n // 2] for j in range(11)]
        s = HB0 * (w[0] + w[10]) + HB2 * (w[2] + w[8]) + HB4 * (w[4] + w[6]) + HB5 * w[5]
        setattr(out, comp, np.float32(0) + s)
    return out, q[n - 1: n - 1 + 11].copy()


def fir_excl(taps: np.ndarray, hist: np.ndarray, x: np.ndarray, at=None) -> tuple[np.ndarray, np.ndarray]:
    """jonti FIR::FIRUpdateAndProcess: after pushing x[t] the sum runs over the N samples before it, oldest first.
    `at`: only these positions of x give an output (every sample is pushed).  Returns (outputs, next hist)."""
    N = taps.size
    X = np.concatenate([hist, x])
    pos = np.arange(x.size) if at is None else at
    acc = np.zeros(pos.size, np.float32)
    for j in range(N):
        acc = acc + taps[j] * X[pos + j]
    return acc, X[X.size - N:].copy()


def to_short(pre: np.ndarray) -> np.ndarray:
    """`short = double` on x86-64: cvttsd2si (out of range / NaN -> INT32_MIN), low 16 bits."""
    bad = ~(np.abs(pre) < 2147483648.0) & ~(pre == -2147483648.0)
    t = np.where(bad, -2147483648.0, np.trunc(np.where(bad, 0.0, pre))).astype(np.int64)
    return (t & 0xFFFF).astype(np.uint16).view(np.int16)


def to_schar(f: np.ndarray) -> np.ndarray:
    bad = ~(np.abs(f) < np.float32(2147483648.0)) & ~(f == np.float32(-2147483648.0))
    t = np.where(bad, -2147483648.0, np.trunc(np.where(bad, 0.0, f.astype(np.float64)))).astype(np.int64)
    return (t & 0xFF).astype(np.uint8).view(np.int8)


def compress(z: np.ndarray, cstyle: int, scalecomp: int) -> np.ndarray:
    if cstyle == 1:
        re = to_schar((z.real / np.float32(scalecomp)) * np.float32(128)).astype(np.int32)
        im = to_schar((z.imag / np.float32(scalecomp)) * np.float32(128)).astype(np.int32)
        return (((re & 0xF0) | ((im & 0xF0) >> 4)) & 0xFF).astype(np.uint8).view(np.int8)
    out = np.empty(2 * z.size, np.int8)
    out[0::2] = to_schar(z.real * np.float32(128))
    out[1::2] = to_schar(z.imag * np.float32(128))
    return out


class Node:
    """One VFO node (a topology.VfoDesc) fed frame by frame."""

    def __init__(self, desc):
        self.d = desc
        self.fs, self.dc = int(desc.fs), int(desc.decimate_count)
        self.tab = table(self.fs, desc.mixer_freq)
        self.k = 0  # samples since the oscillator started
        self.gain = np.float32(desc.gain)
        self.hb = [np.zeros(11, np.complex64) for _ in range(self.dc)]
        self.late = int(desc.late_decimate) if desc.demod_usb else 0
        out_rate = self.fs // 2 ** self.dc
        if self.late:
            out_rate //= self.late
            self.dec = ob.low_pass("port", 2, out_rate * self.late, out_rate // 2, out_rate / (self.late - 1))
            self.dec_hist = np.zeros(self.dec.size, np.complex64)
        n_out = desc.samples_per_buffer // 2 ** self.dc // (self.late or 1)
        self.lpf = ob.low_pass("port", 2, out_rate, desc.filter_bw, desc.filter_bw / 4) if desc.demod_usb and desc.filter_bw > 0 \
            else None
        if self.lpf is not None:
            self.lpf_hist = np.zeros(self.lpf.size, np.float32)
        self.hilbert = ob.hilbert_taps("port", HILBERT, n_out)  # vfo.cpp:137: "Fs" = samplesOut
        self.delay_hist = np.zeros(DELAY, np.float32)
        self.hil_hist = np.zeros(HILBERT - 1, np.float32)
        self.stream = None

    def retune(self, f: float) -> None:
        self.tab = table(self.fs, f)
        self.k = 0

    def set_gain(self, g: float) -> None:
        self.gain = np.float32(g)

    def process(self, x: np.ndarray):
        """One frame of input (complex64).  Returns the payload (int16 audio or int8 IQ; None for a node with children:
        call it on a leaf's description) and keeps decimate[d] in self.stream."""
        z = mix(self.tab, self.k, np.asarray(x, np.complex64))
        self.k += z.size
        for s in range(self.dc):
            z, self.hb[s] = halfband(self.hb[s], z)
        self.stream = z
        return z

    def payload(self) -> np.ndarray:
        z = self.stream
        if not self.d.demod_usb:
            return compress(z, self.d.cstyle, self.d.scalecomp)
        if self.late:
            at = np.arange(0, z.size, self.late)
            fr, h = fir_excl(self.dec, self.dec_hist.real.copy(), z.real, at)
            fi, hq = fir_excl(self.dec, self.dec_hist.imag.copy(), z.imag, at)
            self.dec_hist = (h + 1j * hq).astype(np.complex64)
        else:
            fr, fi = z.real.copy(), z.imag.copy()
        D = np.concatenate([self.delay_hist, fr])
        delayed = D[: fr.size]
        self.delay_hist = D[D.size - DELAY:].copy()
        H = np.concatenate([self.hil_hist, fi])
        acc = np.zeros(fi.size, np.float32)
        for i in range(HILBERT):
            acc = acc + self.hilbert[i] * H[i: i + fi.size]
        self.hil_hist = H[H.size - (HILBERT - 1):].copy()
        usb = (delayed.astype(np.float64) - acc.astype(np.float64)).astype(np.float32)
        if self.lpf is not None:
            usb, self.lpf_hist = fir_excl(self.lpf, self.lpf_hist, usb)
        pre = (usb * self.gain).astype(np.float64) * 32768.0
        self.pre = pre  # (float32 * 2^15: exact as float32 too -- what the meters' `clipped` and `peak` are defined on)
        return to_short(pre)


def run(desc, frames, retunes=(), gains=()):
    """`frames`: the node's input per frame.  retunes / gains: (frame, value) pairs applied before that frame.  Returns the
    list of (stream, payload) per frame."""
    node = Node(desc)
    rt, gn = dict(retunes), dict(gains)
    out = []
    for f, x in enumerate(frames):
        if f in rt:
            node.retune(rt[f])
        if f in gn:
            node.set_gain(gn[f])
        z = node.process(x)
        out.append((z, node.payload()))
    return out
