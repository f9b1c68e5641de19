"""The rational resampler L/M in front of level 0 (include/sdrx.h "Resampler") as a numpy model.

A tree can only halve, and end in /5 or /6; a front end with a fixed master clock (Airspy at 10, 6, 3 or 2.5 MS/s, an RTL
dongle at 2.4 or 2.048 MS/s) delivers another rate.  With ``Receiver(input_rate=...)`` the frames are at that rate and one
more kernel makes the tree's raw frame from them.  The reference has no counterpart: the header's text is the definition and
this module is the yardstick -- :func:`ratio` and :func:`frames` for the lengths, :func:`design` for the built-in Kaiser
prototype, :func:`apply` for the arithmetic, bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

MAX_L, MIN_T, MAX_T, MAX_TAPS = 1024, 8, 64, 32768


def ratio(fs_in: int, fs_out: int) -> tuple[int, int]:
    """``(L, M)``: L = fs_out / g, M = fs_in / g with g = gcd(fs_in, fs_out)."""
    fs_in, fs_out = int(fs_in), int(fs_out)
    if fs_in <= 0 or fs_out <= 0:
        raise ValueError("sample rates must be positive")
    g = math.gcd(fs_in, fs_out)
    return fs_out // g, fs_in // g


def refusal(fs_in: int, fs_out: int, taps_per_phase: int, out_frame: int | None = None) -> str | None:
    """Why the library refuses this ratio (with `out_frame`: and this frame length) with SDRX_EUNSUPPORTED; None: it is offered."""
    L, M = ratio(fs_in, fs_out)
    T = int(taps_per_phase)
    if L > MAX_L:
        return "L exceeds 1024"
    if 2 * M < L or M > 4 * L:
        return "M / L outside 1/2 .. 4"
    if T < MIN_T or T > MAX_T or T % 4:
        return "taps_per_phase must be a multiple of 4 in 8 .. 64"
    if L * T > MAX_TAPS:
        return "L * taps_per_phase exceeds 32768"
    if out_frame is not None:
        n = int(out_frame)
        if n <= 0 or n * M % L:
            return "n * M is not a multiple of L"
        if n * M // L % 16:
            return "the input frame is not a multiple of 16"
        if n * M // L < T:
            return "the input frame is shorter than taps_per_phase"
    return None


def in_frame(fs_in: int, fs_out: int, out_frame: int) -> int:
    """n_in = n M / L (ValueError if that is no whole number)."""
    L, M = ratio(fs_in, fs_out)
    if out_frame * M % L:
        raise ValueError(f"{out_frame} * {M} is not a multiple of {L}")
    return out_frame * M // L


def frames(fs_in: int, fs_out: int, seconds: float, multiple_of: int = 16) -> tuple[int, int]:
    """The valid ``(in_frame, out_frame)`` nearest to `seconds` of signal whose out_frame is a multiple of `multiple_of`:
    out_frame = k L and in_frame = k M, k a multiple of what makes in_frame a multiple of 16 and out_frame one of `multiple_of`;
    a tie goes to the shorter frame."""
    L, M = ratio(fs_in, fs_out)
    k16 = 16 // math.gcd(16, M)
    kmo = int(multiple_of) // math.gcd(int(multiple_of), L)
    step = k16 // math.gcd(k16, kmo) * kmo
    q = float(seconds) * fs_out / (step * L)
    j = math.floor(q)
    if q - j > 0.5:
        j += 1
    k = max(j, 1) * step
    return k * M, k * L


def design(fs_in: int, fs_out: int, taps_per_phase: int, atten_db: float = 80.0) -> tuple[np.ndarray, dict]:
    """The built-in prototype (float32, L T taps) and its info: IEEE double, rounded once.  With N = L T and A = atten_db:
    beta = 0.1102 (A - 8.7), tw = (A - 7.95) / (2.285 (N - 1) 2 pi), fn = 0.5 / max(L, M), fc = fn - tw / 2,
    h[k] = L 2 fc sinc(2 fc (k - (N-1)/2)) I0(beta sqrt(1 - (2k/(N-1) - 1)^2)) / I0(beta).  ValueError where the library returns
    SDRX_EFILTER (fn - tw <= 0) or refuses the ratio."""
    why = refusal(fs_in, fs_out, taps_per_phase)
    if why:
        raise ValueError(why)
    if not 50.0 < atten_db <= 120.0:
        raise ValueError("atten_db must be above 50 and at most 120")
    L, M = ratio(fs_in, fs_out)
    T = int(taps_per_phase)
    N = L * T
    beta = 0.1102 * (atten_db - 8.7)
    tw = (atten_db - 7.95) / (2.285 * (N - 1) * 2 * math.pi)
    fn = 0.5 / max(L, M)
    if fn - tw <= 0:
        raise ValueError("the transition is wider than the band")
    fc = fn - tw / 2
    k = np.arange(N, dtype=np.float64)
    r = 2.0 * k / (N - 1) - 1.0
    win = np.i0(beta * np.sqrt(np.maximum(1.0 - r * r, 0.0))) / np.i0(beta)
    h = L * 2 * fc * np.sinc(2 * fc * (k - (N - 1) / 2.0)) * win
    info = {"fs_in": int(fs_in), "fs_out": int(fs_out), "L": L, "M": M, "taps_per_phase": T, "in_frame": 0, "out_frame": 0,
            "delay_out_samples": (N - 1) / (2.0 * M), "passband_hz": (fn - tw) * L * float(fs_in)}
    return h.astype(np.float32), info


def positions(n_out: int, L: int, M: int) -> tuple[np.ndarray, np.ndarray]:
    """``(i, ph)`` of the outputs 0 .. n_out-1: p = m M in 64 bits, i = p div L, ph = p mod L."""
    p = np.arange(int(n_out), dtype=np.int64) * np.int64(M)
    return p // L, p % L


def apply(x, taps, L: int, M: int, history=None) -> tuple[np.ndarray, np.ndarray]:
    """One frame through the resampler: ``(y, history')``.  `x`: the frame at the input rate (complex64, n_in samples, n_in M'
    = n L with the ratio reduced); `taps`: the prototype h (float32, L T); `history`: the last T-1 samples of the previous
    frame (None: zeros -- the first frame after finalize).  Per component and output m, with (i, ph) = :func:`positions`:
    acc = +0.0f; acc = fl(acc + fl(h[ph + t L] * x[i - t])) for t = 0 .. T-1 ascending; y[m] = acc."""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    h = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    T = h.size // L
    if h.size != L * T or x.size * L % M:
        raise ValueError("taps must hold L * T floats and the frame n_in with n_in * L a multiple of M")
    n_out = x.size * L // M
    hist = np.zeros(T - 1, np.complex64) if history is None else np.ascontiguousarray(history, dtype=np.complex64).reshape(-1)
    if hist.size != T - 1:
        raise ValueError(f"the history has T - 1 = {T - 1} samples")
    ext = np.concatenate([hist, x])  # ext[T - 1 + j] = x[j]
    i, ph = positions(n_out, L, M)
    re, im = ext.real.astype(np.float32), ext.imag.astype(np.float32)
    acc_re, acc_im = np.zeros(n_out, np.float32), np.zeros(n_out, np.float32)
    for t in range(T):
        c = h[ph + t * L]
        j = i - t + (T - 1)
        acc_re = acc_re + c * re[j]  # float32 arrays throughout: a product rounded, then a sum rounded
        acc_im = acc_im + c * im[j]
    y = np.empty(n_out, np.complex64)
    y.real, y.imag = acc_re, acc_im
    return y, ext[ext.size - (T - 1):].copy()


def info_dict(r) -> dict:
    """One ``sdrx_resampler_info`` as a dict."""
    return {"fs_in": int(r.fs_in), "fs_out": int(r.fs_out), "L": int(r.L), "M": int(r.M), "taps_per_phase": int(r.taps_per_phase),
            "in_frame": int(r.in_frame), "out_frame": int(r.out_frame), "delay_out_samples": float(r.delay_out_samples),
            "passband_hz": float(r.passband_hz)}
