"""Post-detection filter of the detector leaves (``sdrx_set_postfilter``): the numpy model, the Kaiser design and the levels.

A detector leaf (sdrreceiver_amd.detect) can be given a real FIR of the caller's taps ``h[t]``, ``t < T``, over the
detector's pre-quantisation floats ``pre``, decimated by an integer ``R``.  include/sdrx.h "Post-detection filter" is the
definition and csrc/sdrx_postdet.h its per-output form; this module restates both one float32 operation at a time, and the
tests hold the device to it bit for bit.  There is no counterpart in the reference.

For output ``m`` in ``[0, n / R)``::

    acc = +0.0f;  acc = fl(acc + fl(h[t] * pre[m R - t]))  for t = 0 .. T-1 ascending;  y[m] = acc

``pre[j]`` for ``j < 0`` is the frame before's ``pre[n + j]`` -- with the carrier and the gain THAT frame had -- and ``+0.0f``
for a leaf that starts as a new vfo (:class:`State`).  The payload is the USB leaves' int16 conversion of ``y``, the output
meter is the USB leaves' over those ``n / R`` values.  ``T = 1, h = [1.0], R = 1`` is the identity.

Limits: ``1 <= T <= 256``, ``1 <= R <= 16``, ``n % R == 0``.  Not offered: IIR de-emphasis, a DC block for FM, changing taps on
a running tree, groups, the AGC.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import detect, meter

MAX_TAPS, MAX_DECIM = 256, 16
_f32 = np.float32


def refusal(ntaps: int, decim: int, n: int | None = None) -> str | None:
    """Why the library refuses these settings (SDRX_EINVAL; with `n`, the leaf's stream samples per frame: SDRX_EUNSUPPORTED at
    finalize); None: they are offered."""
    if not 1 <= int(ntaps) <= MAX_TAPS:
        return "ntaps must be 1 .. 256"
    if not 1 <= int(decim) <= MAX_DECIM:
        return "decim must be 1 .. 16"
    if n is not None and int(n) % int(decim):
        return "the leaf's samples per frame are not a multiple of decim"
    return None


def design(fs: float, cutoff_hz: float, ntaps: int, atten_db: float = 80.0) -> tuple[np.ndarray, dict]:
    """``sdrx_postfilter_design``: a Kaiser low-pass in IEEE double, rounded once to float32, and its info.  With N = ntaps and
    A = atten_db: beta = 0.1102 (A - 8.7), tw = (A - 7.95) / (2.285 (N - 1) 2 pi), fc = cutoff_hz / fs,
    h[k] = 2 fc sinc(2 fc (k - (N-1)/2)) I0(beta sqrt(1 - (2k/(N-1) - 1)^2)) / I0(beta), divided by the sum of the h[k] (k
    ascending): unit DC gain.  ValueError where the library returns SDRX_EINVAL or SDRX_EFILTER."""
    N = int(ntaps)
    if not 50.0 < atten_db <= 120.0:
        raise ValueError("atten_db must be above 50 and at most 120")
    if not 1 <= N <= MAX_TAPS or not fs > 0 or not cutoff_hz > 0:
        raise ValueError("ntaps must be 1 .. 256, fs and cutoff_hz positive")
    if N == 1:
        raise ValueError("the transition does not fit")
    from .front import _i0  # the power series the library sums, term by term
    pi = 3.141592653589793238462643383279502884
    fs, atten_db = float(fs), float(atten_db)
    beta = 0.1102 * (atten_db - 8.7)
    tw = (atten_db - 7.95) / (2.285 * (N - 1) * 2 * pi)
    fc = float(cutoff_hz) / fs
    if not fc - tw / 2 > 0 or not fc + tw / 2 <= 0.5:
        raise ValueError("the transition does not fit")
    i0b, mid = _i0(beta), (N - 1) / 2.0
    h = np.zeros(N, np.float64)
    total = 0.0
    for k in range(N):  # IEEE double, operation for operation the library's
        x = 2 * fc * (k - mid)
        sinc = 1.0 if x == 0 else math.sin(pi * x) / (pi * x)
        r = 2.0 * k / (N - 1) - 1
        arg = 1 - r * r
        win = _i0(beta * math.sqrt(arg if arg > 0 else 0.0)) / i0b
        h[k] = 2 * fc * sinc * win
        total += h[k]
    info = {"decim": 0, "ntaps": N, "out_len": 0, "delay_samples": (N - 1) / 2.0, "pass_hz": (fc - tw / 2) * fs,
            "stop_hz": (fc + tw / 2) * fs}
    return (h / total).astype(np.float32), info


def levels(desc, ntaps: int | None = None, decim: int | None = None) -> dict:
    """Rate, length and delay of a detector leaf `desc` (a VfoDesc) with its post-detection filter (or the one given)."""
    T = len(desc.post_taps) if ntaps is None else int(ntaps)
    R = (desc.post_decim if T else 1) if decim is None else int(decim)
    n = desc.n_stage_out
    if T and n % R:
        raise ValueError(f"{n} samples per frame are not a multiple of decim {R}")
    rate = desc.out_rate_stage // R
    delay = (T - 1) / 2.0 if T else 0.0
    return {"rate": rate, "out_len": n // R, "bytes": 2 * (n // R), "delay_samples": delay, "delay_s": delay / desc.out_rate_stage}


@dataclasses.dataclass
class State:
    """What a filtered detector leaf carries from frame to frame: the detector's (``z[-1]``, FM) and the last ``T - 1`` values of
    ``pre``.  A fresh one is a leaf that starts as a new vfo."""
    det: detect.State = dataclasses.field(default_factory=detect.State)
    hist: np.ndarray | None = None  # None: zeros


def fir(pre, taps, decim: int, hist=None) -> tuple[np.ndarray, np.ndarray]:
    """``(y, hist')``: one frame of `pre` (float32, n values, n % R == 0) through the filter; `hist` = the T - 1 values before
    it (None: zeros)."""
    pre = np.ascontiguousarray(pre, dtype=_f32).reshape(-1)
    h = np.ascontiguousarray(taps, dtype=_f32).reshape(-1)
    T, R = h.size, int(decim)
    why = refusal(T, R, pre.size)
    if why:
        raise ValueError(why)
    old = np.zeros(T - 1, _f32) if hist is None else np.ascontiguousarray(hist, dtype=_f32).reshape(-1)
    if old.size != T - 1:
        raise ValueError(f"the history has T - 1 = {T - 1} values")
    ext = np.concatenate([old, pre])  # ext[T - 1 + i] = pre[i]
    at = np.arange(pre.size // R, dtype=np.int64) * R + (T - 1)
    acc = np.zeros(at.size, _f32)
    with np.errstate(all="ignore"):
        for t in range(T):
            acc = acc + h[t] * ext[at - t]  # float32 arrays throughout: a product rounded, then a sum rounded
    return acc, ext[ext.size - (T - 1):].copy()


def pre_of(kind: int, z, gain, det_state: detect.State | None = None) -> np.ndarray:
    """The detector's pre-quantisation floats of one frame, advancing the detector's state"""
    z = np.ascontiguousarray(np.asarray(z, np.complex64).reshape(-1))
    if kind == detect.AM:
        pre = detect.am_pre(z, gain)
    elif kind == detect.FM:
        pre = detect.fm_pre(z, gain, det_state.z_prev if det_state is not None else 0j)
    else:
        raise ValueError(f"detector kind {kind}")
    if det_state is not None and z.size:
        det_state.z_prev = complex(z[-1])
    return pre


def run(kind: int, z, gain, taps, decim: int, state: State | None = None) -> dict:
    """One frame of a filtered detector leaf: ``payload`` (int16, n / R values) and its output meter (``n_values``, ``sum_sq``,
    ``clipped``, ``peak``), advancing `state`."""
    pre = pre_of(kind, z, gain, state.det if state is not None else None)
    y, hist = fir(pre, taps, decim, state.hist if state is not None else None)
    if state is not None:
        state.hist = hist
    pay, scaled = detect.quantise(y)
    out = meter.meters_from_payload(detect._UsbLike, pay, scaled)
    out["payload"] = pay
    out["y"] = y
    return out


def info_dict(r) -> dict:
    """One ``sdrx_postfilter_info`` as a dict."""
    return {"decim": int(r.decim), "ntaps": int(r.ntaps), "out_len": int(r.out_len), "delay_samples": float(r.delay_samples),
            "pass_hz": float(r.pass_hz), "stop_hz": float(r.stop_hz)}
