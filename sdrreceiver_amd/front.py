"""The half-band front stage in front of the resampler or level 0 (include/sdrx.h "Front stage") as a numpy model.

A front end that delivers real samples of an IF (Airspy R2 / Mini), or one whose rate is more than four times the tree's, gets
1 .. 3 half-band decimations by 2 on the device: ``Receiver(front_stages=..., front_real=..., front_taps=...)``.  The reference
has no counterpart: the header's text is the definition and this module is the yardstick -- :func:`frames` for the lengths,
:func:`design` for the built-in Kaiser half-band, :func:`apply` for one stage's arithmetic, bit for bit, :func:`run` for the
whole chain.
"""
from __future__ import annotations

import math

import numpy as np

MIN_K, MAX_K, MAX_STAGES, MAX_N = 2, 31, 3, 127


def n_taps(K: int) -> int:
    return 4 * int(K) + 3


def centre(K: int) -> int:
    return 2 * int(K) + 1


def k_of(taps) -> int:
    """K of a prototype of N = 4 K + 3 taps (ValueError for any other length, or K outside 2 .. 31)."""
    n = int(np.size(taps))
    K = (n - 3) // 4
    if n != 4 * K + 3 or not MIN_K <= K <= MAX_K:
        raise ValueError(f"a prototype has N = 4 K + 3 taps with K in 2 .. 31, not {n}")
    return K


def nonzero_order(K: int) -> list[int]:
    """The structurally non-zero k in the order they are summed: 0, 2, .. 2K, 2K+1, 2K+2, .. 4K+2."""
    C = centre(K)
    return [k for k in range(n_taps(K)) if k % 2 == 0 or k == C]


def check_taps(taps) -> np.ndarray:
    """`taps` as float32; ValueError unless every odd k != C is +0.0f, bit for bit (where the library returns SDRX_EINVAL)."""
    h = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    K = k_of(h)
    odd = [k for k in range(1, h.size, 2) if k != centre(K)]
    if h[odd].view(np.uint32).any():
        raise ValueError("every odd tap but the centre must be +0.0f")
    return h


def frames(n0: int, stages: int) -> list[tuple[int, int]]:
    """``[(n_in, n_out)]`` of stage 1 .. `stages` for a fed frame of `n0` samples: stage s has n0 2^(stages - s) outputs."""
    if not 1 <= int(stages) <= MAX_STAGES:
        raise ValueError("stages must be 1, 2 or 3")
    return [(int(n0) << (stages - s + 1), int(n0) << (stages - s)) for s in range(1, stages + 1)]


def in_frame(n0: int, stages: int) -> int:
    return frames(n0, stages)[0][0]


def _i0(x: float) -> float:
    """The power series the library sums, term by term in IEEE double"""
    q = x * x / 4
    s = term = 1.0
    for k in range(1, 200):
        term *= q / (float(k) * k)
        s += term
        if term < s * 1e-18:
            break
    return s


def design(K: int, atten_db: float = 80.0) -> tuple[np.ndarray, dict]:
    """The built-in prototype (float32, N = 4 K + 3 taps) and its info: IEEE double, operation for operation the library's,
    rounded once.  With A = atten_db: beta = 0.1102 (A - 8.7), tw = (A - 7.95) / (2.285 (N - 1) 2 pi),
    h[k] = 0.5 sinc(0.5 (k - C)) I0(beta sqrt(1 - (2k/(N-1) - 1)^2)) / I0(beta), the odd k != C exactly +0.0.  ValueError where
    the library returns SDRX_EFILTER (0.25 - tw / 2 <= 0) or SDRX_EINVAL."""
    K = int(K)
    if not MIN_K <= K <= MAX_K:
        raise ValueError("K must be in 2 .. 31")
    A = float(atten_db)
    if not 50.0 < A <= 120.0:
        raise ValueError("atten_db must be above 50 and at most 120")
    pi = 3.141592653589793238462643383279502884
    N, C = n_taps(K), centre(K)
    beta = 0.1102 * (A - 8.7)
    tw = (A - 7.95) / (2.285 * (N - 1) * 2 * pi)
    if 0.25 - tw / 2 <= 0:
        raise ValueError("the transition is wider than the band")
    i0b = _i0(beta)
    h = np.zeros(N, np.float64)
    for k in range(N):
        if k != C and k & 1:
            continue
        x = 0.5 * (k - C)
        sinc = 1.0 if x == 0 else math.sin(pi * x) / (pi * x)
        r = 2.0 * k / (N - 1) - 1
        arg = 1 - r * r
        win = _i0(beta * math.sqrt(arg if arg > 0 else 0.0)) / i0b
        h[k] = 0.5 * sinc * win
    info = {"real_input": 0, "stages": 0, "K": K, "N": N, "in_frame": 0, "out_frame": 0, "tw": tw, "alias_free": 1.0 - 2.0 * tw}
    return h.astype(np.float32), info


def rotate(r, start: int = 0) -> np.ndarray:
    """z[n] = r[n] (-j)^n for the real samples `r` (float32), n counted from `start`: Re z = +r, 0, -r, 0 and Im z = 0, -r, 0, +r
    for n mod 4 = 0, 1, 2, 3, with -r the negation and 0 a +0.0."""
    r = np.ascontiguousarray(r, dtype=np.float32).reshape(-1)
    ph = (np.arange(r.size, dtype=np.int64) + int(start)) % 4
    z = np.zeros(r.size, np.complex64)
    z.real = np.where(ph == 0, r, np.where(ph == 2, -r, np.float32(0.0)))
    z.imag = np.where(ph == 3, r, np.where(ph == 1, -r, np.float32(0.0)))
    return z


def apply(x, h, real: bool = False, history=None) -> tuple[np.ndarray, np.ndarray]:
    """One frame through one stage: ``(y, history')``.  `x`: the stage's input frame -- complex64, or with `real` the converted
    real samples (float32; a multiple of 4 of them, so that the frame starts at n = 0 mod 4); `h`: the prototype (float32,
    N = 4 K + 3); `history`: the last N - 1 input samples of the previous frame (None: zeros -- the first frame after finalize).
    Per component and output m: acc = +0.0f; acc = fl(acc + fl(h[k] z[2m - k])) over :func:`nonzero_order`.  With `real`,
    z = :func:`rotate` of the samples, I sums the even k only and Q is the single product fl(h[C] Im z[2m - C])."""
    h = check_taps(h)
    K = k_of(h)
    N, C = h.size, centre(K)
    x = np.ascontiguousarray(x, dtype=np.float32 if real else np.complex64).reshape(-1)
    if x.size % (4 if real else 2):
        raise ValueError("a stage's input frame is even (real samples: a multiple of 4)")
    hist = np.zeros(N - 1, x.dtype) if history is None else np.ascontiguousarray(history, dtype=x.dtype).reshape(-1)
    if hist.size != N - 1:
        raise ValueError(f"the history has N - 1 = {N - 1} samples")
    ext = np.concatenate([hist, x])  # ext[N - 1 + n] = x[n]
    z = rotate(ext, -(N - 1)) if real else ext
    re, im = z.real.astype(np.float32), z.imag.astype(np.float32)
    n_out = x.size // 2
    base = 2 * np.arange(n_out, dtype=np.int64) + (N - 1)
    acc_re, acc_im = np.zeros(n_out, np.float32), np.zeros(n_out, np.float32)
    if real:
        for k in range(0, N, 2):
            acc_re = acc_re + h[k] * re[base - k]  # float32 arrays throughout: a product rounded, then a sum rounded
        acc_im = h[C] * im[base - C]
    else:
        for k in nonzero_order(K):
            acc_re = acc_re + h[k] * re[base - k]
            acc_im = acc_im + h[k] * im[base - k]
    y = np.empty(n_out, np.complex64)
    y.real, y.imag = acc_re, acc_im
    return y, ext[ext.size - (N - 1):].copy()


def run(x, h, stages: int, real: bool = False, histories=None) -> tuple[np.ndarray, list]:
    """One frame through all `stages`: ``(y, histories')`` with one history per stage (None: the first frame)."""
    hs = [None] * stages if histories is None else list(histories)
    out = []
    for s in range(stages):
        x, hist = apply(x, h, real and s == 0, hs[s])
        out.append(hist)
    return x, out


def info_dict(r) -> dict:
    """One ``sdrx_front_info`` as a dict."""
    return {"real_input": int(r.real_input), "stages": int(r.stages), "K": int(r.K), "N": int(r.N), "in_frame": int(r.in_frame),
            "out_frame": int(r.out_frame), "tw": float(r.tw), "alias_free": float(r.alias_free)}
