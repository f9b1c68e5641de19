"""What the front stage's tests share: the cases, their small trees, the frames the GPU tests feed, and nine wrong devices.

The cases (real, stages, K, in_frame, n0, n, resampler case), each run for three frames: the smallest shapes at which the kernel
can still go wrong -- a second tile, a short last tile (1296 = 1024 + 272), a history longer than a wave's span (K = 31: 126
samples), every stage count, and one in front of the resampler (16/25, T = 24: tests/resample_ref.py's case).  n0 is the frame
the stage feeds, n the tree's; every tree has fs = 4 n for its parent-less VFOs."""
from __future__ import annotations

import functools

import numpy as np

import resample_ref as rr
from sdrreceiver_amd import front as fr, ingest, resample as rs

#         real stages K  in_frame  n0    n     resampler case
CASES = [(1, 1, 2, 2592, 1296, 1296, None),    # a short last tile of 272
         (1, 1, 31, 4096, 2048, 2048, None),   # the longest history
         (0, 1, 7, 2560, 1280, 1280, None),
         (0, 2, 3, 8192, 2048, 2048, None),
         (1, 3, 7, 16384, 2048, 2048, None),   # real + two complex
         (1, 1, 7, 6400, 3200, 2048, rr.CASES[3])]  # in front of the 16/25, T = 24 resampler
IDS = [f"{'real' if c[0] else 'cplx'}{c[1]}_K{c[2]}_{c[3]}" for c in CASES]
N_FRAMES = 3
COMPLEX_FORMATS = (ingest.CU8, ingest.CS8, ingest.CS16)
REAL_FORMATS = (ingest.RS16, ingest.RU12)

for _c in CASES:
    assert fr.in_frame(_c[4], _c[1]) == _c[3] and (_c[6] is None) == (_c[4] == _c[5])
assert CASES[5][6][3:] == (3200, 2048)


def tree(case):
    """resample_ref's tree at the case's n: a main with a USB and a compress sub, and a parent-less compress leaf."""
    n = case[5]
    return rr.tree(case[6] if case[6] else (1, 1, 8, n, n))


def receiver_kw(case, taps) -> dict:
    """The Receiver arguments of a case with the prototype `taps` (an array, or K for the built-in design)"""
    real, stages, K, in_frame, n0, n, rcase = case
    kw = dict(front_stages=stages, front_real=bool(real), front_taps=taps)
    if rcase:
        kw.update(input_rate=rr.rates(rcase)[0], resample_taps=rr.random_taps(rcase))
    return kw


def formats(case) -> tuple:
    return REAL_FORMATS if case[0] else COMPLEX_FORMATS


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def random_taps(case, seed=0) -> np.ndarray:
    """A prototype with full mantissas on the non-zero positions, of mixed sign, spread over a few binades and NOT symmetric
    (symmetric taps hide a reversed index); the odd k != C are +0.0f."""
    K = case[2]
    rng = np.random.default_rng(2000 + seed + 7 * K)
    h = np.zeros(fr.n_taps(K), np.float32)
    nz = fr.nonzero_order(K)
    h[nz] = (rng.standard_normal(len(nz)) * np.exp2(rng.integers(-3, 2, len(nz)))).astype(np.float32)
    assert not np.array_equal(h, h[::-1]) and (h[nz] != 0).all()
    return h


def impulse_positions(case) -> list[int]:
    K = case[2]
    return [0, fr.centre(K), fr.n_taps(K) - 1]


def impulse_taps(case, k) -> np.ndarray:
    h = np.zeros(fr.n_taps(case[2]), np.float32)
    h[k] = 1.0
    return h


def ramp_frames(case, fmt=None) -> list[tuple[np.ndarray, int]]:
    """[(samples, fmt)] of three frames in which every sample is another value: real int16 counting up (RS16), the 12-bit code
    counting up with the frame number in the four bits above it, which the conversion must drop (RU12), or CS16 with I counting
    up and Q counting down."""
    real, in_frame = case[0], case[3]
    if fmt is None:
        fmt = ingest.RS16 if real else ingest.CS16
    out = []
    for f in range(N_FRAMES):
        j = np.arange(f * in_frame, (f + 1) * in_frame, dtype=np.int64)
        if fmt == ingest.RS16:
            v = (j - 24000).astype(np.int16)
        elif fmt == ingest.RU12:
            v = ((j % 4096) | ((j // 4096 % 16) << 12)).astype(np.uint16)
        else:
            v = np.empty(2 * in_frame, np.int16)
            v[0::2] = (j - 16000).astype(np.int16)
            v[1::2] = (15000 - j).astype(np.int16)
        out.append((v, fmt))
    return out


def full_range(fmt, n, seed) -> np.ndarray:
    """n samples (complex formats: n pairs) over the format's whole range; RU12 with random bits above the code"""
    rng = np.random.default_rng(seed)
    if fmt == ingest.RS16:
        return rng.integers(-32768, 32768, n, dtype=np.int16)
    if fmt == ingest.RU12:
        return rng.integers(0, 65536, n, dtype=np.uint16)
    return rr.full_range(fmt, n, seed)


@functools.lru_cache(maxsize=None)
def arithmetic_frames(case, first=0) -> tuple:
    """Three full-range frames, the format alternating among the formats the context takes: ((samples, fmt), ...)"""
    F = formats(case)
    out = []
    for f in range(N_FRAMES):
        fmt = F[(first + f) % len(F)]
        v = full_range(fmt, case[3], 91 * case[3] + 5 * first + f)
        v.setflags(write=False)
        out.append((v, fmt))
    return tuple(out)


def adc_pair_model(v, fmt, frame=0) -> dict:
    """The ADC meter's record of a real frame: the same memory read as pairs -- even samples in arm I, odd samples in arm Q --
    with the format's own codes and rails (adc_ref.model's record, which knows the complex formats only)"""
    import adc_ref as ar
    c = ingest.codes(v, fmt)
    lo, hi = ingest.rails(fmt)

    def arm(a):
        return {"sum": int(a.sum(dtype=np.int64)), "sum_sq": int((a * a).sum(dtype=np.int64)), "min": int(a.min()), "max": int(a.max()),
                "at_lo": int((a == lo).sum()), "at_hi": int((a == hi).sum()), "longest_rail_run": ar.longest_run((a == lo) | (a == hi))}
    vi, vq = c[0::2], c[1::2]
    return {"frame": int(frame), "n_complex": int(vi.size), "fmt": int(fmt), "measured": 1, "i": arm(vi), "q": arm(vq),
            "sum_iq": int((vi * vq).sum(dtype=np.int64)), "bits": [int(b) for b in np.bincount(ar.bit_lengths(c), minlength=ar.BINS)]}


def to_input(v, fmt) -> np.ndarray:
    """The stage-1 input the library computes from the samples: float32 for the real formats, complex64 for the others"""
    x = ingest.to_float(v, fmt)
    return x if ingest.is_real(fmt) else x.view(np.complex64)


@functools.lru_cache(maxsize=None)
def model_run(case, first=0, seed=0) -> tuple:
    """The front model's three output frames (n0 samples each) for arithmetic_frames(case, first) under random_taps(case, seed)"""
    real, stages = case[0], case[1]
    h, hists, out = random_taps(case, seed), None, []
    for v, fmt in arithmetic_frames(case, first):
        y, hists = fr.run(to_input(v, fmt), h, stages, bool(real), hists)
        y.setflags(write=False)
        out.append(y)
    return tuple(out)


def tree_frames(case, front_out, h_rs=None, hist=None):
    """The tree's raw frame for one front-stage output frame: itself, or behind the case's resampler (its taps, its history)"""
    if not case[6]:
        return front_out, None
    L, M = case[6][:2]
    return rs.apply(front_out, h_rs, L, M, hist)


# ---- wrong devices: each one thing a kernel could get wrong -------------------------------------------------------------------
WRONG = ["fma", "descending_k", "zero_history", "z_2m_plus_k", "phase_2m_plus_1", "plus_j", "centre_on_i", "real_as_pairs",
         "stage2_stage1_history"]


def same_by_construction(case, how) -> str | None:
    """Why a wrong device IS the definition on this case (None: it is not)"""
    real, stages = case[0], case[1]
    if how in ("plus_j", "centre_on_i", "real_as_pairs") and not real:
        return "the case has no real stage"
    if how == "stage2_stage1_history" and stages == 1:
        return "the case has one stage"
    return None


def apply_wrong(x, h, real, history, how) -> tuple[np.ndarray, np.ndarray]:
    """front.apply with one thing wrong; how = None is the definition itself (written out a second time)"""
    h = np.ascontiguousarray(h, dtype=np.float32)
    K = fr.k_of(h)
    N, C = h.size, fr.centre(K)
    if real and how == "real_as_pairs":  # the words read as I,Q pairs: half as many samples, through the complex arithmetic
        r = np.ascontiguousarray(x, dtype=np.float32)
        x = np.concatenate([(r[0::2] + 1j * r[1::2]).astype(np.complex64), np.zeros(r.size // 2, np.complex64)])
        real = False
        history = None if history is None else np.asarray(history).astype(np.complex64)
    x = np.ascontiguousarray(x, dtype=np.float32 if real else np.complex64).reshape(-1)
    hist = np.zeros(N - 1, x.dtype) if history is None or how == "zero_history" else np.asarray(history).astype(x.dtype)
    pad = N + 2  # room behind the frame for the devices that read ahead (zeros)
    ext = np.concatenate([hist, x, np.zeros(pad, x.dtype)])
    if real:
        ph = (np.arange(ext.size, dtype=np.int64) - (N - 1)) % 4
        sign = 1 if how == "plus_j" else -1  # (-j)^n: Im = -r at n = 1 (mod 4)
        re = np.where(ph == 0, ext, np.where(ph == 2, -ext, np.float32(0.0))).astype(np.float32)
        im = np.where(ph == (2 - sign), ext, np.where(ph == (2 + sign), -ext, np.float32(0.0))).astype(np.float32)
    else:
        re, im = ext.real.astype(np.float32), ext.imag.astype(np.float32)
    n_out = x.size // 2
    base = 2 * np.arange(n_out, dtype=np.int64) + (N - 1) + (1 if how == "phase_2m_plus_1" else 0)

    def at(a, k):
        return a[base + k] if how == "z_2m_plus_k" else a[base - k]

    def mac(acc, c, v):
        if how == "fma":
            return (acc.astype(np.float64) + np.float64(c) * v.astype(np.float64)).astype(np.float32)
        return acc + c * v

    order = fr.nonzero_order(K)
    if how == "descending_k":
        order = order[::-1]
    acc_re, acc_im = np.zeros(n_out, np.float32), np.zeros(n_out, np.float32)
    if real:
        for k in order:
            if k % 2 == 0:
                acc_re = mac(acc_re, h[k], at(re, k))
            elif how == "centre_on_i":
                acc_re = mac(acc_re, h[k], at(im, k))
        acc_im = h[C] * at(im, C)
    else:
        for k in order:
            acc_re = mac(acc_re, h[k], at(re, k))
            acc_im = mac(acc_im, h[k], at(im, k))
    y = np.empty(n_out, np.complex64)
    y.real, y.imag = acc_re, acc_im
    return y, np.concatenate([hist, x])[-(N - 1):].copy()


def run_wrong(x, h, stages, real, histories, how) -> tuple[np.ndarray, list]:
    """front.run through apply_wrong: the wrong thing in every stage it can happen in"""
    hs = [None] * stages if histories is None else list(histories)
    out = []
    for s in range(stages):
        hist = hs[s]
        if how == "stage2_stage1_history" and s >= 1 and hs[0] is not None:
            hist = np.asarray(hs[0]).astype(np.complex64)
        x, hist = apply_wrong(x, h, bool(real) and s == 0, hist, how)
        out.append(hist)
    return x, out
