"""What the resampler's tests share: the ratios, their small trees, the frames the GPU tests feed, and eight wrong devices.

The ratios (L, M, T, n_in -> n), each run for three frames.  Every tree has fs = 4 n for its parent-less VFOs, so the input
rate is 4 n_in: the ratio is that of the frame lengths."""
from __future__ import annotations

import functools

import numpy as np

from sdrreceiver_amd import ingest, resample as rs, topology as tp

#        L    M    T   n_in   n
CASES = [(128, 125, 32, 4000, 4096),
         (384, 625, 32, 10000, 6144),
         (3, 4, 16, 1728, 1296),     # a short last output chunk of 272
         (16, 25, 24, 3200, 2048),
         (5, 3, 16, 768, 1280)]      # upsampling
IDS = [f"{L}_{M}" for L, M, *_ in CASES]
N_FRAMES = 3
FORMATS = (ingest.CU8, ingest.CS8, ingest.CS16)


def rates(case) -> tuple[int, int]:
    """(fs_in, fs_out) of a case's tree"""
    L, M, T, n_in, n = case
    assert (L, M) == rs.ratio(4 * n_in, 4 * n) and n * M == n_in * L
    return 4 * n_in, 4 * n


def tree(case) -> tp.Topology:
    """A main with one USB and one compress sub (the main at d = 1 where half a frame is still a frame the library takes),
    and a parent-less compress leaf, whose watch source is the raw frame."""
    L, M, T, n_in, n = case
    d = 1 if (n // 2) % 16 == 0 and (n // 2) % 1024 in (0, *range(256, 1024)) else 0
    fs = 4 * n
    t = tp.Topology(fs=fs, frame=n, name=f"rs{L}_{M}")
    t.vfos.append(tp.VfoDesc(topic="MAIN0", parent=-1, fs=fs, decimate_count=d, mixer_freq=float(n // 7), demod_usb=False, cstyle=1,
                             samples_per_buffer=n))
    t.vfos.append(tp.VfoDesc(topic="USB01", parent=0, fs=fs >> d, decimate_count=0, mixer_freq=float(n // 11), filter_bw=0, gain=tp._g(0.05),
                             samples_per_buffer=n >> d))
    t.vfos.append(tp.VfoDesc(topic="CMP02", parent=0, fs=fs >> d, decimate_count=0, mixer_freq=-float(n // 13), demod_usb=False, cstyle=1,
                             samples_per_buffer=n >> d))
    t.vfos.append(tp.VfoDesc(topic="RAW03", parent=-1, fs=fs, decimate_count=0, mixer_freq=-float(n // 5), demod_usb=False, cstyle=0,
                             samples_per_buffer=n))
    return t


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def random_taps(case, seed=0) -> np.ndarray:
    """L T taps with full mantissas, of mixed sign and spread over a few binades (sums of T products round at every step)"""
    L, M, T, *_ = case
    rng = np.random.default_rng(1000 + seed + L)
    return (rng.standard_normal(L * T) * np.exp2(rng.integers(-3, 2, L * T))).astype(np.float32)


def impulse_positions(case) -> list[int]:
    L, M, T, *_ = case
    return [0, L - 1, L, L * T - 1, (L * T) // 2 + 1]


def impulse_taps(case, k) -> np.ndarray:
    L, M, T, *_ = case
    h = np.zeros(L * T, np.float32)
    h[k] = 1.0
    return h


def ramp_frames(case) -> list[np.ndarray]:
    """CS16: I counts up through the three frames, Q counts down -- every sample of the three frames is another value"""
    n_in = case[3]
    out = []
    for f in range(N_FRAMES):
        j = np.arange(f * n_in, (f + 1) * n_in, dtype=np.int64)
        v = np.empty(2 * n_in, np.int16)
        v[0::2] = (j - 16000).astype(np.int16)
        v[1::2] = (15000 - j).astype(np.int16)
        out.append(v)
    return out


def full_range(fmt, n, seed) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if fmt == ingest.CU8:
        return rng.integers(0, 256, 2 * n, dtype=np.uint8)
    if fmt == ingest.CS8:
        return rng.integers(-128, 128, 2 * n, dtype=np.int8)
    return rng.integers(-32768, 32768, 2 * n, dtype=np.int16)


@functools.lru_cache(maxsize=None)
def arithmetic_frames(case, first=0) -> tuple:
    """Three full-range frames, the format alternating (frame f has format FORMATS[(first + f) % 3])"""
    n_in = case[3]
    return tuple(full_range(FORMATS[(first + f) % 3], n_in, 77 * case[0] + 3 * first + f) for f in range(N_FRAMES))


def to_complex(v) -> np.ndarray:
    return ingest.to_float(v).view(np.complex64)


@functools.lru_cache(maxsize=None)
def model_run(case, first=0, seed=0) -> tuple:
    """The model's three output frames for arithmetic_frames(case, first) under random_taps(case, seed): computed once."""
    L, M, *_ = case
    h, hist, out = random_taps(case, seed), None, []
    for v in arithmetic_frames(case, first):
        y, hist = rs.apply(to_complex(v), h, L, M, hist)
        y.setflags(write=False)
        out.append(y)
    return tuple(out)


# ---- wrong devices: each one thing a kernel could get wrong -------------------------------------------------------------------
WRONG = ["fma", "descending_t", "zero_history", "x_i_plus_t", "i_off_by_one", "round_not_floor", "prototype_major", "phase_m_mod_L"]


def apply_wrong(x, taps, L, M, history, how) -> tuple[np.ndarray, np.ndarray]:
    """resample.apply with one thing wrong; how = None is the definition itself (written out a second time)"""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    h = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    T = h.size // L
    n_out = x.size * L // M
    hist = np.zeros(T - 1, np.complex64) if history is None or how == "zero_history" else history
    pad = T + 2  # room behind the frame for the devices that read ahead (zeros)
    ext = np.concatenate([hist, x, np.zeros(pad, np.complex64)])
    re, im = ext.real.astype(np.float32), ext.imag.astype(np.float32)
    m = np.arange(n_out, dtype=np.int64)
    p = m * M
    i = p // L
    ph = p % L
    if how == "i_off_by_one":
        i = i + 1
    if how == "round_not_floor":
        i = (2 * p + L) // (2 * L)
    if how == "phase_m_mod_L":
        ph = m % L
    acc_re, acc_im = np.zeros(n_out, np.float32), np.zeros(n_out, np.float32)
    order = range(T - 1, -1, -1) if how == "descending_t" else range(T)
    for t in order:
        c = h[ph * T + t] if how == "prototype_major" else h[ph + t * L]
        j = (i + t if how == "x_i_plus_t" else i - t) + (T - 1)
        if how == "fma":
            acc_re = (acc_re.astype(np.float64) + c.astype(np.float64) * re[j].astype(np.float64)).astype(np.float32)
            acc_im = (acc_im.astype(np.float64) + c.astype(np.float64) * im[j].astype(np.float64)).astype(np.float32)
        else:
            acc_re = acc_re + c * re[j]
            acc_im = acc_im + c * im[j]
    y = np.empty(n_out, np.complex64)
    y.real, y.imag = acc_re, acc_im
    return y, np.concatenate([hist, x])[-(T - 1):].copy()


def same_by_construction(case, how) -> bool:
    """A wrong device that IS the definition for this ratio: m mod L = m M mod L when M = 1 (mod L)"""
    L, M, *_ = case
    return how == "phase_m_mod_L" and M % L == 1
