"""numpy model of the drift estimate (include/sdrx.h "Drift estimate") for the tests: the yardstick, since the reference has no
counterpart.

* :func:`profile` -- ``profile[s] = sum_i T[i] * PSD[(i + s) mod N]`` for ``s = -K .. K``: the products rounded to double once, their
  sum exact and correctly rounded (``math.fsum``), so the model lies within 2 * 2^-53 relative of the exact value.
* :func:`argmax` -- the first maximum in the order 0, -1, +1, -2, +2, ...; :func:`record` -- what the device reports for a profile.
* :func:`estimate` -- the parabola through the peak and its neighbours, written on its own (not sdrreceiver_amd.drift's).
* :func:`separation` -- runner-up / peak of a profile: the condition on the inputs under which device and model must agree on
  ``shift`` although their profiles differ by rounding.
* :func:`stream` -- tones of distinct amplitudes plus Gaussian noise, all moved by a drift in Hz.
"""
from __future__ import annotations

import math

import numpy as np

N = 8192
MAX_SHIFT = 1024
EPS = 2.0 ** -53
BOUND = (N + 4) * EPS      # device against model, relative (derived in include/sdrx.h)
SEPARATION = 1.0 - 1e-6    # the runner-up of every input `shift` is compared on lies at or below this times the peak


def profile(T: np.ndarray, psd: np.ndarray, K: int) -> np.ndarray:
    """[s + K] for s = -K .. K"""
    T = np.asarray(T, np.float64)
    psd = np.asarray(psd, np.float64)
    nz = np.nonzero(T)[0]  # (a zero entry contributes an exact 0)
    t = T[nz]
    out = np.zeros(2 * K + 1, np.float64)
    for s in range(-K, K + 1):
        out[s + K] = math.fsum((t * psd[(nz + s) % N]).tolist())
    return out


def order(K: int) -> list[int]:
    """the shifts in the order the maximum is searched: 0, -1, +1, -2, +2, ..."""
    out = [0]
    for k in range(1, K + 1):
        out += [-k, k]
    return out


def argmax(prof: np.ndarray) -> int:
    K = (len(prof) - 1) // 2
    best, shift = prof[K], 0
    for s in order(K):
        if prof[s + K] > best:
            best, shift = prof[s + K], s
    return shift


def record(prof: np.ndarray) -> dict:
    K = (len(prof) - 1) // 2
    s = argmax(prof)
    return {"shift": s, "max_shift": K, "peak": float(prof[s + K]), "left": float(prof[s - 1 + K]) if s - 1 >= -K else 0.0,
            "right": float(prof[s + 1 + K]) if s + 1 <= K else 0.0, "zero": float(prof[K])}


def estimate(rec: dict) -> float:
    """bins"""
    s, K = rec["shift"], rec["max_shift"]
    if s == K or s == -K:
        return float(s)
    den = rec["left"] - 2.0 * rec["peak"] + rec["right"]
    if den == 0.0:
        return float(s)
    return s + 0.5 * (rec["left"] - rec["right"]) / den


def separation(prof: np.ndarray) -> float:
    """the largest value beside the first maximum, over the maximum (1.0: a tie; an all-zero profile has none to speak of: 0.0)"""
    K = (len(prof) - 1) // 2
    s = argmax(prof)
    peak = prof[s + K]
    if not peak > 0:
        return 0.0
    rest = np.delete(prof, s + K)
    return float(rest.max() / peak) if rest.size else 0.0


def default_tones(fs: float) -> list[tuple[float, float]]:
    """eight tones at fs (-0.4 + 0.1 k) + 37 k Hz, amplitudes 5 + k"""
    return [(fs * (-0.4 + 0.1 * k) + 37.0 * k, 5.0 + k) for k in range(8)]


def stream(fs: float, n: int, drift_hz: float, seed: int, tones=None, start: int = 0, noise: float = 1.0) -> np.ndarray:
    """n complex64 samples at `fs`: the tones [(Hz, amplitude)] (default :func:`default_tones`), every one moved up by `drift_hz`,
    plus Gaussian noise of `noise` per component; phase-continuous over frames through `start`."""
    tones = default_tones(fs) if tones is None else tones
    rng = np.random.default_rng(seed)
    k = np.arange(start, start + n, dtype=np.float64)
    z = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for f, a in tones:
        z += a * np.exp(2j * np.pi * ((f + drift_hz) / fs) * k)
    return z.astype(np.complex64)


def interleaved(z: np.ndarray) -> np.ndarray:
    """complex64 -> the raw frame's float32 [I0, Q0, I1, Q1, ...]"""
    return np.ascontiguousarray(z, np.complex64).view(np.float32).copy()


# ---- the inputs of the GPU tests (tests/test_gpu_drift.py), built here so that tests/test_drift_model.py can check the
# ---- separation condition on them without a GPU
WT_DRIFT_HZ = 45.0   # 12 bins of the 3.75 Hz the main of watch_ref.watch_tree() has
WT_K = 64


def wt_tones(topo) -> list[tuple[float, float]]:
    """one tone mid-band of every USB sub of watch_ref.watch_tree(), amplitudes 20, 25, ..."""
    import watch_ref as wr
    return [(wr.tone_for(topo, k), 15.0 + 5.0 * k) for k in range(1, 9)]


def wt_frame(topo, drift_hz: float, seed: int, start: int = 0) -> np.ndarray:
    """a raw frame (interleaved float32) for watch_ref.watch_tree()"""
    return interleaved(stream(topo.fs, topo.frame, drift_hz, seed, tones=wt_tones(topo), start=start))


RAW_DRIFT_BINS = 2   # of the raw frame's spectrum: 16 bins of the parent's, whose rate is an eighth
RAW_K = 32


def drift_tree(n_parent: int):
    """A main at d = 3 whose stream has n_parent samples per frame with two USB subs and a compress sub below it, and two
    parent-less leaves: the sources are the parent's tile-layout stream and the raw frame of 8 n_parent samples."""
    from sdrreceiver_amd.topology import Topology, VfoDesc
    n = 8 * n_parent
    t = Topology(fs=4 * n, frame=n, name=f"drift-{n_parent}")
    t.vfos.append(VfoDesc(parent=-1, fs=4 * n, decimate_count=3, mixer_freq=float(n // 3 + 37), demod_usb=False, cstyle=1,
                          samples_per_buffer=n))
    s = dict(parent=0, fs=n // 2, samples_per_buffer=n_parent, cstyle=1)
    t.vfos.append(VfoDesc(topic="S1", decimate_count=2, mixer_freq=float(n // 16 + 11), gain=0.01, **s))
    t.vfos.append(VfoDesc(topic="S2", decimate_count=2, mixer_freq=-1234.625, filter_bw=n // 64, gain=0.01, **s))
    t.vfos.append(VfoDesc(topic="S3", decimate_count=3, mixer_freq=float(-n // 8), demod_usb=False, scalecomp=4, **s))
    t.vfos.append(VfoDesc(topic="R1", parent=-1, fs=4 * n, decimate_count=4, mixer_freq=float(n + 5), gain=0.01, cstyle=1,
                          samples_per_buffer=n))
    t.vfos.append(VfoDesc(topic="R2", parent=-1, fs=4 * n, decimate_count=3, mixer_freq=float(-n // 2), demod_usb=False, cstyle=0,
                          samples_per_buffer=n))
    return t


DT_PARENT_LEAF, DT_RAW_LEAF = 1, 4  # a leaf of each source of drift_tree


def drift_tree_tones(topo) -> list[tuple[float, float]]:
    """eight tones inside the main's band of the raw frame (it hears [-f0 - fs/16, -f0 + fs/16]), amplitudes 5 + k"""
    f0, half = topo.vfos[0].mixer_freq, topo.fs / 16.0
    return [(-f0 + half * (-0.8 + 0.2 * k) + 37.0 * k, 5.0 + k) for k in range(8)]


def raw_frame(topo, drift_hz: float, seed: int) -> np.ndarray:
    """a raw frame for drift_tree with its eight tones, components rounded to integers in -100 .. 100 (so that the same frame can
    be fed as dongle bytes: b = component + 127)"""
    z = stream(topo.fs, topo.frame, drift_hz, seed, tones=drift_tree_tones(topo), noise=2.0)
    x = np.clip(np.rint(interleaved(z)), -100, 100)
    return x.astype(np.float32)
