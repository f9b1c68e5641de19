"""The impulse blanker of include/sdrx.h ("Impulse blanker") in numpy: the model the device is held to bit for bit.

The stage zeroes the samples of a cf32 frame whose power exceeds ``ratio`` times a rank of the PREVIOUS frame's power histogram
(and ``floor``), and ``guard`` samples on either side of each.  :func:`apply` is one frame, :class:`State` what frames hand on,
:func:`run` a sequence of frames.  Everything is integer or single-rounding fp32 arithmetic: there is no tolerance anywhere."""
from __future__ import annotations

import dataclasses

import numpy as np

BINS = 2048
MAX_BIN = 2040      # bin of +inf: the highest reference
MAX_GUARD = 64
NO_HIT = MAX_GUARD + 1  # tail_gap of a frame without a hit, and the most it is stored as
INF_BITS = 0x7F800000
# geometry of k_blank (sdrreceiver_amd/csrc/sdrx_blank.h): samples per lane, per wave (a tile), per workgroup; halo of the bitmap
LANE, TILE, WORKGROUP, HALO = 16, 1024, 4096, 128
RECORD_FIELDS = ("frame", "n_complex", "measured", "thr_bits", "ref_bin", "next_ref_bin", "hits", "blanked", "runs", "carry_in")


@dataclasses.dataclass(frozen=True)
class Cfg:
    ratio: float
    floor: float
    rank_q16: int
    guard: int


@dataclasses.dataclass(frozen=True)
class State:
    """What a frame leaves for the next; the default is the state after ``sdrx_finalize``"""
    ref_bin: int = -1
    tail_gap: int = NO_HIT
    last_blank: bool = False
    frame: int = 0


def check_cfg(cfg: Cfg) -> str | None:
    """None, or why the library refuses these settings (SDRX_EINVAL)"""
    with np.errstate(over="ignore"):  # (a value beyond fp32 is inf there: refused)
        r, f = np.float32(cfg.ratio), np.float32(cfg.floor)
    if not np.isfinite(r) or not r >= 1:
        return "ratio must be finite and at least 1"
    if not np.isfinite(f) or not f >= 0:
        return "floor must be finite and at least 0"
    if not 1 <= int(cfg.rank_q16) <= 65536:
        return "rank_q16 must be in 1 .. 65536"
    if not 0 <= int(cfg.guard) <= MAX_GUARD:
        return "guard must be in 0 .. 64"
    return None


def power(x) -> np.ndarray:
    """p = fl(fl(re re) + fl(im im)): three fp32 roundings"""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    f = x.view(np.float32)
    re, im = f[0::2], f[1::2]
    with np.errstate(over="ignore", invalid="ignore"):
        return (re * re).astype(np.float32) + (im * im).astype(np.float32)


def bin_of(p) -> np.ndarray:
    """(bits(p) & 0x7fffffff) >> 20: an eighth of an octave of power per bin"""
    return ((np.ascontiguousarray(p, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)) >> np.uint32(20)).astype(np.int64)


def edge(b: int) -> np.float32:
    """The bin's lower edge: the float whose bits are b << 20"""
    return np.array([int(b) << 20], np.uint32).view(np.float32)[0]


def threshold(ref_bin: int, cfg: Cfg) -> np.float32:
    if ref_bin < 0:
        return np.float32(np.inf)
    with np.errstate(over="ignore"):
        t = np.float32(cfg.ratio) * edge(ref_bin)
    return max(np.float32(t), np.float32(cfg.floor))


def thr_bits(t) -> int:
    return int(np.array([t], np.float32).view(np.uint32)[0])


def rank_bin(hist, n: int, rank_q16: int) -> int:
    """min(2040, the smallest b with 65536 cum(b) >= rank_q16 n); Python integers, so no width to think about"""
    cum = 0
    for b in range(BINS):
        cum += int(hist[b])
        if 65536 * cum >= int(rank_q16) * int(n):
            return min(b, MAX_BIN)
    return MAX_BIN


def dilate(hit: np.ndarray, guard: int) -> np.ndarray:
    """blank[j] = some hit[m] with |m - j| <= guard, inside the frame"""
    n = hit.size
    c = np.concatenate([[0], np.cumsum(hit, dtype=np.int64)])
    j = np.arange(n)
    return c[np.minimum(j + guard + 1, n)] - c[np.maximum(j - guard, 0)] > 0


def apply(x, cfg: Cfg, state: State = State()) -> tuple[np.ndarray, dict, State]:
    """One frame: (the blanked frame, its record, the state for the next frame)"""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    n, G = x.size, int(cfg.guard)
    p = power(x)
    thr = threshold(state.ref_bin, cfg)
    hit = p > thr
    carry = min(n, max(0, G - state.tail_gap))
    blank = dilate(hit, G)
    blank[:carry] = True
    y = x.copy()
    y[blank] = 0
    hist = np.bincount(bin_of(p), minlength=BINS)
    nxt = rank_bin(hist, n, cfg.rank_q16)
    where = np.flatnonzero(hit)
    tail_gap = min(NO_HIT, n - 1 - int(where[-1])) if where.size else NO_HIT
    before = np.concatenate([[state.last_blank], blank[:-1]])
    rec = {"frame": state.frame, "n_complex": n, "measured": 1, "thr_bits": thr_bits(thr), "ref_bin": state.ref_bin, "next_ref_bin": nxt,
           "hits": int(hit.sum()), "blanked": int(blank.sum()), "runs": int((blank & ~before).sum()), "carry_in": carry}
    return y, rec, State(nxt, tail_gap, bool(blank[-1]), state.frame + 1)


def run(frames, cfg) -> tuple[list[np.ndarray], list[dict]]:
    """A sequence of frames from the state after sdrx_finalize; `cfg`: one Cfg, or one per frame"""
    state, out, recs = State(), [], []
    for f, x in enumerate(frames):
        y, rec, state = apply(x, cfg if isinstance(cfg, Cfg) else cfg[f], state)
        out.append(y)
        recs.append(rec)
    return out, recs


def record_dict(r) -> dict:
    """struct sdrx_blanker_record as a dict of Python integers"""
    return {k: int(getattr(r, k)) for k in RECORD_FIELDS}


def cfg_of(c) -> Cfg:
    """struct sdrx_blanker_cfg as a Cfg"""
    return Cfg(float(c.ratio), float(c.floor), int(c.rank_q16), int(c.guard))
