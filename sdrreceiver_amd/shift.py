"""The frequency shift of include/sdrx.h ("Frequency shift") in numpy: the model the device is held to bit for bit.

The stage multiplies the tree's raw frame by ``exp(+j 2 pi p / 2^32)``, ``p = phase + j inc`` in wrapping 32-bit arithmetic, with the
rotation of every sample looked up from three 256-entry tables: ``rot = (A[h] (x) B[m]) (x) C[l]`` with h, m, l the three top bytes
of p, and ``(x)`` the complex product with three fp32 roundings a component.  :func:`apply` is one frame, :class:`State` what
frames hand on, :func:`run` a sequence of frames.  The tables are built with ``math.cos`` / ``math.sin`` (the C library's, as the
library builds its own); integers and single fp32 operations do the rest: there is no tolerance anywhere."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

LOAD_PHASE = 1         # SDRX_SHIFT_LOAD_PHASE
NAN_BITS = 0x7FC00000  # the one NaN a component is
TAB = 256              # entries per table
# geometry of k_shift (sdrreceiver_amd/csrc/sdrx_shift.h): samples per lane, per wave (a tile), per workgroup
LANE, TILE, WORKGROUP = 16, 1024, 4096
STATE_BYTES, TABLE_BYTES, RECORD_BYTES = 16, 3 * TAB * 8, 64  # what the stage holds on the device: STATE + TABLE + 2 * RECORD
RECORD_FIELDS = ("frame", "n_complex", "applied", "phase", "inc", "next_phase", "next_inc")
M32 = 0xFFFFFFFF


@dataclasses.dataclass(frozen=True)
class Cfg:
    inc: int
    phase0: int = 0
    flags: int = 0


@dataclasses.dataclass(frozen=True)
class State:
    """What a frame leaves for the next.  ``State.initial(cfg)`` is the state after ``sdrx_finalize``"""
    phase: int = 0
    inc: int = 0
    frame: int = 0

    @staticmethod
    def initial(cfg: Cfg) -> "State":
        return State(int(cfg.phase0) & M32, int(cfg.inc) & M32, 0)


def check_cfg(cfg: Cfg) -> str | None:
    """None, or why the library refuses these settings (SDRX_EINVAL)"""
    if not (0 <= int(cfg.inc) <= M32 and 0 <= int(cfg.phase0) <= M32):
        return "inc and phase0 are 32-bit words"
    if int(cfg.flags) & ~LOAD_PHASE:
        return "flags: only bit 0 is defined"
    return None


@functools.lru_cache(maxsize=None)
def tables() -> tuple:
    """(A, B, C): 256 complex64 each, (cos, sin)(2 pi k / 2^8), (.. / 2^16), (.. / 2^24) in double, rounded once; read-only"""
    out = []
    for denom in (256.0, 65536.0, 16777216.0):
        t = np.empty(TAB, np.complex64)
        for k in range(TAB):
            a = 2 * math.pi * float(k) / denom
            t[k] = complex(np.float32(math.cos(a)), np.float32(math.sin(a)))
        t.setflags(write=False)
        out.append(t)
    return tuple(out)


def inc_of(fs_tree: float, hz: float) -> int:
    """sdrx_shift_inc: rint(hz / fs_tree 2^32) in double, ties to even, mod 2^32; ValueError where the library says SDRX_EINVAL"""
    fs_tree, hz = float(fs_tree), float(hz)
    if not (math.isfinite(fs_tree) and math.isfinite(hz)) or not fs_tree > 0 or not abs(hz) <= fs_tree / 2:
        raise ValueError("shift: fs_tree must be positive and finite, |hz| at most fs_tree / 2")
    return int(np.rint(np.float64(hz) / np.float64(fs_tree) * np.float64(4294967296.0))) & M32


def hz_of(fs_tree: float, inc: int) -> float:
    """sdrx_shift_hz: the signed inverse"""
    inc = int(inc) & M32
    return float(np.float64(inc - (1 << 32) if inc >= 1 << 31 else inc) * np.float64(fs_tree) / np.float64(4294967296.0))


def follow(hz_now: float, drift_hz: float, gain: float = 1.0, *, fs: float) -> float:
    """The shift that closes the loop on ``drift.py``'s estimate: hz_now - gain drift_hz, clamped to +-fs / 2 (fs: the tree's
    rate).  A band that sits D Hz high peaks at +D in the drift profile and is corrected by a shift of -D."""
    return float(min(fs / 2, max(-fs / 2, hz_now - gain * drift_hz)))


def phases(phase: int, inc: int, n: int) -> np.ndarray:
    """p of samples 0 .. n - 1: (phase + j inc) mod 2^32, uint32"""
    return ((np.uint64(int(phase) & M32) + np.arange(n, dtype=np.uint64) * np.uint64(int(inc) & M32)) & np.uint64(M32)).astype(np.uint32)


def split(p) -> tuple:
    """(h, m, l): the three top bytes of p; the low byte is dropped"""
    p = np.asarray(p, dtype=np.uint32)
    return (p >> np.uint32(24)).astype(np.intp), ((p >> np.uint32(16)) & np.uint32(255)).astype(np.intp), ((p >> np.uint32(8)) & np.uint32(255)).astype(np.intp)


def cmul(a, b) -> np.ndarray:
    """a (x) b = ( fl(fl(ar br) - fl(ai bi)), fl(fl(ar bi) + fl(ai br)) )"""
    a, b = np.asarray(a, dtype=np.complex64), np.asarray(b, dtype=np.complex64)
    ar, ai, br, bi = (np.ascontiguousarray(v, dtype=np.float32) for v in (a.real, a.imag, b.real, b.imag))
    y = np.empty(np.broadcast(a, b).shape, np.complex64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        y.real = (ar * br).astype(np.float32) - (ai * bi).astype(np.float32)
        y.imag = (ar * bi).astype(np.float32) + (ai * br).astype(np.float32)
    return y


def rotation(p) -> np.ndarray:
    """rot = (A[h] (x) B[m]) (x) C[l] of every phase in p"""
    A, B, C = tables()
    h, m, l = split(p)
    return cmul(cmul(A[h], B[m]), C[l])


def mix(x, phase: int, inc: int) -> np.ndarray:
    """y = x (x) rot; a component that is a NaN is the quiet NaN 0x7fc00000"""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    y = cmul(x, rotation(phases(phase, inc, x.size)))
    u = y.view(np.uint32)
    u[np.isnan(y.view(np.float32))] = NAN_BITS
    return y


def apply(x, state: State) -> tuple[np.ndarray, dict, State]:
    """One frame: (the shifted frame, its record, the state for the next frame)"""
    y = mix(x, state.phase, state.inc)
    n = y.size
    nxt = (state.phase + n * state.inc) & M32
    rec = {"frame": state.frame, "n_complex": n, "applied": 1, "phase": state.phase, "inc": state.inc, "next_phase": nxt, "next_inc": state.inc}
    return y, rec, State(nxt, state.inc, state.frame + 1)


def load(state: State, cfg: Cfg) -> State:
    """sdrx_set_shift between two frames: the increment, and under LOAD_PHASE the phase"""
    return State(int(cfg.phase0) & M32 if cfg.flags & LOAD_PHASE else state.phase, int(cfg.inc) & M32, state.frame)


def run(frames, cfg) -> tuple[list[np.ndarray], list[dict]]:
    """A sequence of frames from the state after sdrx_finalize; `cfg`: one Cfg, or one per frame (a later one that is another
    object than its predecessor is set in front of its frame, as sdrx_set_shift does)"""
    first = cfg if isinstance(cfg, Cfg) else cfg[0]
    state, out, recs = State.initial(first), [], []
    for f, x in enumerate(frames):
        if f and not isinstance(cfg, Cfg) and cfg[f] is not cfg[f - 1]:
            state = load(state, cfg[f])
        y, rec, state = apply(x, state)
        out.append(y)
        recs.append(rec)
    return out, recs


def reference(x, phase: int, inc: int) -> np.ndarray:
    """x exp(j 2 pi p / 2^32) in double, complex128: what the tables approximate (for accuracy figures only)"""
    p = phases(phase, inc, np.asarray(x).size).astype(np.float64)
    return np.asarray(x, dtype=np.complex128).reshape(-1) * np.exp(2j * np.pi * p / 4294967296.0)


def record_dict(r) -> dict:
    """struct sdrx_shift_record as a dict of Python integers"""
    return {k: int(getattr(r, k)) for k in RECORD_FIELDS}


def cfg_of(c) -> Cfg:
    """struct sdrx_shift_cfg as a Cfg"""
    return Cfg(int(c.inc), int(c.phase0), int(c.flags))
