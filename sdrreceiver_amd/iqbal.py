"""The IQ balance correction of include/sdrx.h ("IQ balance") in numpy: the model the device is held to bit for bit.

The stage replaces Q by ``fl(fl(c I) + fl(d Q))`` and moves the pair ``(c, d)`` once per frame from exact integer statistics of
what it produced.  :func:`apply` is one frame, :class:`State` what frames hand on, :func:`run` a sequence of frames.  The apply is
three fp32 roundings, the statistics are integers, the step is a fixed sequence of single IEEE double operations: there is no
tolerance anywhere."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

IQ_LOAD = 1         # SDRX_IQ_LOAD
CLAMP = 32767       # |q(x)| at the most
NAN_BITS = 0x7FC00000  # the one NaN a Q' is
MAX_C, MIN_D, MAX_D = 0.5, 0.5, 2.0
# geometry of k_iqbal (sdrreceiver_amd/csrc/sdrx_iqbal.h): samples per lane, per wave (a tile), per workgroup
LANE, TILE, WORKGROUP = 16, 1024, 4096
STATE_BYTES, RECORD_BYTES = 64, 96  # what the stage holds on the device: STATE_BYTES + 2 * RECORD_BYTES
SUMS = ("sum_i", "sum_q", "sum_iq", "sum_ii", "sum_qq")
RECORD_FIELDS = ("frame", "n_complex", "measured", "adapted", "rejected", "c_bits", "d_bits", "next_c_bits", "next_d_bits") + SUMS


@dataclasses.dataclass(frozen=True)
class Cfg:
    mu: float
    min_power: float
    c0: float = 0.0
    d0: float = 1.0
    flags: int = 0


@dataclasses.dataclass(frozen=True)
class State:
    """What a frame leaves for the next: the pair as fp32 values held in Python floats.  ``State.initial(cfg)`` is the state
    after ``sdrx_finalize``"""
    c: float = 0.0
    d: float = 1.0
    frame: int = 0

    @staticmethod
    def initial(cfg: Cfg) -> "State":
        return State(float(np.float32(cfg.c0)), float(np.float32(cfg.d0)), 0)


def bits(x) -> int:
    return int(np.array([x], np.float32).view(np.uint32)[0])


def from_bits(u: int) -> float:
    return float(np.array([u], np.uint32).view(np.float32)[0])


def check_cfg(cfg: Cfg) -> str | None:
    """None, or why the library refuses these settings (SDRX_EINVAL)"""
    with np.errstate(over="ignore"):  # (a value beyond fp32 is inf there: refused)
        mu, mp, c0, d0 = (np.float32(v) for v in (cfg.mu, cfg.min_power, cfg.c0, cfg.d0))
    if not (mu >= 0 and mu <= 1):
        return "mu must be in 0 .. 1"
    if not np.isfinite(mp) or not mp >= 0:
        return "min_power must be finite and at least 0"
    if not (c0 >= -MAX_C and c0 <= MAX_C):
        return "c0 must be in -0.5 .. 0.5"
    if not (d0 >= MIN_D and d0 <= MAX_D):
        return "d0 must be in 0.5 .. 2"
    if int(cfg.flags) & ~IQ_LOAD:
        return "flags: only bit 0 is defined"
    return None


def correct(x, c, d) -> np.ndarray:
    """Rule 1: I' = I (bits kept), Q' = fl(fl(c I) + fl(d Q)); a NaN Q' is the quiet NaN 0x7fc00000"""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    y = x.copy()
    f, g = x.view(np.float32), y.view(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        a = (np.float32(c) * f[0::2]).astype(np.float32)
        b = (np.float32(d) * f[1::2]).astype(np.float32)
        g[1::2] = (a + b).astype(np.float32)
    u = y.view(np.uint32)
    u[1::2][np.isnan(g[1::2])] = NAN_BITS
    return y


def quantise(v) -> np.ndarray:
    """Rule 2: 0 for NaN, else fl(x 256) rounded to nearest even, saturated to +-32767; int64"""
    with np.errstate(over="ignore", invalid="ignore"):
        w = (np.ascontiguousarray(v, dtype=np.float32) * np.float32(256)).astype(np.float32)
        w = np.where(np.isnan(w), np.float32(0), np.clip(w, -CLAMP, CLAMP))
    return np.rint(w).astype(np.int64)


def sums(y) -> dict:
    """Rule 3 of a frame as it leaves the stage: Python integers"""
    f = np.ascontiguousarray(y, dtype=np.complex64).reshape(-1).view(np.float32)
    qi, qq = quantise(f[0::2]), quantise(f[1::2])
    return {"sum_i": int(qi.sum()), "sum_q": int(qq.sum()), "sum_iq": int((qi * qq).sum()), "sum_ii": int((qi * qi).sum()),
            "sum_qq": int((qq * qq).sum())}


def moments(s: dict, n: int) -> tuple:
    """(A, B, C) of rule 4: single double operations in the header's order"""
    D = np.float64
    N = D(n)
    mi, mq = D(s["sum_i"]) / N, D(s["sum_q"]) / N
    A = D(s["sum_ii"]) / N - mi * mi
    B = D(s["sum_qq"]) / N - mq * mq
    C = D(s["sum_iq"]) / N - mi * mq
    return A, B, C


def pair_ok(c, d) -> bool:
    return bool(np.isfinite(c) and np.isfinite(d) and abs(c) <= MAX_C and MIN_D <= d <= MAX_D)


def step(s: dict, n: int, cfg: Cfg, c, d) -> dict:
    """Rule 4: measured / adapted / rejected and the next pair (fp32 values)"""
    D = np.float64
    c, d, mu = np.float32(c), np.float32(d), np.float32(cfg.mu)
    A, B, C = moments(s, n)
    out = {"measured": 0, "adapted": 0, "rejected": 0, "c": float(c), "d": float(d)}
    if not (A > 0 and B > 0 and (A + B) * D(2.0 ** -16) >= D(np.float32(cfg.min_power))):
        return out
    out["measured"] = 1
    if not mu > 0:
        return out
    m = D(mu)
    with np.errstate(over="ignore", invalid="ignore"):
        ep = C / A
        eg = (A - B) / (A + B)
        g = D(1) + m * eg
        cn = np.float32(g * (D(c) - m * ep))
        dn = np.float32(g * D(d))
    if pair_ok(cn, dn):
        out.update(adapted=1, c=float(cn), d=float(dn))
    else:
        out["rejected"] = 1
    return out


def apply(x, cfg: Cfg, state: State | None = None) -> tuple[np.ndarray, dict, State]:
    """One frame: (the corrected frame, its record, the state for the next frame); state None: the one after sdrx_finalize"""
    st = State.initial(cfg) if state is None else state
    y = correct(x, st.c, st.d)
    n = y.size
    s = sums(y)
    r = step(s, n, cfg, st.c, st.d)
    rec = {"frame": st.frame, "n_complex": n, "measured": r["measured"], "adapted": r["adapted"], "rejected": r["rejected"], "c_bits": bits(st.c),
           "d_bits": bits(st.d), "next_c_bits": bits(r["c"]), "next_d_bits": bits(r["d"]), **s}
    return y, rec, State(r["c"], r["d"], st.frame + 1)


def run(frames, cfg) -> tuple[list[np.ndarray], list[dict]]:
    """A sequence of frames from the state after sdrx_finalize; `cfg`: one Cfg, or one per frame (a later one with IQ_LOAD in its
    flags loads its c0, d0 in front of its frame, as sdrx_set_iq_balance does)"""
    first = cfg if isinstance(cfg, Cfg) else cfg[0]
    state, out, recs = State.initial(first), [], []
    for f, x in enumerate(frames):
        cf = cfg if isinstance(cfg, Cfg) else cfg[f]
        if f and not isinstance(cfg, Cfg) and cf is not cfg[f - 1] and cf.flags & IQ_LOAD:
            state = State(float(np.float32(cf.c0)), float(np.float32(cf.d0)), state.frame)
        y, rec, state = apply(x, cf, state)
        out.append(y)
        recs.append(rec)
    return out, recs


def levels(record: dict) -> dict:
    """The residual imbalance a record's sums show, in ``ingest.adc_levels``' terms: ``gain_imbalance`` = sqrt(A / B) (I over
    Q), ``phase_error`` = asin(C / sqrt(A B)) in radians, and ``image_rejection_db``, what a single carrier's image would lie
    below it with that residue: 10 log10((1 + 2 g cos p + g^2) / (1 - 2 g cos p + g^2)).  None where A or B is not positive."""
    A, B, C = (float(v) for v in moments(record, record["n_complex"]))
    if not (A > 0 and B > 0):
        return {"gain_imbalance": None, "phase_error": None, "image_rejection_db": None}
    g = math.sqrt(A / B)
    p = math.asin(max(-1.0, min(1.0, C / math.sqrt(A * B))))
    num, den = 1 + 2 * g * math.cos(p) + g * g, 1 - 2 * g * math.cos(p) + g * g
    return {"gain_imbalance": g, "phase_error": p, "image_rejection_db": math.inf if den <= 0 else 10 * math.log10(num / den)}


def from_adc_levels(lv: dict) -> tuple[float, float]:
    """The (c0, d0) that the two figures of ``ingest.adc_levels`` imply -- with g = gain_imbalance (I over Q) and p =
    phase_error, Q = (Q0 cos p + I sin p) / g undone: c0 = -tan p, d0 = g / cos p -- clipped to what the library takes.  A helper
    to seed the loop: the caller decides."""
    g, p = float(lv["gain_imbalance"]), float(lv["phase_error"])
    c0, d0 = -math.tan(p), g / math.cos(p)
    return float(np.float32(min(MAX_C, max(-MAX_C, c0)))), float(np.float32(min(MAX_D, max(MIN_D, d0))))


def record_dict(r) -> dict:
    """struct sdrx_iq_record as a dict of Python integers"""
    return {k: int(getattr(r, k)) for k in RECORD_FIELDS}


def cfg_of(c) -> Cfg:
    """struct sdrx_iq_cfg as a Cfg"""
    return Cfg(float(c.mu), float(c.min_power), float(c.c0), float(c.d0), int(c.flags))
