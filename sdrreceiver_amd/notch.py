"""The spur canceller of include/sdrx.h ("Spur canceller") in numpy: the model the device is held to bit for bit.

Up to eight tones are removed from the tree's raw frame.  Each is a complex amplitude ``a`` times the frequency shift's table
oscillator (``shift.rotation``).  The frame is cut into blocks of ``L = 4096`` samples; every block is correlated with every
tone's oscillator (:func:`correlate`: fp32 sums in one fixed order), a one-pole loop in double smooths the block estimates and hands
each block the amplitude it held in front of that block (:func:`step`), which is subtracted (:func:`subtract`).  Once a frame the
tone's increment moves by the rotation between consecutive block estimates, if they are coherent.  :func:`apply` is one frame,
:class:`State` what frames hand on, :func:`run` a sequence of frames.  Integers, single fp32 operations and single double operations
do everything: there is no tolerance anywhere."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import shift as sh

MAX = 8                # SDRX_NOTCH_MAX
LOAD = 1               # SDRX_NOTCH_LOAD
L = sh.WORKGROUP       # samples per block: one workgroup of k_shift's geometry
LANE = sh.LANE
SPACING = 1 << 23      # 8 2^32 / L: the least circular distance of two tones' inc0
RAD_TO_INC = 166886.05360752725  # 2^20 / (2 pi) = 2^32 / (2 pi L): one radian of rotation per block, in inc units
M32 = sh.M32
NAN_BITS = sh.NAN_BITS
STATE_BYTES, RECORD_BYTES, TABLE_BYTES = 32 * MAX, 544, sh.TABLE_BYTES
TONE_FIELDS = ("inc", "inc_next", "a_re_bits", "a_im_bits", "coherent", "adapted", "clamped", "rejected", "s_re", "s_im", "p", "e")
F32 = np.float32


def device_bytes(n: int, shift_on: bool = False) -> int:
    """What the stage holds on the device for tree frames of n samples: the eight slots, c and used of one frame's blocks (8 bytes a
    block and a slot each), two records, and the tables unless the shift's copy serves"""
    return STATE_BYTES + 2 * blocks(n) * MAX * 8 + 2 * RECORD_BYTES + (0 if shift_on else TABLE_BYTES)


@dataclasses.dataclass(frozen=True)
class Cfg:
    inc0: tuple
    mu: float
    afc_gain: float
    min_coherence: float
    max_pull: int
    flags: int = 0

    @property
    def n_tones(self) -> int:
        return len(self.inc0)


@dataclasses.dataclass(frozen=True)
class Tone:
    """A slot's state: (0, inc0, 0) after sdrx_finalize"""
    phase: int
    inc: int
    inc0: int
    a_re: np.float32 = F32(0)
    a_im: np.float32 = F32(0)

    @staticmethod
    def start(inc0: int) -> "Tone":
        return Tone(0, int(inc0) & M32, int(inc0) & M32)


@dataclasses.dataclass(frozen=True)
class State:
    tones: tuple = ()
    frame: int = 0

    @staticmethod
    def initial(cfg: Cfg) -> "State":
        return State(tuple(Tone.start(v) for v in cfg.inc0), 0)


def distance(a: int, b: int) -> int:
    """Circular distance of two increments"""
    d = (int(a) - int(b)) & M32
    return min(d, (1 << 32) - d) if d else 0


def check_cfg(cfg: Cfg) -> str | None:
    """None, or why the library refuses these settings (SDRX_EINVAL)"""
    if not 0 <= len(cfg.inc0) <= MAX:
        return "n_tones must lie in 0 .. 8"
    if any(not 0 <= int(v) <= M32 for v in cfg.inc0) or not 0 <= int(cfg.max_pull) <= M32:
        return "inc0 and max_pull are 32-bit words"
    mu, g, c = F32(cfg.mu), F32(cfg.afc_gain), F32(cfg.min_coherence)
    if not (mu > 0 and mu <= 1):
        return "mu must lie in (0, 1]"
    if not (g >= 0 and g <= 1):
        return "afc_gain must lie in [0, 1]"
    if not (c > 0 and c <= 1):
        return "min_coherence must lie in (0, 1]"
    if int(cfg.flags) & ~LOAD:
        return "flags: only bit 0 is defined"
    for i in range(len(cfg.inc0)):
        for j in range(i + 1, len(cfg.inc0)):
            if distance(cfg.inc0[i], cfg.inc0[j]) < SPACING:
                return "two tones are closer than 2^23 increment units"
    return None


def blocks(n: int) -> int:
    return -(-int(n) // L)


def block_len(n: int, b: int) -> int:
    return min(L, n - b * L)


def correlate(x, phase: int, inc: int) -> np.ndarray:
    """c[b] of one tone, complex64: t = x (x) conj(rot); lane sums of 16 in ascending order from +0; the wave tree at distance 1, 2,
    .., 32; the four waves as (w0 + w1) + (w2 + w3)"""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    n, nb = x.size, blocks(x.size)
    t = np.zeros(nb * L, np.complex64)  # (lanes behind the frame's end carry +0; a sum that starts from +0 never is -0)
    t[:n] = sh.cmul(x, np.conj(sh.rotation(sh.phases(phase, inc, n))))
    out = np.empty(nb, np.complex64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for part in ("real", "imag"):
            v = np.ascontiguousarray(getattr(t, part), dtype=F32).reshape(nb, L // LANE, LANE)
            s = np.zeros((nb, L // LANE), F32)
            for j in range(LANE):
                s = s + v[:, :, j]
            w = s.reshape(nb, 4, 64).copy()
            d = 1
            while d < 64:
                w[:, :, 0::2 * d] = w[:, :, 0::2 * d] + w[:, :, d::2 * d]
                d *= 2
            w = w[:, :, 0]
            setattr(out, part, (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3]))
    return out


def step(c, n: int, tone: Tone, cfg: Cfg) -> tuple[np.ndarray, dict, Tone]:
    """One tone over a frame's block correlations c: (used[b] complex64, the tone's part of the record, the slot's next state).
    Python floats are IEEE doubles: every operation below is one double operation."""
    nb, nfull = blocks(n), n // L
    mu, afc, coh = float(F32(cfg.mu)), float(F32(cfg.afc_gain)), float(F32(cfg.min_coherence))
    ar, ai = F32(tone.a_re), F32(tone.a_im)
    used = np.empty(nb, np.complex64)
    s_re = s_im = p = e = 0.0
    pr = pi = 0.0
    rejected = 0
    cr, ci = np.ascontiguousarray(c.real, dtype=F32), np.ascontiguousarray(c.imag, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(nb):
            lb = float(block_len(n, b))
            mr, mi = float(cr[b]) / lb, float(ci[b]) / lb
            used[b] = complex(ar, ai)
            if 1 <= b < nfull:
                s_re = s_re + (mr * pr + mi * pi)
                s_im = s_im + (mi * pr - mr * pi)
                p = p + (mr * mr + mi * mi)
                dr, di = mr - float(ar), mi - float(ai)
                e = e + (dr * dr + di * di)
            pr, pi = mr, mi
            nr = F32(float(ar) + mu * (mr - float(ar)))
            ni = F32(float(ai) + mu * (mi - float(ai)))
            if not (np.isfinite(nr) and np.isfinite(ni)):
                nr, ni = F32(0), F32(0)
                rejected += 1
            ar, ai = nr, ni
    inc = tone.inc
    inc_next, coherent, adapted, clamped = inc, 0, 0, 0
    if nfull >= 2:
        coherent = int(s_re > 0.0 and s_re >= coh * p)
        if coherent and afc > 0.0:
            r = s_im / s_re
            r = 1.0 if r > 1.0 else r
            r = r if r >= -1.0 else -1.0  # (a NaN is -1)
            d = int(np.rint((afc * r) * RAD_TO_INC))
            inc_next, adapted = (inc + d) & M32, 1
            off = (inc_next - tone.inc0) & M32
            off = off - (1 << 32) if off >= 1 << 31 else off
            if off > int(cfg.max_pull):
                inc_next, clamped = (tone.inc0 + int(cfg.max_pull)) & M32, 1
            elif off < -int(cfg.max_pull):
                inc_next, clamped = (tone.inc0 - int(cfg.max_pull)) & M32, 1
    bits = np.array([ar, ai], F32).view(np.uint32)
    rec = {"inc": inc, "inc_next": inc_next, "a_re_bits": int(bits[0]), "a_im_bits": int(bits[1]), "coherent": coherent, "adapted": adapted,
           "clamped": clamped, "rejected": rejected, "s_re": s_re, "s_im": s_im, "p": p, "e": e}
    return used, rec, Tone((tone.phase + n * inc) & M32, inc_next, tone.inc0, ar, ai)


def subtract(y, used, phase: int, inc: int) -> np.ndarray:
    """y <- fl(y - (used[b] (x) rot)) per component, in place on the complex64 frame y"""
    n = y.size
    q = sh.cmul(np.repeat(used, L)[:n], sh.rotation(sh.phases(phase, inc, n)))
    with np.errstate(over="ignore", invalid="ignore"):
        y.real = np.ascontiguousarray(y.real) - np.ascontiguousarray(q.real)
        y.imag = np.ascontiguousarray(y.imag) - np.ascontiguousarray(q.imag)
    return y


def apply(x, cfg: Cfg, state: State) -> tuple[np.ndarray, dict, State]:
    """One frame: (the notched frame, its record, the state for the next frame)"""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    n = x.size
    assert len(state.tones) == cfg.n_tones
    y = x.copy()
    tones, recs = [], []
    for tone in state.tones:  # (k ascending)
        used, rec, nxt = step(correlate(x, tone.phase, tone.inc), n, tone, cfg)
        subtract(y, used, tone.phase, tone.inc)
        tones.append(nxt)
        recs.append(rec)
    u = y.view(np.uint32)
    u[np.isnan(y.view(F32))] = NAN_BITS
    zero = dict.fromkeys(TONE_FIELDS[:8], 0) | dict.fromkeys(TONE_FIELDS[8:], 0.0)
    rec = {"frame": state.frame, "n_complex": n, "n_tones": cfg.n_tones, "blocks": blocks(n), "tones": recs + [dict(zero) for _ in range(MAX - len(recs))]}
    return y, rec, State(tuple(tones), state.frame + 1)


def load(state: State, before: Cfg, after: Cfg) -> State:
    """sdrx_set_notch between two frames: a slot whose inc0 is unchanged keeps phase, inc and a; a changed or new slot starts at
    (0, inc0, 0); LOAD restarts every slot"""
    tones = []
    for k, v in enumerate(after.inc0):
        keep = not (after.flags & LOAD) and k < before.n_tones and int(before.inc0[k]) == int(v)
        tones.append(state.tones[k] if keep else Tone.start(v))
    return State(tuple(tones), state.frame)


def run(frames, cfg) -> tuple[list[np.ndarray], list[dict]]:
    """A sequence of frames from the state after sdrx_finalize; `cfg`: one Cfg, or one per frame (a later one that is another
    object than its predecessor is set in front of its frame, as sdrx_set_notch does)"""
    cur = cfg if isinstance(cfg, Cfg) else cfg[0]
    state, out, recs = State.initial(cur), [], []
    for f, x in enumerate(frames):
        if f and not isinstance(cfg, Cfg) and cfg[f] is not cfg[f - 1]:
            state, cur = load(state, cur, cfg[f]), cfg[f]
        y, rec, state = apply(x, cur, state)
        out.append(y)
        recs.append(rec)
    return out, recs


def reference(frames, cfg: Cfg) -> tuple[list[np.ndarray], list[dict]]:
    """The same rule evaluated in double throughout (exact oscillator, double sums): what the fp32 model approximates.  For accuracy
    figures only."""
    K = cfg.n_tones
    phase = [0.0] * K  # turns
    inc = [float(v if v < 1 << 31 else v - (1 << 32)) for v in cfg.inc0]
    inc0 = list(inc)
    a = [0j] * K
    out, recs = [], []
    for x in frames:
        x = np.asarray(x, dtype=np.complex128).reshape(-1)
        n, nb, nfull = x.size, blocks(x.size), x.size // L
        y = x.copy()
        j = np.arange(n, dtype=np.float64)
        rec = []
        for k in range(K):
            rot = np.exp(2j * np.pi * ((phase[k] + j * inc[k] / 4294967296.0) % 1.0))
            t = x * np.conj(rot)
            m = np.array([t[b * L: b * L + block_len(n, b)].mean() for b in range(nb)])
            used = np.empty(nb, np.complex128)
            for b in range(nb):
                used[b] = a[k]
                a[k] = a[k] + cfg.mu * (m[b] - a[k])
            y -= np.repeat(used, L)[:n] * rot
            nxt = inc[k]
            s, p, e = 0j, 0.0, 0.0
            if nfull >= 2:
                s = np.sum(m[1:nfull] * np.conj(m[0:nfull - 1]))
                p = float(np.sum(np.abs(m[1:nfull]) ** 2))
                e = float(np.sum(np.abs(m[1:nfull] - used[1:nfull]) ** 2))
                if s.real > 0 and s.real >= cfg.min_coherence * p and cfg.afc_gain > 0:
                    d = float(np.rint(cfg.afc_gain * min(1.0, max(-1.0, s.imag / s.real)) * RAD_TO_INC))
                    nxt = min(inc0[k] + cfg.max_pull, max(inc0[k] - cfg.max_pull, inc[k] + d))
            rec.append({"inc": inc[k], "inc_next": nxt, "a": a[k], "s_re": float(np.real(s)), "s_im": float(np.imag(s)), "p": p, "e": e})
            phase[k] = (phase[k] + n * inc[k] / 4294967296.0) % 1.0
            inc[k] = nxt
        out.append(y)
        recs.append(rec)
    return out, recs


def _key(v):
    return "nan" if isinstance(v, float) and math.isnan(v) else v.hex() if isinstance(v, float) else v


def record_key(rec: dict) -> tuple:
    """A record as a tuple that compares bit for bit (doubles by their hex; every NaN alike)"""
    return (rec["frame"], rec["n_complex"], rec["n_tones"], rec["blocks"], tuple(tuple(_key(t[f]) for f in TONE_FIELDS) for t in rec["tones"]))


def record_dict(r) -> dict:
    """struct sdrx_notch_record as a dict of Python numbers"""
    return {"frame": int(r.frame), "n_complex": int(r.n_complex), "n_tones": int(r.n_tones), "blocks": int(r.blocks),
            "tones": [{f: (float if f in TONE_FIELDS[8:] else int)(getattr(r.tone[k], f)) for f in TONE_FIELDS} for k in range(MAX)]}


def cfg_of(c) -> Cfg:
    """struct sdrx_notch_cfg as a Cfg"""
    return Cfg(tuple(int(c.inc0[k]) for k in range(int(c.n_tones))), float(c.mu), float(c.afc_gain), float(c.min_coherence), int(c.max_pull), int(c.flags))


def levels(record: dict, fs: float) -> list[dict]:
    """Per tone of a record: the tracked frequency in Hz at the tree's rate `fs` (of inc_next), the amplitude |a|, the coherence
    S_re / P of the block estimates, the depth figure P / E (how much of the tone's power the estimate caught; power ratio) and the
    lock flags"""
    out = []
    for t in record["tones"][:record["n_tones"]]:
        a = np.array([t["a_re_bits"], t["a_im_bits"]], np.uint32).view(F32)
        out.append({"hz": sh.hz_of(fs, t["inc_next"]), "amplitude": float(np.hypot(np.float64(a[0]), np.float64(a[1]))),
                    "coherence": t["s_re"] / t["p"] if t["p"] > 0 else 0.0, "depth": t["p"] / t["e"] if t["e"] > 0 else math.inf if t["p"] > 0 else 0.0,
                    "locked": bool(t["coherent"]) and not t["clamped"] and not t["rejected"], "coherent": bool(t["coherent"]),
                    "adapted": bool(t["adapted"]), "clamped": bool(t["clamped"]), "rejected": int(t["rejected"])})
    return out
