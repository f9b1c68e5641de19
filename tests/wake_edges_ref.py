"""The wake rule at its thresholds (include/sdrx.h "Device-side wake": `>=`, IEEE double, the 64-bit product contrast_q8 * n,
the clause n < N, hold_left up to 2^32 - 1 and its restart by sdrx_set_wake) for tests/test_gpu_wake_edges.py; no GPU.

The rule's inputs are device results -- a leaf's watch record -- and cannot be crafted from the input bytes.  They are
reproducible, though: a leaf's source depends on no leaf (wake_ref.sources) and the watch sums have no data-dependent order.
So a first receiver without the wake (pass A) measures every (frame, leaf), a *plan builder* here turns those figures into
settings that put chosen decisions exactly on a threshold or one step off it, and a second receiver (pass B) runs under them.
A :class:`Plan` is a wake_ref.Scenario (the settings before frame 0), the settings of later frames in wake_ref.decide's form and
the :class:`Crafted` decisions with the condition each one stands on, which pass B asserts on its OWN record
(:func:`holds`).  tests/test_wake_edges_model.py runs the same builders on the model's figures (wake_ref.figures) and shows that
every wrong rule of :data:`WRONG_RULES` would give another record somewhere.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

import wake_ref as kr
from lattice import _Build
from sdrreceiver_amd import wake

U32 = 2 ** 32 - 1
N = wake.BINS
HOLD_LONG = 100  # outlasts every scenario: hold_left in a fetched frame then tells the last hot frame before it


# ---- the bracket ------------------------------------------------------------------------------------------------------------------
def c_ok(q8: int, b, t, n, step=wake.step) -> bool:
    """Does `step` pass the contrast condition with contrast_q8 = q8?  (min_band_pwr 0: hot is c_ok for every b >= 0)"""
    return step(wake.Cfg(0.0, int(q8), 0), 0, b, t, n)[1] == 1


def bracket_q8(b, t, n, step=wake.step):
    """The largest q8 in [1, 2^32 - 1] that `step` (wake.step) passes, by bisection on the rule itself -- it is monotone in q8
    when t - b > 0; None when there is no bracket: q8 = 1 is cold, or q8 = 2^32 - 1 is hot."""
    if not c_ok(1, b, t, n, step) or c_ok(U32, b, t, n, step):
        return None
    lo, hi = 1, U32  # lo passes, hi does not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if c_ok(mid, b, t, n, step):
            lo = mid
        else:
            hi = mid
    return lo


# ---- the wrong rules --------------------------------------------------------------------------------------------------------------
def _rule(cfg, hold_left, band_pwr, total_pwr, n_bins, gt=False, f32=False, mul32=False, n_lt_N=True, wrap=False):
    """wake.step with one defect switched on"""
    fl = np.float32 if f32 else np.float64
    b, t = np.float64(band_pwr), np.float64(total_pwr)
    n, q = int(n_bins), int(cfg.contrast_q8)
    ok = q == 0
    if not ok and (n < N or not n_lt_N):
        qn = (q * n) & U32 if mul32 else q * n
        with np.errstate(all="ignore"):
            lhs = fl(fl(b) * fl(256 * (N - n)))
            rhs = fl(fl(fl(t) - fl(b)) * fl(qn))
        ok = bool(lhs >= rhs)
    thr = np.float64(cfg.min_band_pwr)
    hot = bool(b > thr if gt else b >= thr) and ok
    if hot:
        return 1, 1, int(cfg.hold_frames)
    if wrap:  # `if (hold_left-- > 0)`: the word is decremented at 0 too
        return (1 if hold_left > 0 else 0), 0, (int(hold_left) - 1) & U32
    if hold_left > 0:
        return 1, 0, int(hold_left) - 1
    return 0, 0, 0


def _wrong(**kw):
    return lambda cfg, hold_left, b, t, n: _rule(cfg, hold_left, b, t, n, **kw)


# name -> (stepper with wake.step's signature, wake_ref.decide's reset_hold)
WRONG_RULES = {
    "gt": (_wrong(gt=True), True),                # the band power compared with >
    "f32": (_wrong(f32=True), True),              # every operand and product of the contrast rounded to float32
    "mul32": (_wrong(mul32=True), True),          # contrast_q8 * n taken mod 2^32
    "no_n_lt_N": (_wrong(n_lt_N=False), True),    # the contrast evaluated when n == N
    "hold_wrap": (_wrong(wrap=True), True),       # hold_left decremented at 0, as uint32
    "no_hold_reset": (wake.step, False),          # sdrx_set_wake leaves hold_left standing
}


def decide(plan, figs, wrong=None) -> list:
    """wake_ref.decide for `plan` on `figs`, under the rule or one of WRONG_RULES"""
    stepper, reset = WRONG_RULES[wrong] if wrong else (wake.step, True)
    return kr.decide(plan.scn, figs, stepper, plan.cfgs, reset_hold=reset)


# ---- plans ------------------------------------------------------------------------------------------------------------------------
EQ, ABOVE = "band_pwr == min_band_pwr", "nextafter(band_pwr, +inf) == min_band_pwr"
BR, BR1 = "contrast_q8 == bracket_q8", "contrast_q8 == bracket_q8 + 1"
PROD, FULL, ZERO, PLAIN = "contrast_q8 * n_bins >= 2^32", "n_bins == N", "min_band_pwr == 0", "away from every threshold"


@dataclasses.dataclass(frozen=True)
class Crafted:
    frame: int
    leaf: int
    cond: str
    hot: bool


@dataclasses.dataclass(frozen=True)
class Plan:
    key: str
    scn: kr.Scenario   # cfgs: the settings before frame 0, every leaf of the plan among them
    cfgs: dict         # frame -> {leaf: Cfg}, wake_ref.decide's form
    crafted: tuple
    fetch_at: tuple    # queued sdrx_process_device: the frames fetched (each frame before a later setting among them)


def holds(cond: str, cfg, b, t, n) -> bool:
    """Does the condition a crafted decision stands on hold for the record (b, t, n) under `cfg`?  Doubles compared as such."""
    if cond == EQ:
        return np.float64(b) == np.float64(cfg.min_band_pwr) and cfg.contrast_q8 == 0
    if cond == ABOVE:
        return math.nextafter(float(b), math.inf) == float(cfg.min_band_pwr) and cfg.contrast_q8 == 0
    if cond in (BR, BR1):
        q = bracket_q8(b, t, n)
        return q is not None and cfg.contrast_q8 == q + (cond == BR1) and cfg.min_band_pwr == 0.0
    if cond == PROD:
        return cfg.contrast_q8 * int(n) >= 2 ** 32
    if cond == FULL:
        return int(n) == N
    if cond == ZERO:
        return cfg.min_band_pwr == 0.0 and cfg.contrast_q8 == 0
    assert cond == PLAIN, cond
    return True


def cfg_at(cfgs: dict, frame: int, leaf: int):
    """the setting of `leaf` in force in `frame`"""
    return next(cfgs[f][leaf] for f in sorted(cfgs, reverse=True) if f <= frame and leaf in cfgs[f])


def bits(row: dict) -> tuple:
    """a row of figures {leaf: (band_pwr, total_pwr, n_bins)} as bit patterns"""
    return tuple((i, float(b).hex(), float(t).hex(), int(n)) for i, (b, t, n) in sorted(row.items()))


# Where the settings change (the frames before it and from it on are the two halves a leaf's two crafted decisions come from),
# the frames a queued run fetches, and the leaves: a level-1, a level-2 and the parent-less leaf of "deep" (sources: the main's
# stream, the inner node's, the raw frame), USB, fused /5 and compress leaves of "watch".
# ("watch" has a contrast of 1/256 and more for every leaf only in its quiet frames 6 and 8 and a leaf's own tone frames: the
# contrast plan splits it behind frame 6.)
SPLIT = {"deep": 4, "watch": 5}
CONTRAST_SPLIT = {"deep": 4, "watch": 7}
FETCH = {"deep": (1, 3, 5, 7), "watch": (2, 4, 6, 8)}
BAND_LEAVES = {"deep": (4, 2, 5, 3, 6), "watch": (1, 3, 9, 6)}
# (leaf, "tone" | "quiet"): the frame of a half with the largest bracket, or the one whose bracket is nearest 256 (contrast 1)
CONTRAST_LEAVES = {"deep": ((4, "tone"), (2, "tone"), (5, "tone"), (3, "quiet"), (6, "quiet")),
                   "watch": ((3, "tone"), (1, "tone"), (2, "quiet"), (9, "tone"), (6, "quiet"))}


def _plan(key, name, cfgs, crafted, fetch_at, parked0=None):
    base = kr.scenario(name)
    scn = dataclasses.replace(base, cfgs=dict(cfgs[0]), parked0=base.parked0 if parked0 is None else tuple(parked0))
    assert all(set(c) <= set(cfgs[0]) for c in cfgs.values()), "every leaf of a plan is set before frame 0"
    return Plan(key, scn, cfgs, tuple(crafted), tuple(fetch_at))


def _halves(name, split=SPLIT):
    K, n = split[name], len(kr.scenario(name).frames)
    return K, (range(0, K), range(K, n))


def plan_band(name: str, figs, hold: int = 0) -> Plan:
    """Case 1.  contrast_q8 = 0.  Leaf k of BAND_LEAVES: in one half min_band_pwr is its band_pwr of a frame, exactly -- hot --,
    in the other the next double above its band_pwr of a frame -- cold; even k: hot first.  The frame is the one with the
    largest band_pwr among the half's frames of one parity (that of k / 2 in the first half, the other in the second)."""
    K, halves = _halves(name)
    cfgs, crafted = {0: {}, K: {}}, []
    for k, i in enumerate(BAND_LEAVES[name]):
        for h, fr in enumerate(halves):
            f = max((f for f in fr if (f ^ (k >> 1) ^ h) & 1 == 0), key=lambda f: figs[f][i][0])
            b = float(figs[f][i][0])
            eq = (k + h) % 2 == 0
            cfgs[h * K][i] = wake.Cfg(b if eq else math.nextafter(b, math.inf), 0, hold)
            crafted.append(Crafted(f, i, EQ if eq else ABOVE, eq))
    return _plan(f"band-{name}-{hold}", name, cfgs, crafted, FETCH[name])


def plan_contrast(name: str, figs, hold: int = 0) -> Plan:
    """Case 2.  min_band_pwr = 0.  Leaf k of CONTRAST_LEAVES: in one half contrast_q8 is bracket_q8 of a frame -- hot --, in the
    other bracket_q8 of a frame, plus 1 -- cold; even k: hot first.  A decision whose product contrast_q8 * n_bins does not fit
    32 bits is listed once more, with PROD."""
    K, halves = _halves(name, CONTRAST_SPLIT)
    cfgs, crafted = {0: {}, K: {}}, []
    for k, (i, kind) in enumerate(CONTRAST_LEAVES[name]):
        for h, fr in enumerate(halves):
            br = {f: bracket_q8(*figs[f][i]) for f in fr}
            br = {f: q for f, q in br.items() if q is not None and q < U32 - 1}
            assert br, (name, i, h, "no frame of this half has a bracket")
            f = max(br, key=br.get) if kind == "tone" else min(br, key=lambda f: abs(math.log(br[f] / 256.0)))
            ok = (k + h) % 2 == 0
            c = wake.Cfg(0.0, br[f] + (0 if ok else 1), hold)
            cfgs[h * K][i] = c
            crafted.append(Crafted(f, i, BR if ok else BR1, ok))
            if c.contrast_q8 * int(figs[f][i][2]) >= 2 ** 32:
                crafted.append(Crafted(f, i, PROD, ok))
    return _plan(f"contrast-{name}-{hold}", name, cfgs, crafted, FETCH[name])


def plan_always(figs=None) -> Plan:
    """Case 4.  min_band_pwr = 0 and no contrast on every leaf of "flat": hot in every frame, the quiet frame 5 included.  The
    leaves parked before frame 0 wake in it; none is parked again."""
    base = kr.scenario("flat")
    cfgs = {0: {i: wake.Cfg(0.0, 0, 0) for i in base.controlled}}
    crafted = [Crafted(f, i, ZERO, True) for f in range(len(base.frames)) for i in base.controlled]
    return _plan("always-flat", "flat", cfgs, crafted, (1, 3, 4, 6))


# Case 5 on "deep", thresholds a factor 4 and more from every figure (wake_ref.DEEP_MIN).  A tone raises the band of its own
# leaf and of the leaves whose bands hold it too; tests/test_wake_edges_model.py asserts what follows on the model's figures:
#   leaf 5: hold_frames 2^32 - 1 -- hot in frames 0-2 and 6: the records read 2^32 - 1, then 2^32 - 2, - 3, - 4, and 2^32 - 1 again;
#   leaf 4: hold_frames 0 -- cold with hold_left 0 in frames 0 and 1 (parked, and the word stays 0), hot in 2, parked at once in 3;
#   leaf 2: hold_frames 5, hot until frame 2, held in 3 and 4; named with unchanged settings before frame 5: parked in 5 (and
#           hot again in 6);
#   leaf 3: hold_frames 5, hot in 2 and 4, held from 5 on -- through the batches before 5 and 7, which name other leaves;
#   leaf 6: hold_frames 5, hot in 2, 4 and 5, held in 6; named before 7: parked in 7.
HOLD_RESET = {5: (2,), 7: (6,)}
HOLD_FRAMES = {5: U32, 4: 0, 2: 5, 3: 5, 6: 5}


def plan_hold(figs) -> Plan:
    first = {i: wake.Cfg(kr.DEEP_MIN[i], 0, h) for i, h in HOLD_FRAMES.items()}
    cfgs = {0: first}
    for f, ids in HOLD_RESET.items():
        cfgs[f] = {i: first[i] for i in ids}
    crafted = [Crafted(f, i, PLAIN, bool(row[i][0] >= first[i].min_band_pwr)) for f, row in enumerate(figs) for i in sorted(first)]
    return _plan("hold-deep", "deep", cfgs, crafted, (1, 4, 6, 7))


# ---- case 3: a leaf whose band is the whole spectrum ----------------------------------------------------------------------------------
# None of watch_tree, deep_tree and flat_tree has an IQ leaf without half-band stages (their IQ leaves have 2 or 3).  Node 0: the
# main (d = 1 on 4 800 samples); 1: an IQ leaf with d = 0 -- its band is its source's whole rate: n_bins 8192 --; 2: a USB leaf
# beside it, hot in frame 2 alone.
FULL_LEAF, FULL_USB = 1, 2


def full_tree():
    b = _Build("wake-full-band", 4800)
    m = b.inner(-1, 1)
    b.iq(m, 0, 1, 3)
    b.usb(m, 2)
    for d in b.t.vfos:
        if d.demod_usb:
            d.gain = float(np.float32(0.004))
    return b.t


def _full_scenario():
    topo = full_tree()
    bursts = ((FULL_LEAF, 1, 2), (FULL_USB, 2, 3))
    cfgs = {FULL_LEAF: wake.Cfg(0.0, 1, 0), FULL_USB: wake.Cfg(kr.FLAT_MIN, 0, 0)}
    return kr.Scenario("full", topo, tuple(kr.burst_frames(topo, 4, bursts)), cfgs, (), bursts)


kr.register("full", _full_scenario)


def plan_full(figs=None, contrast_q8: int = 1) -> Plan:
    """Case 3.  contrast_q8 = 1 asks for next to nothing, and with n == N the leaf is never hot: parked in every frame.  With
    contrast_q8 = 0 the same leaf is hot in every frame and runs throughout, as in a run without the option."""
    base = kr.scenario("full")
    cfgs = {0: {**base.cfgs, FULL_LEAF: wake.Cfg(0.0, contrast_q8, 0)}}
    crafted = [Crafted(f, FULL_LEAF, FULL, contrast_q8 == 0) for f in range(len(base.frames))]
    return _plan(f"full-{contrast_q8}", "full", cfgs, crafted, (1, 3))


def model_figs(plan: Plan) -> tuple:
    """the model's figures (wake_ref.figures) for the leaves of `plan`"""
    return tuple({i: row[i] for i in plan.scn.controlled} for row in kr.figures(plan.scn.name))
