"""Model of the device-side wake (option "wake", include/sdrx.h "Device-side wake") for the tests; no GPU.  The reference has no
counterpart, so this is the yardstick, and it needs nothing new below it:

* a wake before frame f is live_ref.ModelTree.apply([("unpark", [leaf])]) before f -- a fresh retune_ref.Node --, a park is
  ("park", ..);
* the decisions come from sdrreceiver_amd.wake.step on watch_ref.psd / watch_ref.levels of the model's source streams.  A
  leaf's source does not depend on any leaf, so they are computed ahead of the frames (:func:`decide`).

:class:`Scenario` is a tree, its frames (quiet frames of +-1 LSB noise and tone bursts placed through every ancestor's mixer,
:func:`tone_for`), the settings per controlled leaf and the leaves parked before frame 0.  :func:`scenario` builds the three of
the tests -- watch_ref.watch_tree(), catchup_ref.deep_tree(), catchup_ref.flat_tree() --, :func:`reference` runs the model once
per scenario (shared: nobody writes into it), :func:`run` runs it with one of the wrong devices of :data:`WRONG`.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import catchup_ref as cu
import live_ref
import retune_ref as rr
import watch_ref as wr
from sdrreceiver_amd import wake

AMP = 50.0          # tone amplitude (watch_ref.tone_frame's)
MARGIN = 4.0        # no decision closer than this factor to a threshold


def tone_for(topo, leaf: int, at: float = 0.5) -> float:
    """The raw frequency that lands at fraction `at` of the passband of `leaf`: its place in its source's stream, less the
    mixer of every ancestor (a component at g in a node's input is at g + f in its output)."""
    lo, hi = wr.band_hz(topo.vfos[leaf])
    hz = lo + at * (hi - lo)
    i = topo.vfos[leaf].parent
    while i >= 0:
        hz -= topo.vfos[i].mixer_freq
        i = topo.vfos[i].parent
    return hz


def burst_frames(topo, n_frames: int, bursts, seed: int = 5) -> list:
    """`bursts`: (leaf, first, end) in frames, fractions allowed -- a tone of amplitude 50 mid-passband of `leaf` over the
    samples [first * n, end * n), phase-continuous; every frame carries +-1 LSB of noise.  Interleaved float32 per frame."""
    n = topo.frame
    rng = np.random.default_rng(seed)
    out = []
    for f in range(n_frames):
        k = np.arange(f * n, (f + 1) * n, dtype=np.float64)
        z = np.zeros(n, np.complex128)
        for leaf, first, end in bursts:
            on = (k >= first * n) & (k < end * n)
            if on.any():
                z += on * AMP * np.exp(2j * np.pi * tone_for(topo, leaf) * k / topo.fs)
        iq = np.empty(2 * n, np.float32)
        iq[0::2] = np.round(z.real)
        iq[1::2] = np.round(z.imag)
        out.append(iq + rng.integers(-1, 2, 2 * n).astype(np.float32))
    return out


@dataclasses.dataclass(frozen=True)
class Scenario:
    name: str
    topo: object
    frames: tuple           # interleaved float32 per frame
    cfgs: dict              # controlled leaf -> wake.Cfg, set before frame 0
    parked0: tuple          # leaves parked (sdrx_set_active) before frame 0, before they come under control
    bursts: tuple

    @property
    def controlled(self):
        return sorted(self.cfgs)


# ---- the three scenarios ----------------------------------------------------------------------------------------------------------
# watch_tree: the thresholds of the issue's table -- min_band_pwr 1e8 with contrast 100 (q8 25 600) -- for the leaves that are hot
# alone; the two leaves that are hot in ONE frame (6, the /5 leaf, and 9, the compress leaf) have no contrast condition: each
# one's band is the other's "outside".
#   leaf 1: parked before frame 0, tone in 0 and 1 (a wake in frame 0), cold from 2 (parks), tone again in 5: wakes with the
#           state of frame 1 behind it (stale state), cold in 6;
#   leaf 3: parked before frame 0, hold 1: a burst that begins mid-frame 2 and ends mid-frame 4 -> hot 2, 3, 4, held in 5, parked in 6;
#   leaf 2: controlled and never hot: active at the start, parked by frame 0;
#   leaves 6 and 9: active at the start, parked by frame 0, both hot in frame 7; 9 holds two frames, 6 parks in 8;
#   leaves 4, 5, 7, 8: not controlled -- they run in every frame.
def _watch_scenario():
    topo = wr.watch_tree()
    both = wake.Cfg(1e8, 25600, 0)
    cfgs = {1: both, 2: both, 3: wake.Cfg(1e8, 25600, 1), 6: wake.Cfg(1e8, 0, 0), 9: wake.Cfg(1e8, 0, 2)}
    bursts = ((1, 0, 2), (3, 2.5, 4.5), (1, 5, 6), (6, 7, 8), (9, 7, 8))
    return Scenario("watch", topo, tuple(burst_frames(topo, 9, bursts)), cfgs, (1, 3), bursts)


# deep_tree: the parent-less leaf 5 (source: the raw frame), the level-1 leaves 4 and 6 (the main's stream) and the level-2
# leaves 2 and 3 (the inner node's).  Every leaf is controlled and parked before frame 0.
def _deep_scenario():
    topo = cu.deep_tree()
    cfgs = {i: wake.Cfg(DEEP_MIN[i], 0, 1 if i == 2 else 0) for i in (2, 3, 4, 5, 6)}
    bursts = ((5, 0, 1), (2, 1, 3), (4, 2, 3), (3, 4, 5), (6, 4.5, 6), (5, 6, 7))
    return Scenario("deep", topo, tuple(burst_frames(topo, 8, bursts)), cfgs, (2, 3, 4, 5, 6), bursts)


# flat_tree: the leaf shapes -- fused /5 and /6, k_lpf_long, fuse_demod's shape, IQ cstyle 0 and 1.  Two whole-frame tones per
# frame, each mid-band of one leaf (whichever other bands hold one are hot with it); frame 5 is quiet; in frame 6 leaves 2 and 8
# (the long low-pass) are hot again, with the state of their first run behind them.  Every leaf is controlled; the odd ones are
# parked before frame 0.
def _flat_scenario():
    topo = cu.flat_tree()
    cfgs = {i: wake.Cfg(FLAT_MIN, 0, 0) for i in range(1, 11)}
    bursts = tuple((leaf, f, f + 1) for f in range(5) for leaf in (1 + f, 6 + f)) + ((2, 6, 7), (8, 6, 7))
    return Scenario("flat", topo, tuple(burst_frames(topo, 7, bursts)), cfgs, (1, 3, 5, 7, 9), bursts)


# Thresholds of the small trees (4 800-sample frames: one zero-padded segment of 4 800 raw or 2 400 decimated samples).  A
# tone of amplitude 50 over a whole source frame of n samples puts about (50 n / 2)^2 into its bin and its neighbours (the
# Hann window's coherent gain is 1/2): 1.4e10 raw, 3.6e9 on the 2 400-sample streams, and a burst that covers a tenth of the
# frame still a hundredth of that; +-1 LSB of noise is about n * (4/3) * (3/8) = n / 2 per bin, below 1.3e6 over the widest
# band.  test_wake_model.py asserts the margin of every scheduled decision against these.
DEEP_MIN = {2: 3e7, 3: 3e7, 4: 3e7, 6: 3e7, 5: 1e8}
FLAT_MIN = 3e7

_BUILD = {"watch": _watch_scenario, "deep": _deep_scenario, "flat": _flat_scenario}


def register(name: str, build) -> None:
    """Another scenario under `name` (tests/wake_edges_ref.py's): :func:`scenario`, :func:`sources` and :func:`figures` then
    serve it as they serve the three above, which stay what they are."""
    assert _BUILD.get(name, build) is build, name
    _BUILD[name] = build


@functools.lru_cache(maxsize=None)
def scenario(name: str) -> Scenario:
    return _BUILD[name]()


# ---- the decisions ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sources(name: str) -> tuple:
    """Per frame: node -> model stream of every node that has children (-1: the raw frame).  No leaf runs."""
    scn = scenario(name)
    model = live_ref.ModelTree(scn.topo)
    model.park(model.leaves)
    out = []
    for iq in scn.frames:
        s = model.process(iq)["streams"]
        s = {i: z for i, z in s.items() if z is not None}
        s[-1] = np.ascontiguousarray(iq, np.float32).view(np.complex64)
        out.append(s)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def figures(name: str, retunes: tuple = ()) -> tuple:
    """Per frame: controlled leaf -> (band_pwr, total_pwr, n_bins) of the model (watch_ref: exact sums).  `retunes`: (frame,
    leaf, mixer) -- the leaf's band from that frame on."""
    scn = scenario(name)
    descs = list(scn.topo.vfos)
    psd_of: dict = {}
    out = []
    for f, src in enumerate(sources(name)):
        for fr, leaf, hz in retunes:
            if fr == f:
                descs[leaf] = dataclasses.replace(descs[leaf], mixer_freq=float(hz))
        row = {}
        for i in scn.controlled:
            p = descs[i].parent
            if (f, p) not in psd_of:
                psd_of[(f, p)] = wr.psd(src[p])
            first, n = wr.band(descs[i])
            b, t = wr.levels(psd_of[(f, p)], first, n)
            row[i] = (b, t, n)
        out.append(row)
    return tuple(out)


def step_hold_decremented_when_hot(cfg, hold_left, band_pwr, total_pwr, n_bins):
    """A wrong device: hold_left counts down in hot frames too."""
    active, hot, left = wake.step(cfg, hold_left, band_pwr, total_pwr, n_bins)
    return (active, hot, max(left - 1, 0)) if hot else (active, hot, left)


def decide(scn: Scenario, figs, stepper=wake.step, cfgs=None, start=None, reset_hold=True) -> list:
    """Per frame: controlled leaf -> dict(frame, since_frame, active, hot, hold_left, controlled) -- the wake records.
    `cfgs`: frame -> {leaf: Cfg} set before that frame (default: scn.cfgs before frame 0); `start`: leaf -> (active, since);
    `reset_hold` False: a wrong device whose sdrx_set_wake leaves hold_left standing."""
    cfgs = {0: scn.cfgs} if cfgs is None else cfgs
    cur: dict = {}
    state = {i: [0 if i in scn.parked0 else 1, 0, 0] for i in scn.topo.leaves_in_publish_order()}  # active, since, hold_left
    if start:
        for i, (a, s) in start.items():
            state[i] = [a, s, 0]
    out = []
    for f, row in enumerate(figs):
        for i, c in cfgs.get(f, {}).items():
            if reset_hold:
                state[i][2] = 0
            if c.on:
                cur[i] = c
            else:
                cur.pop(i, None)
        recs = {}
        for i in sorted(cur):
            b, t, n = row[i]
            active, hot, left = stepper(cur[i], state[i][2], b, t, n)
            if active != state[i][0]:
                state[i][1] = f
            state[i][0], state[i][2] = active, left
            recs[i] = dict(frame=f, since_frame=state[i][1], active=active, hot=hot, hold_left=left, controlled=1)
        out.append(recs)
    return out


def margins(scn: Scenario, figs) -> list:
    """(frame, leaf, what, ratio) of every scheduled decision: band_pwr / min_band_pwr, and contrast / (contrast_q8 / 256)
    for the leaves with a contrast condition."""
    out = []
    for f, row in enumerate(figs):
        for i, (b, t, n) in row.items():
            c = scn.cfgs[i]
            out.append((f, i, "band_pwr", b / c.min_band_pwr))
            if c.contrast_q8:
                out.append((f, i, "contrast", wr.contrast(b, t, n) / (c.contrast_q8 / 256.0)))
    return out


# ---- the frames -------------------------------------------------------------------------------------------------------------------
WRONG = ("late", "no_zero", "origin", "prev_open", "hold_dec", "tail_early")


class Tree(live_ref.ModelTree):
    """live_ref.ModelTree whose unpark can be one of the wrong devices."""

    def __init__(self, topo, wrong=None):
        super().__init__(topo)
        self.wrong = wrong

    def unpark(self, ids):
        for i in ids:
            if self.active[i]:
                continue
            old = self.nodes[i]
            super().unpark([i])
            if self.wrong == "no_zero":    # a node that merely skipped its parked frames: its state stands, the oscillator is new
                old.retune(self.descs[i].mixer_freq)
                self.nodes[i] = old
            elif self.wrong == "origin":   # zero state, but the oscillator runs on from frame 0
                self.nodes[i].k = self.frame_no * self.descs[i].samples_per_buffer


def run(scn: Scenario, wrong: str | None = None, figs=None, cfgs=None, ops=None, start=None, tree_cls=None, stepper=None,
        reset_hold=True) -> list:
    """The frames of `scn` under the device-side wake: per frame live_ref.ModelTree.process's result plus "wake" (the records
    of :func:`decide`), "events" (leaf -> 'u' | 'p' of this frame: test_park_model.gate_with_parking's; the wrong device
    "prev_open" says 'c') and "descs".  `ops`: frame -> host calls before it (ModelTree.apply: retunes, gains); `tree_cls`:
    another model tree on top of :class:`Tree` (agc_ref.agc_tree(Tree): the AGC loop, whose "agc" calls `ops` may then hold);
    `stepper`, `reset_hold`: another rule in place of wake.step, :func:`decide`'s wrong sdrx_set_wake."""
    assert wrong is None or wrong in WRONG, wrong
    figs = figures(scn.name) if figs is None else figs
    if stepper is None:
        stepper = step_hold_decremented_when_hot if wrong == "hold_dec" else wake.step
    recs = decide(scn, figs, stepper, cfgs, start, reset_hold)
    model = Tree(scn.topo, wrong) if tree_cls is None else tree_cls(scn.topo)
    model.park([i for i in scn.parked0])
    if start:
        model.park([i for i, (a, _) in start.items() if not a])
    want = []
    for f, iq in enumerate(scn.frames):
        model.apply((ops or {}).get(f, []))
        use = recs[f - 1] if wrong == "late" and f > 0 else {} if wrong == "late" else recs[f]
        events = {}
        for i, r in use.items():
            if r["active"] and not model.active[i]:
                model.unpark([i])
                events[i] = "c" if wrong == "prev_open" else "u"
            elif not r["active"] and model.active[i]:
                model.park([i])
                events[i] = "p"
        w = model.process(iq)
        w["wake"] = recs[f]
        w["events"] = events
        w["descs"] = list(model.descs)
        want.append(w)
    if wrong == "tail_early":  # the tail of f-1 ran under the flags of f: what f-1 delivers is what f's decisions allow
        for f in range(len(want) - 1):
            nxt = want[f + 1]["active"]
            want[f] = dict(want[f], published=[p for p, i in zip(want[f]["published"], [j for j in model.leaves if want[f]["active"][j]])
                                               if nxt[i]])
    return want


@functools.lru_cache(maxsize=None)
def reference(name: str) -> tuple:
    """(scenario, want) -- computed once and shared: nobody writes into it."""
    scn = scenario(name)
    return scn, run(scn)


def events_of(scn: Scenario, want, leaf) -> dict:
    """gate_with_parking's events of one leaf over the frames of `want` (a leaf parked before frame 0: a 'p' in front)"""
    ev = {f: w["events"][leaf] for f, w in enumerate(want) if leaf in w["events"]}
    if leaf in scn.parked0:
        ev[0] = "p" + ev.get(0, "")
    return ev


def differs(a: list, b: list) -> bool:
    """Does any scheduled payload, callback, wake record or gate event of two runs differ?"""
    for wa, wb in zip(a, b):
        if wa["published"] != wb["published"] or wa["wake"] != wb["wake"] or wa["events"] != wb["events"]:
            return True
    return False
