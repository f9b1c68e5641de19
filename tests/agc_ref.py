"""The closed loop of option "agc" on the whole-tree model (test infrastructure; no GPU).

:class:`AgcTree` is live_ref.ModelTree with sdrreceiver_amd.agc.step applied to every USB leaf after each ``process``, its
result handed on as ``set_gain`` before the next frame -- which is all the option is (include/sdrx.h "device-side AGC").  The
model tree is pinned to the plain-C oracle by tests/test_live_model.py, so it is the oracle of the closed loop.
:func:`agc_tree` puts the same loop on another model tree (catchup_ref.CatchupTree: parking with catch-up).

:func:`settings` draws every USB leaf's window and initial gain from the model's OWN levels at unit gain
(:func:`unit_levels`), as live_ref.gate_settings draws thresholds: about a third of the leaves start hot (a gain that wraps),
a third cold, the rest in the window; a few sit out ``hold_frames``, a few have a limit within reach, one or two are silent.
:func:`reference` is the shared closed-loop run of one tree; :data:`TREES` names the trees the GPU test uses."""
from __future__ import annotations

import functools

import numpy as np

import catchup_ref
import lattice
import live_ref as lr
from sdrreceiver_amd import agc, synth

N_FRAMES = 8
RANDOM_SEEDS = (3, 11, 17, 24)
LATTICE_TREES = ("sub-3840", "sub-4352", "freq", "inner", "late-deep", "late0-2400", "deep-long")
SMALL_TREES = ("flat", "deep")  # catchup_ref's: "flat" holds the leaf with the long low-pass (k_lpf_long, K4Vfo::gain)
TREES = tuple(f"rnd-{s}" for s in RANDOM_SEEDS) + tuple(f"lat-{n}" for n in LATTICE_TREES) + tuple(f"small-{n}" for n in SMALL_TREES)
CASES = ("hot", "cold_raise", "cold_held", "in_window", "silent", "clamp_max", "clamp_min")


class _AgcMixin:
    """The step behind every frame.  cfg[leaf]: agc.Cfg (USB leaves; all zero = off, the start), quiet[leaf]: quiet_run."""

    def __init__(self, topo):
        super().__init__(topo)
        self.usb = [i for i in self.leaves if self.descs[i].demod_usb]
        self.cfg = {i: agc.Cfg(0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0) for i in self.usb}
        self.quiet = {i: 0 for i in self.usb}

    def set_agc(self, i, cfg):
        assert agc.invalid(cfg, self.descs[i].demod_usb) is None, (i, cfg)
        if i in self.cfg:
            self.cfg[i] = cfg
            self.quiet[i] = 0

    def unpark(self, ids):
        for i in ids:
            if i in self.quiet and not self.active[i]:  # the gain stays what the loop left; the cold run starts again
                self.quiet[i] = 0
        super().unpark(ids)

    def apply(self, ops):
        for op in ops:
            if op[0] == "agc":
                self.set_agc(op[1], op[2])
            else:
                super().apply([op])

    def process(self, iq) -> dict:
        res = super().process(iq)
        rec = {}
        for i in self.usb:
            g = np.float32(self.descs[i].gain)
            g2, q, action = agc.step(self.cfg[i], self.quiet[i], g, res["meters"][i], parked=not self.active[i])
            self.quiet[i] = q
            if action:
                self.set_gain(i, g2)
            rec[i] = dict(gain_used=g, gain_next=np.float32(g2), action=action, quiet_run=q)
        res["agc"] = rec
        return res


class AgcTree(_AgcMixin, lr.ModelTree):
    pass


@functools.lru_cache(maxsize=None)
def agc_tree(base):
    return type("Agc" + base.__name__, (_AgcMixin, base), {})


def _same(a, b) -> bool:
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


# ---- the trees and their frames -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tree(name):
    """(topo, frames) of one of :data:`TREES`: shared, nobody writes into them."""
    kind, key = name.split("-", 1)
    if kind == "rnd":
        topo = lr.topology_of(int(key))
        return topo, tuple(lr.frames_of(topo, int(key), N_FRAMES))
    if kind == "lat":
        return lattice.trees()[key], lattice.frames(key, N_FRAMES)
    topo = catchup_ref.TREES[key]()
    lcg = synth.Lcg(61)
    return topo, tuple(synth.lcg_frame(topo.frame, lcg) + synth.tone_frame(topo.frame, topo.fs, [(topo.fs / 9.1, 20.0)], f * topo.frame)
                       for f in range(N_FRAMES))


@functools.lru_cache(maxsize=None)
def unit_levels(name):
    """levels[leaf][f] = (mean square, peak) of the USB leaf's pre-quantisation values of frame f at gain 1 (floats): what its
    payload's mean square and peak are at gain g, times g^2 and g, as long as nothing wraps."""
    topo, frames = tree(name)
    model = lr.ModelTree(topo)
    usb = [i for i in model.leaves if topo.vfos[i].demod_usb]
    for i in usb:
        model.set_gain(i, 1.0)
    out = {i: [] for i in usb}
    for iq in frames:
        model.process(iq)
        for i in usb:
            pre = model.nodes[i].pre
            out[i].append((float(np.mean(pre * pre)), float(np.abs(pre).max())))
    return out


# ---- the settings ---------------------------------------------------------------------------------------------------------------
TARGET_MS = 2000 * 2000  # the middle of every window, LSB^2
UP, DOWN = 1.5, 0.5      # steps; window_is_stable wants hi >= 4 lo


def settings(topo, rng, levels):
    """{leaf: (agc.Cfg, initial gain, the class drawn)} for every USB leaf.  The window is TARGET_MS / 3 .. TARGET_MS * 3 (stable
    for the steps above); `levels` = :func:`unit_levels`.  With m, pk the median mean square and the largest peak of the leaf
    at unit gain: "in" starts at the gain that puts m on the target, "hot" at one whose peak wraps (at least 8 times that
    gain), "cold" 6 to 30 times below it.  Of the cold leaves every second one sits out 1 or 3 frames; some leaves get a
    gain_max / gain_min one step away from where they start; a "silent" leaf starts so low that its mean square is below
    silent_ms.

    `levels` are the model's pre-quantisation values at unit gain (mean square and peak of retune_ref.Node.pre), not its int16
    meters at unit gain: at gain 1 a leaf's int16 payload wraps many times over (a 20 LSB tone demodulates to 40 * 32768), so
    its meter says nothing about the level, and at a gain low enough not to wrap a weak leaf quantises to zero.  The floats
    are the same model's, one step earlier in the same chain."""
    out = {}
    usb = [i for i in topo.leaves_in_publish_order() if topo.vfos[i].demod_usb]
    usb.sort(key=lambda i: -lattice.lpf_taps(topo.vfos[i]))  # (stable: the longest audio low-pass first -- it starts hot, the next cold)
    classes = ["hot", "cold", "in"]
    for k, i in enumerate(usb):
        m = float(np.median([lv[0] for lv in levels[i]]))
        pk = max(lv[1] for lv in levels[i])
        m = max(m, 1e-12)
        g_in = float(np.sqrt(TARGET_MS / m))
        cls = classes[(k + int(rng.integers(0, 3))) % 3] if k >= 3 else classes[k]
        lo, hi, silent = TARGET_MS // 3, TARGET_MS * 3, 4
        hold = 0
        gmin, gmax = g_in / 1e4, g_in * 1e4
        if cls == "hot":
            g0 = max(g_in * 8.0, 40000.0 / max(pk, 1e-9)) * float(rng.uniform(1.0, 2.0))
            if rng.random() < 0.3:  # a floor one step below: the first step down is clamped
                gmin = g0 * 0.7
        elif cls == "cold":
            g0 = g_in / float(rng.uniform(6.0, 30.0))
            if rng.random() < 0.5:
                hold = int(rng.choice([1, 3]))
            elif rng.random() < 0.4:  # a ceiling one step above
                gmax = g0 * 1.2
        else:
            g0 = g_in * float(rng.uniform(0.8, 1.25))
        if k % 7 == 5:  # silent: a mean square below 4 LSB^2 however the frames differ
            cls, g0, hold = "silent", float(np.sqrt(1.0 / max(lv[0] for lv in levels[i]))), 0
        cfg = agc.Cfg(lo, hi, silent, hold, UP, DOWN, float(np.float32(gmin)), float(np.float32(gmax)))
        assert agc.invalid(cfg) is None and agc.window_is_stable(cfg), cfg
        out[i] = (cfg, float(np.float32(g0)), cls)
    return out


def classify(cfg, rec, m) -> str:
    """Which of :data:`CASES` one frame of one leaf is (None: AGC off, parked or an empty frame)."""
    if cfg.hi_ms == 0 or m["n_values"] == 0:
        return None
    if rec["action"] < 0:
        return "clamp_min" if _same(rec["gain_next"], cfg.gain_min) and not _same(np.float32(rec["gain_used"]) * np.float32(cfg.down), cfg.gain_min) else "hot"
    if rec["action"] > 0:
        return "clamp_max" if _same(rec["gain_next"], cfg.gain_max) and not _same(np.float32(rec["gain_used"]) * np.float32(cfg.up), cfg.gain_max) else "cold_raise"
    s, n = m["sum_sq"], m["n_values"]
    if s < cfg.silent_ms * n:
        return "silent"
    if s < cfg.lo_ms * n:
        return "cold_held"
    return "in_window"


@functools.lru_cache(maxsize=None)
def reference(name, base=lr.ModelTree):
    """(topo, frames, sets, want): sets = :func:`settings` of the tree (seeded by its name), want[f] = the closed loop's record
    of frame f -- ModelTree.process plus "agc": {leaf: gain_used, gain_next, action, quiet_run}.  Shared; read-only."""
    topo, frames = tree(name)
    sets = settings(topo, np.random.default_rng(70000 + TREES.index(name)), unit_levels(name))
    model = agc_tree(base)(topo)
    for i, (cfg, g0, _) in sets.items():
        model.set_gain(i, g0)
        model.set_agc(i, cfg)
    want = [model.process(iq) for iq in frames]
    return topo, frames, sets, want


def coverage(names=TREES) -> dict:
    """Counts over the closed loops of `names`: every case of :data:`CASES`, "leaves" (USB leaves) and "moved" (those whose gain
    changed at least once)."""
    out = {c: 0 for c in CASES}
    out["leaves"] = out["moved"] = 0
    for name in names:
        topo, _, sets, want = reference(name)
        for i, (cfg, _, _) in sets.items():
            out["leaves"] += 1
            out["moved"] += any(w["agc"][i]["action"] != 0 for w in want)
            for w in want:
                c = classify(cfg, w["agc"][i], w["meters"][i])
                if c:
                    out[c] += 1
    return out
