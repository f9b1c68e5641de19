"""A model of a WHOLE tree under live controls, and a random schedule of them (test infrastructure; no GPU).

:class:`ModelTree` chains one retune_ref.Node per VFO, parent to child, frame by frame: roots get the raw frame, every other
node its parent's model stream.  Between frames it takes the four calls that change a running tree, with the semantics of
DESIGN.md 4d / 4i: a retune restarts the node's oscillator and keeps its filter state; a gain change acts on a USB leaf's next
frame (an IQ leaf's payload does not depend on it); a parked leaf does nothing; an unpark of a parked leaf replaces its node by
a fresh retune_ref.Node of the descriptor as it stands then (the reference's `new vfo`).  tests/test_live_model.py pins the
chain to the plain-C oracle on every random tree of helpers.random_topology, which is what makes it an oracle for
tests/test_gpu_live_random.py.

:func:`random_schedule` draws, per frame, the list of calls made before it; :func:`gate_settings` draws squelch settings
from the model's own meters, so that the gate opens in some frames and not in others."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import retune_ref as rr
from helpers import random_topology
from sdrreceiver_amd import meter, squelch as sq, synth
from test_park_model import gate_with_parking

N_FRAMES = 8
KINDS = ("iq_cstyle0", "iq_cstyle1", "childless_main", "d0_no_late", "late5", "late6", "usb_lpf", "usb_plain", "level2")


def depth(topo, i) -> int:
    """0 for a main, 1 for its children, 2 for theirs."""
    n = 0
    while topo.vfos[i].parent >= 0:
        i = topo.vfos[i].parent
        n += 1
    return n


def leaf_kinds(topo, i) -> set:
    """The kinds of KINDS leaf `i` belongs to (a leaf has several: every one selects code of its own in apply_active)."""
    d = topo.vfos[i]
    k = set()
    if d.demod_usb:
        k.add("usb_lpf" if d.filter_bw > 0 else "usb_plain")
        if d.late_decimate:
            k.add(f"late{d.late_decimate}")
    else:
        k.add(f"iq_cstyle{d.cstyle}")
    if d.parent < 0:
        k.add("childless_main")
    if d.decimate_count == 0 and not (d.demod_usb and d.late_decimate):
        k.add("d0_no_late")
    if depth(topo, i) == 2:
        k.add("level2")
    return k


def topic5(d) -> bytes:
    return d.topic.encode()[:5].ljust(5, b"\0")


class ModelTree:
    def __init__(self, topo):
        self.topo = topo
        self.descs = list(topo.vfos)
        self.nodes = [rr.Node(d) for d in self.descs]
        self.leaves = topo.leaves_in_publish_order()
        self.active = {i: 1 for i in self.leaves}
        self.since = {i: 0 for i in self.leaves}
        self.frame_no = 0  # the next frame

    # -- the calls between two frames -------------------------------------------------------------------------------------
    def retune(self, i, f):
        self.descs[i] = dataclasses.replace(self.descs[i], mixer_freq=float(f))
        self.nodes[i].retune(float(f))  # (a parked leaf's node is replaced at its unpark anyway)

    def set_gain(self, i, g):
        assert i in self.active, "gains act on leaves"
        self.descs[i] = dataclasses.replace(self.descs[i], gain=float(np.float32(g)))
        self.nodes[i].set_gain(g)

    def park(self, ids):
        for i in ids:
            if self.active[i]:
                self.active[i], self.since[i] = 0, self.frame_no

    def unpark(self, ids):
        for i in ids:
            if not self.active[i]:
                self.active[i], self.since[i] = 1, self.frame_no
                self.nodes[i] = rr.Node(self.descs[i])

    def apply(self, ops):
        """ops: ("park" | "unpark", ids) and ("freq" | "gain", id, value), in order."""
        for op in ops:
            if op[0] == "park":
                self.park(op[1])
            elif op[0] == "unpark":
                self.unpark(op[1])
            elif op[0] == "freq":
                self.retune(op[1], op[2])
            else:
                self.set_gain(op[1], op[2])

    # -- one frame ------------------------------------------------------------------------------------------------------
    def process(self, iq) -> dict:
        """`iq`: the raw frame, interleaved float32.  Returns streams[i] (None for a parked leaf), payload[leaf] (None when
        parked), meters[leaf] (meters_from_payload; the zero meter when parked) and published: the (topic, rate, bytes) of
        the active leaves in publish order."""
        raw = np.ascontiguousarray(iq, np.float32).view(np.complex64)
        streams, payload, meters, published = {}, {}, {}, []
        for i, d in enumerate(self.descs):  # (a parent precedes its children)
            if i in self.active and not self.active[i]:
                streams[i] = None
                continue
            streams[i] = self.nodes[i].process(raw if d.parent < 0 else streams[d.parent])
        for i in self.leaves:
            d = self.descs[i]
            if not self.active[i]:
                payload[i] = None
                meters[i] = {"n_values": 0, "sum_sq": 0, "clipped": 0, "peak": np.float32(0.0)}
                continue
            pay = self.nodes[i].payload()
            payload[i] = pay
            meters[i] = meter.meters_from_payload(d, pay, self.nodes[i].pre.astype(np.float32) if d.demod_usb else streams[i])
            published.append((topic5(d), d.output_rate, pay.tobytes()))
        self.frame_no += 1
        return dict(streams=streams, payload=payload, meters=meters, published=published,
                    active=dict(self.active), since=dict(self.since))


# ---- the schedule -------------------------------------------------------------------------------------------------------------
def _freq(rng, fs):
    """An integer in (-fs/2, fs/2); sometimes 0.0; sometimes a non-integer value."""
    r = rng.random()
    if r < 0.1:
        return 0.0
    v = float(int(rng.integers(-fs // 2 + 1, fs // 2)))
    if r < 0.25:
        v += float(int(rng.integers(1, 8))) / 8.0  # (eighths: exact in a double; v + 7/8 < fs/2 still)
    return v


def _gain(rng):
    return float(np.float32(rng.uniform(0.01, 0.08)))


def random_schedule(topo, rng, n_frames=N_FRAMES):
    """sched[f] = the calls before frame f, in order (the op tuples of ModelTree.apply; every op is one call of the library).
    Frames 0 and 1 and one later frame carry none.  Frame 2 parks 1 .. all leaves, and whatever is parked two frames before
    the end is unparked there, so that every tree parks and later unparks-and-delivers; in between the draws are free."""
    leaves = topo.leaves_in_publish_order()
    inner = [i for i in range(len(topo.vfos)) if topo.children(i)]
    usb = [i for i in leaves if topo.vfos[i].demod_usb]
    iq = [i for i in leaves if not topo.vfos[i].demod_usb]
    sched = [[] for _ in range(n_frames)]
    quiet = int(rng.integers(3, n_frames - 2))
    parked: set = set()

    def subset(pool, lo=1):
        pool = sorted(pool)
        k = int(rng.integers(lo, len(pool) + 1))
        return [int(v) for v in rng.choice(pool, size=k, replace=False)]

    for f in range(2, n_frames):
        if f == quiet:
            continue
        ops = sched[f]
        menu = []
        if f == 2:
            menu.append("park")
        elif f == n_frames - 2 and parked:
            menu.append("unpark_all")
        for _ in range(int(rng.integers(1, 4))):
            menu.append(str(rng.choice(["park", "unpark", "pu", "freq_leaf", "freq_inner", "freq_parked", "freq_unpark",
                                        "gain_usb", "gain_iq"], p=[0.12, 0.2, 0.1, 0.1, 0.14, 0.1, 0.1, 0.08, 0.06])))
        for what in menu:
            act = [i for i in leaves if i not in parked]
            if what == "park" and act:
                ids = subset(act)
                parked |= set(ids)
                ops.append(("park", ids))
            elif what == "unpark" and parked:
                ids = subset(parked)
                parked -= set(ids)
                ops.append(("unpark", ids))
            elif what == "unpark_all":
                ops.append(("unpark", sorted(parked)))
                parked.clear()
            elif what == "pu" and act:
                i = int(rng.choice(act))
                ops += [("park", [i]), ("unpark", [i])]
            elif what == "freq_leaf" and act:
                i = int(rng.choice(act))
                ops.append(("freq", i, _freq(rng, topo.vfos[i].fs)))
            elif what == "freq_inner" and inner:
                deep = [i for i in inner if any(topo.children(c) for c in topo.children(i))]
                i = int(rng.choice(deep if deep and rng.random() < 0.5 else inner))
                ops.append(("freq", i, _freq(rng, topo.vfos[i].fs)))
            elif what == "freq_parked" and parked:
                i = int(rng.choice(sorted(parked)))
                ops.append(("freq", i, _freq(rng, topo.vfos[i].fs)))
            elif what == "freq_unpark" and parked:
                i = int(rng.choice(sorted(parked)))
                pair = [("freq", i, _freq(rng, topo.vfos[i].fs)), ("unpark", [i])]
                ops += pair if rng.random() < 0.5 else pair[::-1]
                parked.discard(i)
            elif what == "gain_usb" and usb:
                ops.append(("gain", int(rng.choice(usb)), _gain(rng)))
            elif what == "gain_iq" and iq:
                ops.append(("gain", int(rng.choice(iq)), _gain(rng)))
    return sched


def events_of(sched, leaves):
    """The schedule as gate_with_parking's events: events[leaf][f] = a string of 'p' and 'u' in call order."""
    ev = {i: {} for i in leaves}
    for f, ops in enumerate(sched):
        for op in ops:
            if op[0] in ("park", "unpark"):
                for i in op[1]:
                    ev[i][f] = ev[i].get(f, "") + op[0][0]
    return ev


def coverage(topo, sched) -> dict:
    """What one schedule does, as counts: "parked_delivered:<kind>" for every kind of a leaf that is parked in some frame and
    active in a later one; the retunes of inner nodes with an inner child, of childless mains, of parked leaves; "pu" restarts;
    the kinds of retune value."""
    leaves = topo.leaves_in_publish_order()
    out: dict = {}

    def hit(k):
        out[k] = out.get(k, 0) + 1

    active = {i: 1 for i in leaves}
    was_parked = set()  # parked in at least one frame that ran
    for f, ops in enumerate(sched):
        at_start = dict(active)
        for n, op in enumerate(ops):
            if op[0] == "park":
                for i in op[1]:
                    if active[i] and n + 1 < len(ops) and ops[n + 1] == ("unpark", [i]):
                        hit("pu_restart")
                    active[i] = 0
            elif op[0] == "unpark":
                for i in op[1]:
                    active[i] = 1
            elif op[0] == "freq":
                i, v = op[1], op[2]
                hit("freq_zero" if v == 0.0 else "freq_integer" if v == int(v) else "freq_non_integer")
                if topo.children(i):
                    hit("retune_inner")
                    if any(topo.children(c) for c in topo.children(i)):
                        hit("retune_inner_with_inner_child")
                else:
                    if topo.vfos[i].parent < 0:
                        hit("retune_childless_main")
                    hit("retune_active_leaf" if active[i] else "retune_parked_leaf")
                    if not at_start[i] and any(o[0] == "unpark" and i in o[1] for o in ops):
                        hit("retune_with_unpark")
            else:
                hit("gain_usb" if topo.vfos[op[1]].demod_usb else "gain_iq")
        for i in leaves:  # frame f runs
            if not active[i]:
                was_parked.add(i)
            elif i in was_parked:
                was_parked.discard(i)
                for k in leaf_kinds(topo, i):
                    hit("parked_delivered:" + k)
        if not ops and f >= 2:
            hit("quiet_frame")
    return out


REQUIRED = tuple("parked_delivered:" + k for k in KINDS) + ("retune_inner_with_inner_child", "retune_childless_main",
                                                            "pu_restart", "retune_parked_leaf")


# ---- the gate settings --------------------------------------------------------------------------------------------------------
def gate_settings(topo, rng, sum_sq, events):
    """Per leaf: thr, hang (0..2), ratio_q8 and window (a third of the leaves: a ratio and a window of 2), and the model run
    `gate` = gate_with_parking's records.  sum_sq[leaf][f]: the model's meter (anything for a parked frame).  A fifth of the
    leaves keep thr 0 (always open while active).  For the others thr is an order statistic of the leaf's own active frames,
    starting at the median and moving on until the model run has an open AND a closed active frame; a leaf for which no order
    statistic does is reported in `exempt` with thr 0 -- the caller decides what to make of it."""
    leaves = topo.leaves_in_publish_order()
    out = {"thr": {}, "hang": {}, "ratio": {}, "window": {}, "gate": {}, "exempt": {}}
    for i in leaves:
        hang = int(rng.integers(0, 3))
        auto = rng.random() < 1 / 3
        ratio, window = (int(rng.choice([128, 256, 384, 512])), 2) if auto else (0, 0)
        zero = rng.random() < 0.2
        run = lambda thr: gate_with_parking(sum_sq[i], events[i], thr, hang, ratio, window)  # noqa: E731
        thr, g = 0, run(0)
        if not zero:
            vals = sorted({int(s) for s, r in zip(sum_sq[i], g) if r["active"]} - {0})
            start = len(vals) // 2
            for k in range(len(vals)):
                t = vals[(start + k) % len(vals)]
                gt = run(t)
                act = [r for r in gt if r["active"]]
                if any(r["open"] for r in act) and any(not r["open"] for r in act):
                    thr, g = t, gt
                    break
            else:
                out["exempt"][i] = f"no order statistic of {len(vals)} distinct sum_sq values opens and closes it (hang {hang}, ratio {ratio})"
        out["thr"][i], out["hang"][i], out["ratio"][i], out["window"][i], out["gate"][i] = thr, hang, ratio, window, g
    return out


# ---- one reference per seed, shared ------------------------------------------------------------------------------------------
def topology_of(seed):
    return random_topology(np.random.default_rng(1000 + seed))


def frames_of(topo, seed, n=N_FRAMES):
    """synth.lcg_frame plus one tone, phase-continuous over the frames."""
    lcg = synth.Lcg(700 + seed)
    return [synth.lcg_frame(topo.frame, lcg) + synth.tone_frame(topo.frame, topo.fs, [(topo.fs / 7.3, 20.0)], f * topo.frame)
            for f in range(n)]


@functools.lru_cache(maxsize=None)
def reference(seed, n=N_FRAMES):
    """(topo, frames, sched, want, gate) of one seed: want[f] = ModelTree.process of frame f under the schedule; gate =
    gate_settings on the model's meters.  Computed once and shared: nobody writes into it."""
    topo = topology_of(seed)
    frames = frames_of(topo, seed, n)
    sched = random_schedule(topo, np.random.default_rng(20000 + seed), n)
    model = ModelTree(topo)
    want = []
    for f, iq in enumerate(frames):
        model.apply(sched[f])
        want.append(model.process(iq))
    leaves = topo.leaves_in_publish_order()
    s = {i: [w["meters"][i]["sum_sq"] for w in want] for i in leaves}
    gate = gate_settings(topo, np.random.default_rng(30000 + seed), s, events_of(sched, leaves))
    return topo, frames, sched, want, gate, model.descs


def units(payload) -> int:
    return sq.align64(payload.nbytes)
