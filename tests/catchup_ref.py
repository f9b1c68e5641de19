"""Model of unpark with catch-up (option "catchup", include/sdrx.h "Unpark with catch-up") for the tests; no GPU.

It extends the models the parking tests stand on by the two sentences of the definition:

* :class:`CatchupTree` -- live_ref.ModelTree, where an unpark of a leaf that has a parent and was parked in the frame before
  replaces its node by a fresh retune_ref.Node (the reference's `new vfo`) and feeds it the parent's MODEL stream of that frame
  at once: the node's frames K-1, K, K+1 are those of a new vfo fed the parent's stream from K-1 on.  What the frame K-1 gave
  (stream, payload, meter) is kept as long as the leaf's present active state lasts: sdrx_get_catchup.
* :func:`gate` -- test_park_model.gate_with_parking with one more event: 'c', an unpark that catches up, leaves prev_open = 0
  where 'u' leaves 1.  No gate runs on K-1, so pre(K) = open(K).
* :func:`delivery` -- what a delivered frame carries: per open leaf in publish order its pre-rolled payload, then its payload;
  the counts and the packed bytes.

:func:`flat_tree` and :func:`deep_tree` are the small trees of the GPU tests (tests/lattice.py's builder and geometry rules),
:func:`reference` the shared model run over their schedules.  :func:`reference_random` runs the random trees and schedules of
tests/live_ref.py, :func:`reference_lattice` every tree of tests/lattice.py under :func:`lattice_schedule`; :func:`coverage`
says what a schedule catches up (tests/test_catchup_trees_model.py asserts :data:`REQUIRED` and the lattice cells)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import lattice
import live_ref
import retune_ref as rr
from sdrreceiver_amd import meter, squelch as sq, synth
from sdrreceiver_amd.topology import _g
from test_park_model import NONE, gate_with_parking  # noqa: F401

N_FRAMES = 7


class CatchupTree(live_ref.ModelTree):
    def __init__(self, topo):
        super().__init__(topo)
        self.last_streams: dict = {}                  # the model streams of the last frame that ran
        self.ran = {i: 1 for i in self.leaves}        # was the leaf active in that frame?
        self.caught: dict = {}                        # leaf -> dict(frame, stream, payload, meter) of its catch-up
        self.kinds = {i: {} for i in self.leaves}     # leaf -> {frame: 'p' | 'u' | 'c' ...}: the events of :func:`gate`

    def _event(self, i, e):
        self.kinds[i][self.frame_no] = self.kinds[i].get(self.frame_no, "") + e

    def park(self, ids):
        for i in ids:
            if self.active[i]:
                self.caught.pop(i, None)              # parked again before K: the catch-up is discarded
                self._event(i, "p")
        super().park(ids)

    def unpark(self, ids):
        for i in ids:
            if self.active[i]:
                continue
            d = self.descs[i]
            catch = d.parent >= 0 and self.frame_no >= 1 and not self.ran[i]
            super().unpark([i])
            self.caught.pop(i, None)
            self._event(i, "c" if catch else "u")
            if catch:
                node = self.nodes[i]
                z = node.process(self.last_streams[d.parent])
                pay = node.payload()
                m = meter.meters_from_payload(d, pay, node.pre.astype(np.float32) if d.demod_usb else z)
                self.caught[i] = dict(frame=self.frame_no - 1, stream=z, payload=pay, meter=m, desc=d)

    def process(self, iq) -> dict:
        res = super().process(iq)
        self.last_streams = res["streams"]
        self.ran = dict(self.active)
        res["caught"] = {i: c for i, c in self.caught.items()}  # (what sdrx_get_catchup answers after this frame)
        return res


def gate(sum_sq, events, thr, hang_frames, ratio_q8=0, window_frames=0):
    """One leaf's gate over the frames of `sum_sq`: test_park_model.gate_with_parking, whose event 'c' is the catch-up."""
    return gate_with_parking(sum_sq, events, thr, hang_frames, ratio_q8, window_frames)


def delivery(topo, want, gates, f):
    """Frame f as delivered: (published, n_open, n_pre, packed bytes).  want: the frames of CatchupTree.process; gates[leaf]:
    :func:`gate`'s records.  The pre-rolled payload of a leaf caught up in f-1 is the catch-up's, else its payload of f-1."""
    pub, n_open, n_pre, nbytes = [], 0, 0, 0
    for i in topo.leaves_in_publish_order():
        g = gates[i][f]
        if not g["open"]:
            continue
        d = want[f]["descs"][i]
        pay = want[f]["payload"][i]
        n_open += 1
        nbytes += sq.align64(pay.nbytes)
        if g["pre"]:
            pre = preroll_of(want, i, f)
            n_pre += 1
            nbytes += sq.align64(pre.nbytes)
            pub.append((live_ref.topic5(d), d.output_rate, pre.tobytes()))
        pub.append((live_ref.topic5(d), d.output_rate, pay.tobytes()))
    return pub, n_open, n_pre, nbytes


def preroll_of(want, i, f):
    c = want[f]["caught"].get(i)
    if c is not None and c["frame"] == f - 1 and want[f]["since"][i] == f:
        return c["payload"]
    return want[f - 1]["payload"][i]


# ---- the small trees ------------------------------------------------------------------------------------------------------------
def flat_tree():
    """Two levels.  Node 0: the main, d = 1 on 4 800 samples -> 2 400 at 9 600 S/s (2 chunks and 352 samples: a partial last
    chunk; 2.5 chunks of the fused /5, 2.38 of the /6).  Its leaves, in order: 1 d = 2 USB; 2 d = 2 USB with a 47-tap low-pass
    (fuse_demod's shape); 3 d = 5 USB; 4 /5 at d = 0; 5 /6 at d = 0 with a low-pass; 6 /5 at d = 1; 7 /6 at d = 3; 8 d = 1 USB
    with a long low-pass (k_lpf_long); 9 IQ cstyle 0; 10 IQ cstyle 1."""
    b = lattice._Build("catchup-flat", 4800)
    m = b.inner(-1, 1)
    b.usb(m, 2)
    b.usb(m, 2, bw=500)
    b.usb(m, 5)
    b.usb(m, 0, late=5)
    b.usb(m, 0, late=6, bw=320)
    b.usb(m, 1, late=5)
    b.usb(m, 3, late=6)
    b.usb(m, 1, bw=150)
    b.iq(m, 3, 0)
    b.iq(m, 2, 1, 3)
    return _gains(b.t)


def deep_tree():
    """Three levels and a parent-less leaf.  0: the main (d = 1); 1: an inner node below it (d = 0); 2, 3: level-2 leaves (USB
    d = 3, IQ cstyle 0 d = 2); 4: a d = 2 USB leaf with the low-pass on level 1; 5: a parent-less USB leaf (d = 3); 6: a d = 0 USB leaf on level 1 (no late decimation)."""
    b = lattice._Build("catchup-deep", 4800)
    m = b.inner(-1, 1)
    a = b.inner(m, 0)
    b.usb(a, 3)
    b.iq(a, 2, 0)
    b.usb(m, 2, bw=500)
    b.usb(-1, 3)
    b.usb(m, 0)
    return _gains(b.t)


def _gains(t):
    for d in t.vfos:
        if d.demod_usb:
            d.gain = _g(0.004)  # (no int16 wraps on frames(): asserted by tests/test_catchup_model.py)
    return t


TREES = {"flat": flat_tree, "deep": deep_tree}
LONG_LPF_LEAF = 8

# frame -> the calls before it, in order (live_ref.ModelTree.apply).  flat: everything but leaf 1 is parked before frame 1 (leaf
# 1 never is); the unparks are staggered over frames 3 .. 5, leaf 2 retuned and re-gained while parked; leaf 3 is parked again
# and restarted before frame 5 (not caught up), leaf 4 caught up, parked and unparked again before frame 4 (caught up anew).
# deep: the parent-less leaf 5 is unparked before frame 3 (not caught up), the level-2 leaves before 3 and 4.
SCHED = {
    "flat": {1: [("park", [2, 3, 4, 5, 6, 7, 8, 9, 10])],
             2: [("freq", 2, -1300.0), ("gain", 2, _g(0.003))],
             3: [("unpark", [2, 3, 9])],
             4: [("unpark", [4]), ("park", [4]), ("unpark", [4, 5, 8])],
             5: [("unpark", [6, 7, 10]), ("park", [3]), ("unpark", [3])]},
    "deep": {1: [("park", [2, 3, 4, 5, 6])], 3: [("unpark", [2, 5])], 4: [("unpark", [3, 4, 6])]},
}


@functools.lru_cache(maxsize=None)
def frames(key, n=N_FRAMES, seed=23):
    topo = TREES[key]()
    lcg = synth.Lcg(seed)
    return [synth.lcg_frame(topo.frame, lcg) + synth.tone_frame(topo.frame, topo.fs, [(topo.fs / 9.1, 20.0)], f * topo.frame)
            for f in range(n)]


def run_model(topo, frs, sched):
    model = CatchupTree(topo)
    want = []
    for f, iq in enumerate(frs):
        model.apply(sched.get(f, []))
        w = model.process(iq)
        w["descs"] = list(model.descs)
        want.append(w)
    return want, model


@functools.lru_cache(maxsize=None)
def reference(key):
    """(topo, want, events, gates at threshold 0) of one tree under its schedule.  Computed once and shared: nobody writes
    into it."""
    topo = TREES[key]()
    want, model = run_model(topo, frames(key), SCHED[key])
    leaves = topo.leaves_in_publish_order()
    s = {i: [w["meters"][i]["sum_sq"] for w in want] for i in leaves}
    gates = {i: gate(s[i], model.kinds[i], 0, 0) for i in leaves}
    return topo, want, model.kinds, gates


# ---- the random trees and the lattice under catch-up --------------------------------------------------------------------------
def _sum_sq(topo, want):
    return {i: [w["meters"][i]["sum_sq"] for w in want] for i in topo.leaves_in_publish_order()}


@functools.lru_cache(maxsize=None)
def reference_random(seed, n=live_ref.N_FRAMES):
    """(topo, frames, sched, want, gate, descs, kinds) of one seed: the topology, frames and schedule of live_ref.reference(seed)
    run on a CatchupTree.  want[f] carries "caught" and "descs"; kinds = CatchupTree.kinds; gate = live_ref.gate_settings drawn
    from THIS model's meters and events (a caught-up leaf's levels of K on are not ModelTree's).  Computed once and shared:
    nobody writes into it."""
    topo = live_ref.topology_of(seed)
    frs = live_ref.frames_of(topo, seed, n)
    sched = live_ref.random_schedule(topo, np.random.default_rng(20000 + seed), n)
    want, model = run_model(topo, frs, dict(enumerate(sched)))
    gate_set = live_ref.gate_settings(topo, np.random.default_rng(30000 + seed), _sum_sq(topo, want), model.kinds)
    return topo, frs, sched, want, gate_set, list(model.descs), model.kinds


def _freq_class(d):
    return {c[2] for c in lattice.cells(lattice.Topology(fs=d.fs, frame=d.samples_per_buffer, vfos=[dataclasses.replace(d, parent=-1)]))
            if c[2].startswith("freq:")}


def lattice_schedule(topo, n=lattice.N_FRAMES) -> list:
    """sched[f] = the calls before frame f on a lattice tree.  Before 1: every leaf that has a parent is parked.  Before 2: every
    second one of them is unparked in one call (caught up on frame 1, parity 1); in front of that call the first of them whose
    mixer is in no class of its own is retuned by a sixteenth of its output rate plus 3/8 Hz (the tone stays in its passband).
    Before 3: the first USB leaf still parked gets half its gain, then the rest is unparked in one call (caught up on frame 2,
    parity 0).  Before 4: the first leaf with a parent is parked and unparked again -- a restart, not caught up."""
    v = topo.vfos
    below = [i for i in topo.leaves_in_publish_order() if v[i].parent >= 0]
    sched = [[] for _ in range(n)]
    if not below:
        return sched
    first, rest = below[0::2], below[1::2]
    sched[1].append(("park", below))
    plain = [i for i in first if not _freq_class(v[i])]
    if plain:
        i = plain[0]
        sched[2].append(("freq", i, v[i].mixer_freq + round(v[i].output_rate / 16.0) + 0.375))
    sched[2].append(("unpark", first))
    usb = [i for i in rest if v[i].demod_usb]
    if usb:
        sched[3].append(("gain", usb[0], _g(v[usb[0]].gain * 0.5)))
    if rest:
        sched[3].append(("unpark", rest))
    sched[4] += [("park", [below[0]]), ("unpark", [below[0]])]
    return sched


@functools.lru_cache(maxsize=None)
def reference_lattice(name):
    """(topo, frames, sched, want, descs, kinds) of one lattice tree under :func:`lattice_schedule` on lattice.frames(name)."""
    topo = lattice.trees()[name]
    frs = [np.array(iq) for iq in lattice.frames(name)]
    sched = lattice_schedule(topo)
    want, model = run_model(topo, frs, dict(enumerate(sched)))
    return topo, frs, sched, want, list(model.descs), model.kinds


def leaf_cells(topo, descs, i) -> set:
    """The cells of tests/lattice.py that leaf i holds, from its chain alone, with the descriptors as they stand in `descs`."""
    chain = [i]
    while descs[chain[-1]].parent >= 0:
        chain.append(descs[chain[-1]].parent)
    chain.reverse()
    t = lattice.Topology(fs=topo.fs, frame=topo.frame, name=topo.name,
                         vfos=[dataclasses.replace(descs[k], parent=n - 1) for n, k in enumerate(chain)])
    return {c for c in lattice.cells(t) if not c[0].startswith("inner")}


def coverage(topo, sched, want, kinds) -> dict:
    """What one schedule catches up, as counts (the style of live_ref.coverage), from the model run: "caught:<kind>" per kind of
    live_ref.leaf_kinds of a leaf caught up and delivered in K; the parities of K-1; a retune while parked before a catch-up and
    the two orders of a retune and the unpark in one frame; a catch-up discarded by a park before K; unparks that are not caught
    up (parent-less, restart, K = 0); one call that catches up leaves of two tree levels; "cell:<cell>" per lattice cell of a
    caught-up leaf (descriptors as at the catch-up)."""
    out: dict = {}

    def hit(k):
        out[k] = out.get(k, 0) + 1

    leaves = topo.leaves_in_publish_order()
    active = {i: 1 for i in leaves}
    ran = dict(active)
    retuned_parked = set()
    for f, ops in enumerate(sched):
        for n, op in enumerate(ops):
            if op[0] == "park":
                for i in op[1]:
                    active[i] = 0
            elif op[0] == "freq" and op[1] in active and not active[op[1]]:
                retuned_parked.add(op[1])
            elif op[0] == "unpark":
                caught = [i for i in op[1] if not active[i] and not ran[i] and f >= 1 and topo.vfos[i].parent >= 0]
                for i in op[1]:
                    if active[i]:
                        continue
                    active[i] = 1
                    if i in caught:
                        if i in retuned_parked:
                            hit("caught_after_parked_retune")
                        if any(o[0] == "freq" and o[1] == i for o in ops[:n]):
                            hit("freq_then_unpark_caught")
                        if any(o[0] == "freq" and o[1] == i for o in ops[n + 1:]):
                            hit("unpark_then_freq_caught")
                    elif topo.vfos[i].parent < 0:
                        hit("unpark_parent_less")
                    elif f == 0:
                        hit("unpark_before_frame_0")
                    else:
                        hit("pu_restart")
                    retuned_parked.discard(i)
                if len({live_ref.depth(topo, i) for i in caught}) >= 2:
                    hit("one_call_two_levels")
        for i in leaves:
            ev = kinds[i].get(f, "")
            for a, b in zip(ev, ev[1:]):
                if a + b == "cp":
                    hit("discarded_by_park")
            c = want[f]["caught"].get(i)
            if c is not None and c["frame"] == f - 1 and want[f]["since"][i] == f:  # caught up and delivered in K = f
                assert ev.endswith("c"), (f, i, ev)
                hit(f"parity:{(f - 1) & 1}")
                for k in live_ref.leaf_kinds(topo, i):
                    hit("caught:" + k)
                if live_ref.depth(topo, i) == 2:
                    hit("caught_on_level_2")
                descs = list(want[f]["descs"])
                descs[i] = c["desc"]
                for cell in leaf_cells(topo, descs, i):
                    hit(f"cell:{cell}")
        ran = dict(active)
    return out


# a childless main has no parent: it is never caught up, and "unpark_parent_less" asks for its unpark instead
REQUIRED = tuple("caught:" + k for k in live_ref.KINDS if k != "childless_main") + (
    "caught_on_level_2", "caught_after_parked_retune", "freq_then_unpark_caught", "unpark_then_freq_caught", "discarded_by_park",
    "unpark_parent_less", "pu_restart", "parity:0", "parity:1", "one_call_two_levels")


def required_lattice_cells() -> set:
    """Every cell of lattice.required_cells() that a leaf with a parent occupies in some lattice tree."""
    held = set()
    for topo in lattice.trees().values():
        for i in topo.leaves_in_publish_order():
            if topo.vfos[i].parent >= 0:
                held |= leaf_cells(topo, topo.vfos, i)
    return held & lattice.required_cells()
