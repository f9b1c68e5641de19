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
:func:`reference` the shared model run over their schedules."""
from __future__ import annotations

import functools

import numpy as np

import lattice
import live_ref
import retune_ref as rr
from sdrreceiver_amd import meter, squelch as sq, synth
from sdrreceiver_amd.topology import _g
from test_park_model import NONE

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
                self.caught[i] = dict(frame=self.frame_no - 1, stream=z, payload=pay, meter=m)

    def process(self, iq) -> dict:
        res = super().process(iq)
        self.last_streams = res["streams"]
        self.ran = dict(self.active)
        res["caught"] = {i: c for i, c in self.caught.items()}  # (what sdrx_get_catchup answers after this frame)
        return res


def gate(sum_sq, events, thr, hang_frames):
    """One leaf's gate over the frames of `sum_sq`: gate_with_parking's rules (no auto-squelch) plus 'c'."""
    thr_of = (lambda f: int(thr[f])) if isinstance(thr, (list, tuple)) else (lambda f: int(thr))
    active, left, prev_open = 1, 0, 1
    out = []
    for f, s in enumerate(sum_sq):
        for e in events.get(f, ""):
            if e == "p":
                active = 0
            elif e in "uc" and not active:
                active, left, prev_open = 1, 0, int(e == "u")
        is_open = pre = 0
        if active:
            if int(s) >= thr_of(f):
                is_open, left = 1, int(hang_frames)
            elif left > 0:
                is_open, left = 1, left - 1
            pre = int(is_open and not prev_open)
            prev_open = is_open
        out.append(dict(active=active, open=is_open, pre=pre, hang_left=left, prev_open=prev_open))
    return out


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
