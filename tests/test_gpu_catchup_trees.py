"""Unpark with catch-up (option "catchup") on the seeded random trees and on the lattice of tests/lattice.py, and with the
default keep_streams = 0, where a fused late decimation and a fused demodulation leave the leaf without a stream buffer.

tests/test_gpu_catchup.py runs two hand-built trees on one frame length with every stream kept.  Here the catch-up -- per-leaf
sub-lists of the work lists, launched with frame K-1 against the parent's buffer of parity (K-1) & 1 -- meets what those trees
do not hold: 60 random trees under live_ref.random_schedule (three levels, IQ leaves, retunes and gain changes of parked leaves
and of their parents, restarts, catch-ups discarded by a park, several leaves of different levels in one call), and every
lattice tree under catchup_ref.lattice_schedule (d = 0 .. 8, 3-8 chunks with and without a partial last one, the late
decimation on 2-5 late-chunks, scalecomp 3 .. 100, mixers at and beyond Nyquist).  The references -- catchup_ref.reference_random
and reference_lattice: catchup_ref.CatchupTree, pinned to the plain-C oracle by tests/test_catchup_trees_model.py, which also
shows that at frame K a caught-up leaf's payload differs from the model without the option on more than 95 % of the leaves --
are computed once and shared.

Bars: exact = 1 bit for bit; exact = 0 and 2 within 1e-5 of max|model stream|, int16 within 1 LSB, int8 within 1
(test_gpu_live_random.py's).  A tree sdrx_finalize refuses must carry one of the two documented messages; 55 of 60 must run."""
import os

import numpy as np
import pytest

import catchup_ref as cr
import lattice as lt
import retune_ref as rr
import spectrum_ref as sr
from test_gpu_catchup import _close, _meter_of, _run, _want_meter
from test_gpu_live_random import REL_TOL, _apply_ops, _check_after, _create, _drive, _options
from test_park_model import NONE

pytestmark = pytest.mark.gpu

N_SEEDS = int(os.environ.get("SDRX_TEST_SEEDS", "60"))
LATTICE = sorted(lt.trees())
SEGMENTS = [0, 1, 2, 3, 5]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _open_gates(topo, want, kinds):
    """every threshold 0: open while active, and pre(K) = 1 for a caught-up leaf"""
    return {i: cr.gate([w["meters"][i]["sum_sq"] for w in want], kinds[i], 0, 0) for i in topo.leaves_in_publish_order()}


class _Stepper:
    """The context as _drive and _apply_ops see it, counting the calls of the schedule: when the last call in front of frame f
    has returned -- before frame f runs and, in the device form, sometimes before frame f - 1 is fetched -- sdrx_get_catchup
    must answer what the model holds for f."""

    def __init__(self, rx, topo, sched, want, ctx, exact=True):
        self._rx, self._leaves, self._want, self._ctx, self._exact = rx, topo.leaves_in_publish_order(), want, ctx, exact
        self._left = {f: len(ops) for f, ops in enumerate(sched) if ops}
        self._f = min(self._left) if self._left else None
        self.steps = 0

    def __getattr__(self, name):
        return getattr(self._rx, name)

    def _called(self):
        f = self._f
        self._left[f] -= 1
        if self._left[f]:
            return
        del self._left[f]
        self._f = min(self._left) if self._left else None
        check_catchup(self._rx, self._leaves, self._want[f]["caught"], (self._ctx, "before frame", f), self._exact)
        self.steps += 1

    def set_active(self, vids, active):
        self._rx.set_active(vids, active)
        self._called()

    def set_mixer_freqs(self, vids, freqs):
        self._rx.set_mixer_freqs(vids, freqs)
        self._called()

    def set_gains(self, vids, gains):
        self._rx.set_gains(vids, gains)
        self._called()


def check_catchup(rx, leaves, caught, ctx, exact=True):
    cu = rx.catchup(leaves)
    for k, i in enumerate(leaves):
        c = caught.get(i)
        if c is None:
            assert (int(cu["frame"][k]), _meter_of(cu, k)) == (-1, (0, 0, 0, 0)), (ctx, i, "not caught up")
            continue
        assert int(cu["frame"][k]) == c["frame"] and int(cu["n_values"][k]) == c["meter"]["n_values"], (ctx, i, "caught-up frame")
        if exact is True:
            assert _meter_of(cu, k) == _want_meter(c["meter"]), (ctx, i, "the meter of the caught-up frame")


def _check_frame(rx, topo, want, gates, f, ctx, streams, settings=None):
    """Delivered frame f, bit for bit: what the callback saw (a pre-rolled payload ahead of the leaf's payload; after a
    catch-up that is the payload of K-1 the catch-up computed), egress and pre-roll counts, per leaf the payload, the
    pre-rolled payload and the meter, and every stream that is readable.  With `settings` (live_ref.gate_settings) also the
    gate's own state."""
    leaves = topo.leaves_in_publish_order()
    w = want[f]
    pub, n_open, n_pre, nbytes = cr.delivery(topo, want, gates, f)
    assert [(t, r, len(b)) for t, r, b in rx.published] == [(t, r, len(b)) for t, r, b in pub], (ctx, f, "callbacks: topics, order, sizes")
    assert rx.published == pub, (ctx, f, "callbacks: bytes")
    eg, pc = rx.egress(), rx.preroll_count()
    assert (eg["frame"], eg["n_open"], eg["n_leaves"], eg["payload_bytes_copied"]) == (f, n_open, len(leaves), nbytes), (ctx, f, eg)
    assert pc["n_preroll"] == n_pre, (ctx, f, pc)
    m = rx.meters(leaves)
    if settings is not None:
        st, au = rx.squelch(leaves), rx.squelch_auto(leaves)
    for k, i in enumerate(leaves):
        g = gates[i][f]
        pay, pre = rx.output(i), rx.preroll(i)
        assert int(m["frame"][k]) == f, (ctx, f, i)
        if settings is not None:
            assert int(st["open"][k]) == g["open"], (ctx, f, i, "open")
            assert int(st["hang_left"][k]) == g["hang_left"], (ctx, f, i, "hang_left")
            assert int(au["thr_eff_sum_sq"][k]) == g["thr_eff"], (ctx, f, i, "thr_eff")
            assert int(au["floor_valid"][k]) == int(g["floor"] != NONE), (ctx, f, i, "floor_valid")
            assert int(au["floor_sum_sq"][k]) == (0 if g["floor"] == NONE else g["floor"]), (ctx, f, i, "floor")
        if w["payload"][i] is None:  # parked in f -- also for a K-1 fetched after the unpark: the reports stay "parked"
            assert pay.size == 0 and pre.size == 0, (ctx, f, i, "a parked leaf is delivered")
            assert _meter_of(m, k) == (0, 0, 0, 0), (ctx, f, i, "a parked leaf has a meter")
            continue
        assert _meter_of(m, k) == _want_meter(w["meters"][i]), (ctx, f, i, "meter")
        if not g["open"]:
            assert pay.size == 0 and pre.size == 0, (ctx, f, i, "a closed leaf is delivered")
            continue
        assert np.array_equal(_bits(pay), _bits(w["payload"][i])), (ctx, f, i, "payload")
        if g["pre"]:
            assert np.array_equal(_bits(pre), _bits(cr.preroll_of(want, i, f))), (ctx, f, i, "pre-rolled payload")
        else:
            assert pre.size == 0, (ctx, f, i, "pre-roll")
    if streams:
        for i in range(len(topo.vfos)):
            got, z = rx.stream(i, missing_ok=True), w["streams"][i]
            if z is None:
                assert got is None, (ctx, f, i, "a parked leaf has a stream")
            else:
                assert got is None or np.array_equal(_bits(got), _bits(z)), (ctx, f, i, "stream")


def _check_afterwards(rx, topo, sched, want, descs, ctx):
    """_check_after (the retuned tables, active, since_frame = K and not K-1), and the table of every leaf that was unparked"""
    _check_after(rx, topo, sched, want, descs, ctx)
    for i in topo.leaves_in_publish_order():
        if want[-1]["since"][i]:
            L = topo.vfos[i].fs
            assert np.array_equal(_bits(rx.nco(i, L - 64, 64)), _bits(rr.table(L, descs[i].mixer_freq)[L - 64:])), (ctx, i, "nco")


# ------------------------------------------------------------------------------ the random trees
@pytest.mark.parametrize("form", ["process", "submit", "device"])
def test_random_trees_exact(form):
    """catchup = 1, meter = 1 and the launch options of test_gpu_live_random._options (keep_streams on for the even seeds, the
    default for the odd ones) under the random schedules: every delivered frame and, right after each schedule step,
    sdrx_get_catchup against the model."""
    from sdrreceiver_amd.receiver import Receiver
    ran = caught = 0
    for seed in range(N_SEEDS):
        topo, frames, sched, want, _, descs, kinds = cr.reference_random(seed)
        opts = _options(seed)
        rx = _create(lambda: Receiver.from_topology(topo, exact=True, catchup=True, meter=True, **opts), seed)
        if rx is None:
            continue
        ctx = ("catchup", form, seed, opts)
        gates = _open_gates(topo, want, kinds)
        step = _Stepper(rx, topo, sched, want, ctx)
        seen = _drive(step, topo, frames, sched, form, lambda f, s: _check_frame(rx, topo, want, gates, f, ctx, s), seed)
        assert seen and seen[-1] == len(frames) - 1 and (form == "device" or seen == list(range(len(frames)))), (ctx, seen)
        assert step.steps == sum(1 for ops in sched if ops), (ctx, "a schedule step without its sdrx_get_catchup check")
        _check_afterwards(rx, topo, sched, want, descs, ctx)
        rx.close()
        ran += 1
        caught += sum(1 for f, w in enumerate(want) for c in w["caught"].values() if c["frame"] == f - 1)
    assert ran >= N_SEEDS * 55 // 60, ran
    assert caught >= 2 * ran, (caught, ran)


@pytest.mark.parametrize("form", ["process", "device"])
def test_random_trees_with_the_gate(form):
    """squelch, preroll, squelch_auto and catchup with the settings of catchup_ref.reference_random (thresholds that are order
    statistics of the leaf's own model sum_sq, a third of the leaves with a ratio over a tracked floor): open, hang_left,
    thr_eff, the floor, pre, the pre-rolled payload -- the catch-up's where catchup_ref.preroll_of says so --, n_open and the
    bytes copied, for every leaf and delivered frame.  No leaf is exempt: tests/test_catchup_trees_model.py holds that share
    to 0."""
    from sdrreceiver_amd.receiver import Receiver
    ran = 0
    for seed in range(N_SEEDS):
        topo, frames, sched, want, gate, descs, kinds = cr.reference_random(seed)
        opts = dict(segments=seed % 3, fuse_demod=seed % 2 == 1)
        rx = _create(lambda: Receiver.from_topology(topo, exact=True, squelch=True, preroll=True, squelch_auto=True, catchup=True,
                                                    **opts), seed)
        if rx is None:
            continue
        leaves = topo.leaves_in_publish_order()
        rx.set_squelch(leaves, [gate["thr"][i] for i in leaves], [gate["hang"][i] for i in leaves])
        rx.set_squelch_auto(leaves, [gate["ratio"][i] for i in leaves], [gate["window"][i] for i in leaves])
        ctx = ("catchup, gate", form, seed, opts)
        step = _Stepper(rx, topo, sched, want, ctx)
        seen = _drive(step, topo, frames, sched, form, lambda f, s: _check_frame(rx, topo, want, gate["gate"], f, ctx, s, gate), seed)
        assert seen and seen[-1] == len(frames) - 1, (ctx, seen)
        rx.close()
        ran += 1
    assert ran >= N_SEEDS * 55 // 60, ran


def test_random_trees_on_a_group():
    """Every second seed on sdrx_group_*, 2-5 members on device 0 (inner nodes replicated; a leaf has one owner): what the
    callback publishes -- the pre-rolled catch-up ahead of the payload, in the reference's order over the whole tree --,
    sdrx_group_get_catchup through group_gather after every schedule step, and sdrx_group_get_active afterwards."""
    from sdrreceiver_amd.receiver import Group
    seeds = list(range(0, N_SEEDS, 2))
    ran = 0
    for seed in seeds:
        topo, frames, sched, want, _, _, kinds = cr.reference_random(seed)
        members = int(np.random.default_rng(9000 + seed).integers(2, 6))
        g = _create(lambda: Group.from_topology(topo, [0] * members, catchup=1), seed)
        if g is None:
            continue
        leaves = topo.leaves_in_publish_order()
        gates = _open_gates(topo, want, kinds)
        for f, iq in enumerate(frames):
            ctx = ("catchup, group", seed, members, f)
            _apply_ops(g, sched[f])
            check_catchup(g, leaves, want[f]["caught"], ctx)
            g.process(iq)
            pub, _, n_pre, nbytes = cr.delivery(topo, want, gates, f)
            assert [(t, r, len(b)) for t, r, b in g.published] == [(t, r, len(b)) for t, r, b in pub], (ctx, "topics / order / sizes")
            assert g.published == pub, (ctx, "published payloads")
            assert g.preroll_count()["n_preroll"] == n_pre and g.egress()["payload_bytes_copied"] == nbytes, ctx
            for i in leaves:
                if want[f]["payload"][i] is None:
                    assert g.output(i).size == 0 and g.preroll(i).size == 0, (ctx, i)
                elif gates[i][f]["pre"]:
                    assert np.array_equal(_bits(g.preroll(i)), _bits(cr.preroll_of(want, i, f))), (ctx, i)
        st = g.active(leaves)
        assert [int(v) for v in st["active"]] == [want[-1]["active"][i] for i in leaves], (seed, members)
        assert [int(v) for v in st["since_frame"]] == [want[-1]["since"][i] for i in leaves], (seed, members)
        g.close()
        ran += 1
    assert ran >= len(seeds) * 5 // 6, ran


def _check_tolerance(rx, topo, want, gates, f, ctx, all_streams=True):
    w = want[f]
    for i, d in enumerate(topo.vfos):
        z, got = w["streams"][i], rx.stream(i, missing_ok=True)
        if z is None:
            assert got is None and rx.output(i).size == 0 and rx.preroll(i).size == 0, (ctx, f, i, "a parked leaf")
            continue
        assert got is not None or not all_streams, (ctx, f, i, "keep_streams keeps every stream")
        if got is not None:
            ratio = float(np.abs(got - z).max()) / float(np.abs(z).max())
            assert ratio <= REL_TOL, (ctx, f, i, "stream", ratio)
        if topo.children(i):
            continue
        assert _close(topo, i, rx.output(i), w["payload"][i]), (ctx, f, i, "payload")
        pre = rx.preroll(i)
        if gates[i][f]["pre"]:
            assert _close(topo, i, pre, cr.preroll_of(want, i, f)), (ctx, f, i, "pre-rolled payload")
        else:
            assert pre.size == 0, (ctx, f, i, "pre-roll")


@pytest.mark.parametrize("exact", [0, 2])
def test_random_trees_tolerance_arithmetics(exact):
    """exact = 0 and 2, every third seed, keep_streams on, against test_live_controls_tolerance's bars: every stream within
    1e-5 of max|model stream|, int16 within 1 LSB, int8 within 1 -- the pre-rolled catch-up payload included."""
    from sdrreceiver_amd.receiver import Receiver
    seeds = list(range(0, N_SEEDS, 3))
    ran = pre = 0
    for seed in seeds:
        topo, frames, sched, want, _, _, kinds = cr.reference_random(seed)
        rx = _create(lambda: Receiver.from_topology(topo, exact=exact, catchup=True, keep_streams=True, segments=seed % 3), seed)
        if rx is None:
            continue
        gates = _open_gates(topo, want, kinds)
        ctx = ("catchup", exact, seed)
        step = _Stepper(rx, topo, sched, want, ctx, exact=exact)
        for f, iq in enumerate(frames):
            _apply_ops(step, sched[f])
            rx.process(iq)
            _check_tolerance(rx, topo, want, gates, f, ctx)
            pre += sum(gates[i][f]["pre"] for i in gates)
        rx.close()
        ran += 1
    assert ran >= len(seeds) * 5 // 6, ran
    assert pre >= ran, (pre, ran)


# ------------------------------------------------------------------------------ the lattice
@pytest.mark.parametrize("form", ["process", "device"])
def test_lattice_exact(form):
    """Every lattice tree under catchup_ref.lattice_schedule: every leaf with a parent is parked before frame 1, half of them
    caught up on frame 1 (parity 1) by one call, the rest on frame 2 (parity 0), one retuned and one re-gained while parked,
    one restarted before frame 4.  segments rotate over 0 .. 5, keep_streams alternates, fuse_demod on every third tree."""
    from sdrreceiver_amd.receiver import Receiver
    for k, name in enumerate(LATTICE):
        topo, frames, sched, want, descs, kinds = cr.reference_lattice(name)
        opts = dict(segments=SEGMENTS[k % 5], keep_streams=k % 2 == 1, fuse_demod=k % 3 == 0)
        rx = Receiver.from_topology(topo, exact=True, catchup=True, meter=True, **opts)
        ctx = ("catchup", name, form, opts)
        gates = _open_gates(topo, want, kinds)
        step = _Stepper(rx, topo, sched, want, ctx)
        seen = _drive(step, topo, frames, sched, form, lambda f, s: _check_frame(rx, topo, want, gates, f, ctx, s), k)
        assert seen and seen[-1] == lt.N_FRAMES - 1, (ctx, seen)
        assert step.steps == 4, ctx
        _check_afterwards(rx, topo, sched, want, descs, ctx)
        rx.close()


def test_lattice_widest_tree_robust():
    """The widest tree (USB leaves at d = 0 .. 8, IQ leaves at d = 5 .. 8 with scalecomp up to 100) once in the robust
    arithmetic, the bars of test_gpu_lattice.py::test_live_controls_robust."""
    from sdrreceiver_amd.receiver import Receiver
    name = lt.WIDEST
    topo, frames, sched, want, _, kinds = cr.reference_lattice(name)
    rx = Receiver.from_topology(topo, exact=2, catchup=True, keep_streams=True, segments=2)
    gates = _open_gates(topo, want, kinds)
    ctx = ("catchup", name, "robust")
    step = _Stepper(rx, topo, sched, want, ctx, exact=2)
    for f, iq in enumerate(frames):
        _apply_ops(step, sched[f])
        rx.process(iq)
        _check_tolerance(rx, topo, want, gates, f, ctx)
    rx.close()


# ------------------------------------------------------------------------------ the two small trees without kept streams
CASES_DEFAULT_STREAMS = [
    ("flat", "process", dict()),
    ("flat", "process", dict(fuse_demod=True)),
    ("flat", "device", dict()),
    ("flat", "device", dict(fuse_demod=True, tail_in_levels=True)),
    ("flat", "process", dict(fuse_late=False)),
    ("flat", "device", dict(segments=3)),
    ("flat", "process", dict(segments=3, fuse_demod=True)),
    ("deep", "process", dict()),
    ("deep", "process", dict(segments=3)),
    ("deep", "device", dict(fuse_demod=True)),
    ("deep", "device", dict()),
]


@pytest.mark.parametrize("key,mode,opts", CASES_DEFAULT_STREAMS, ids=[f"{k}-{m}-{'-'.join(f'{a}{int(b)}' for a, b in o.items())}"
                                                                      for k, m, o in CASES_DEFAULT_STREAMS])
def test_small_trees_with_default_streams(key, mode, opts):
    """keep_streams = 0, the shipped configuration: the fused /5 and /6 leaves and, under fuse_demod, the d = 2 leaves have no
    stream buffer and no tap -- the catch-up's mix items write their demodulation state and nothing else.  Payloads, pre-rolled
    payloads, meters, callbacks and sdrx_get_catchup as in tests/test_gpu_catchup.py; a stream is compared where one is kept."""
    _run(key, mode, keep_streams=False, **opts)


# ------------------------------------------------------------------------------ spectrum, tap and watch around a catch-up
def test_a_spectrum_counts_the_frames_from_k_on_and_the_tap_of_a_fused_leaf_comes_back():
    """"A spectrum is not updated by the catch-up" (DESIGN.md 4k), on the flat tree without kept streams: leaf 1 (plain USB)
    and leaf 4 (the fused /5: a stream only as the tap) carry a spectrum and are parked for frames 0 and 1.  Unparked before
    frame 2 they run frame 1 in the catch-up; `updates` counts frames 2, 3, 4 alone, and the display is the model's fed the
    device's own stream of those frames -- which is the CatchupTree's, as are the payloads."""
    from sdrreceiver_amd.receiver import Receiver
    from test_gpu_spectrum import check
    topo = cr.flat_tree()
    frames = cr.frames("flat")[:5]
    vids = [1, 4]
    sched = {0: [("park", vids)], 2: [("unpark", vids)]}
    want, _ = cr.run_model(topo, frames, sched)
    assert all(want[2]["caught"][v]["frame"] == 1 for v in vids)
    rx = Receiver.from_topology(topo, keep_streams=False, catchup=True)
    rx.set_tap(4)
    for v in vids:
        rx.set_spectrum(v)
    disp = {v: sr.Display() for v in vids}
    for f, iq in enumerate(frames):
        _apply_ops(rx, sched.get(f, []))
        if f == 2:  # caught up, frame 2 not yet run: what is reported is still frame 1, where both were parked
            check_catchup(rx, vids, want[2]["caught"], "spectrum")
            assert [int(u) for u in rx.spectrum_levels(vids)["updates"]] == [0, 0], "the catch-up updated a spectrum"
            assert all(rx.stream(v, missing_ok=True) is None for v in vids), "frame 1 reports a stream"
        rx.process(iq)
        for v in vids:
            if f < 2:
                assert rx.stream(v, missing_ok=True) is None, (f, v)
            else:
                z = rx.stream(v)  # (leaf 4: the tap selection was kept while it was parked)
                assert np.array_equal(_bits(z), _bits(want[f]["streams"][v])), (f, v, "stream")
                assert np.array_equal(_bits(rx.output(v)), _bits(want[f]["payload"][v])), (f, v, "payload")
                disp[v].update(z)
            check(rx.spectrum(v), disp[v], ("catchup", f, v))
        assert [int(u) for u in rx.spectrum_levels(vids)["updates"]] == [max(0, f - 1)] * 2, f
        if f == 2:
            assert all(np.array_equal(_bits(rx.preroll(v)), _bits(want[2]["caught"][v]["payload"])) for v in vids), "pre-roll"
    rx.close()


def test_a_watch_reads_the_same_before_and_after_the_catch_up_and_as_without_the_option():
    """Watched, parked leaves of the flat tree (a plain USB leaf, the fused /5 and an IQ leaf): sdrx_get_watch and
    sdrx_get_watch_psd of frame K-1 read the same before and after the sdrx_set_active that catches the leaves up, and in every
    frame they are those of a twin with catchup = 0 under the same calls."""
    from sdrreceiver_amd.receiver import Receiver
    topo = cr.flat_tree()
    frames = cr.frames("flat")[:5]
    ids = [2, 4, 9]

    def figures(rx):
        w = rx.watch(ids)
        psd = [rx.watch_psd(i) for i in ids]
        return {k: np.array(v).tobytes() for k, v in w.items()}, [(p.tobytes(), fr) for p, fr in psd]

    seen = {}
    for cu in (True, False):
        rx = Receiver.from_topology(topo, keep_streams=False, watch=True, park=True, preroll=True, catchup=cu)
        rx.set_active(ids, [0] * len(ids))
        rx.set_watch(ids, [1] * len(ids))
        rec = []
        for f, iq in enumerate(frames):
            if f == 3:
                before = figures(rx)
                rx.set_active(ids, [1] * len(ids))
                if cu:
                    assert [int(v) for v in rx.catchup(ids)["frame"]] == [2] * len(ids)
                assert figures(rx) == before, (cu, "the figures of frame K-1 changed under sdrx_set_active")
                assert before == rec[-1]
            rx.process(iq)
            rec.append(figures(rx))
            assert [fr for _, fr in rec[-1][1]] == [f] * len(ids), (cu, f)
            assert [int(v) for v in rx.watch(ids)["watched"]] == [1] * len(ids), (cu, f)
            if f == 3:  # (the twins differ in what they deliver, not in what they watch)
                assert [rx.preroll(i).size > 0 for i in ids] == [cu] * len(ids), (cu, "the pre-roll of frame 3")
        assert all(rx.output(i).size > 0 for i in ids)
        seen[cu] = rec
        rx.close()
    for f, (a, b) in enumerate(zip(seen[True], seen[False])):
        assert a == b, (f, "a watch figure differs from the option off")
    assert len({r[1][0][0] for r in seen[True]}) == len(frames), "the PSD does not change from frame to frame: nothing was compared"
