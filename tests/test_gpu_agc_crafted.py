"""Option "agc" on the device against the crafted schedules of tests/agc_crafted_ref.py: the gain step at its thresholds
(s == T n and one unit either side, products past 2^32, several meter records, one wrapped sample in a later record), the one
fp32 multiply and the clamp on arbitrary bit patterns, and 520 USB leaves -- three blocks of k_agc_step, nine of k_agc_set.
What the schedules hold, and that each wrong rule of ``agc_crafted_ref.mutants()`` would give another record somewhere, is
asserted without a GPU by tests/test_agc_crafted_model.py.

Everything is compared bit for bit, in the exact arithmetic: gain_used and gain_next as uint32 patterns, action, quiet_run, the
settings read back, every leaf's meter and payload of every frame checked (test_gpu_agc._check).

quiet_run saturating at 2^32 - 1 is not tested: no call can set the word, and the library gets no back door for it."""
import numpy as np
import pytest

import agc_crafted_ref as cr
from test_gpu_agc import COLS, _check, _device_frames, _f32

pytestmark = pytest.mark.gpu


def _call(rx, kind, ids, vals):
    if kind == "gain":
        rx.set_gains(list(ids), list(vals))
    else:
        rx.set_agc(list(ids), *[[getattr(c, k) for c in vals] for k in COLS])


def _apply(rx, calls):
    for kind, ids, vals in calls:
        _call(rx, kind, ids, vals)


def _check_settings(rx, expect, ctx):
    """The settings of EVERY USB leaf as sdrx_get_agc reads them back against `expect` = {leaf: Cfg}"""
    ids = list(expect)
    st = rx.agc(ids)
    for k, i in enumerate(ids):
        c = expect[i]
        got = tuple(int(st[n][k]) for n in COLS[:4]) + tuple(_f32(st[n][k]) for n in COLS[4:])
        want = tuple(getattr(c, n) for n in COLS[:4]) + tuple(_f32(getattr(c, n)) for n in COLS[4:])
        assert got == want, (ctx, i, "settings read back", got, want)


def _run_process(rx, ref, ctx, settings=False):
    expect = cr.settings_after(ref) if settings else None
    for f, iq in enumerate(ref["frames"]):
        for c, (kind, ids, vals) in enumerate(ref["sched"][f]):
            _call(rx, kind, ids, vals)
            if settings and f > 0:  # after each call: named leaves changed, all others untouched (the getter needs a delivered frame)
                _check_settings(rx, expect[f][c], (ctx, f, c))
        rx.process(iq)
        _check(rx, ref["topo"], ref["want"][f], f, ctx)
        if settings and expect[f]:
            _check_settings(rx, expect[f][-1], (ctx, f, "after the frame"))


# ---- 1. the boundary schedule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("park", [False, True])
@pytest.mark.parametrize("name", cr.TREES)
def test_boundary_schedule(name, park):
    """Both forms of k_agc_step (PARK is its one template parameter), every frame, the settings read back after every call."""
    from sdrreceiver_amd.receiver import Receiver
    ref = cr.boundary(name)
    rx = Receiver.from_topology(ref["topo"], exact=True, agc=True, park=park)
    _run_process(rx, ref, ("boundary", name, park), settings=True)
    rx.close()


@pytest.mark.parametrize("name", cr.TREES)
def test_boundary_schedule_queued_on_the_device(name):
    """The frames through sdrx_process_device back to back, with a fetch only where the schedule calls sdrx_set_agc (the gains
    of the hold section are set between queued frames): the frame in front of every such call and the last one are checked,
    and they are right only if every step in between ran in its place."""
    from sdrreceiver_amd.receiver import Receiver
    ref = cr.boundary(name)
    topo = ref["topo"]
    rx = Receiver.from_topology(topo, exact=True, agc=True)
    dev = _device_frames(ref["frames"])
    queued = fetched = 0
    for f, t in enumerate(dev):
        if queued and any(kind == "agc" for kind, _, _ in ref["sched"][f]):
            rx.fetch()
            _check(rx, topo, ref["want"][f - 1], f - 1, ("queued", name))
            queued, fetched = 0, fetched + 1
        _apply(rx, ref["sched"][f])
        rx.process_device(t.data_ptr(), topo.frame)
        queued += 1
    assert queued == cr.B_HOLD and fetched == cr.B_CASE + 2, "the hold section runs back to back"
    rx.fetch()
    _check(rx, topo, ref["want"][-1], len(dev) - 1, ("queued", name))
    rx.close()


# ---- 2. the multiply-and-clamp schedule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["process", "submit", "device"])
@pytest.mark.parametrize("name", cr.TREES)
def test_multiply_and_clamp(name, form):
    """Gains that compound over seven raises and seven lowerings, synchronously, with two frames in flight, and queued on the
    device with one fetch per half: gain_next of frame f is the gain frame f + 1 was computed with, so every payload checks
    the float the step stored, and the last frame of a half queued back to back is right only if all seven steps were."""
    from sdrreceiver_amd.receiver import Receiver
    ref = cr.clamp(name)
    topo = ref["topo"]
    rx = Receiver.from_topology(topo, exact=True, agc=True)
    ctx = ("clamp", name, form)
    if form == "process":
        _run_process(rx, ref, ctx, settings=True)
    elif form == "device":
        dev = _device_frames(ref["frames"])
        for first in (0, cr.C_ZERO):
            _apply(rx, ref["sched"][first])
            last = first + (cr.C_ZERO if first == 0 else cr.C_LOUD) - 1
            for f in range(first, last + 1):
                assert f == first or not ref["sched"][f]
                rx.process_device(dev[f].data_ptr(), topo.frame)
            rx.fetch()
            _check(rx, topo, ref["want"][last], last, ctx)
    else:
        done = 0

        def deliver():
            nonlocal done
            rx.wait()
            _check(rx, topo, ref["want"][done], done, ctx)
            done += 1

        for f, iq in enumerate(ref["frames"]):
            if ref["sched"][f]:
                while rx.in_flight():
                    deliver()
                _apply(rx, ref["sched"][f])
            rx.submit(iq)
            if rx.in_flight() == 2:
                deliver()
        while rx.in_flight():
            deliver()
        assert done == len(ref["frames"])
    rx.close()


# ---- 3. the wide tree -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("park", [False, True])
def test_wide_tree(park):
    """sdrx_set_agc with shuffled lists of 1, 63, 64, 65, 256, 257 and 520 leaves; after each call the settings of every leaf
    read back; every leaf's record, meter and payload of every frame."""
    from sdrreceiver_amd.receiver import Receiver
    ref = cr.wide()
    rx = Receiver.from_topology(ref["topo"], exact=True, agc=True, park=park)
    _run_process(rx, ref, ("wide", park), settings=True)
    rx.close()


def test_wide_tree_group_of_two():
    """The same calls and frames through sdrx_group_set_agc / sdrx_group_get_agc on two members of one device: the single
    context's records."""
    from sdrreceiver_amd.receiver import Group
    ref = cr.wide()
    g = Group.from_topology(ref["topo"], [0, 0], agc=1)
    _run_process(g, ref, ("wide", "group"), settings=True)
    g.close()
