"""Retune, gain and parking on the seeded random trees, against the whole-tree model of tests/live_ref.py.

The 60 random trees of helpers.random_topology carry what the hand-built trees of test_gpu_retune.py / test_gpu_park.py do
not: IQ leaves of both compress styles (k_compress, its K3Vfo flag), childless mains, d = 0 leaves without a late decimation,
the /5 and /6 late decimation fused and unfused on frames that are no multiple of the chunk, three levels, and rates of
6 144 ... 98 304 Hz >> d for the NCO replay.  Every tree runs 8 frames under live_ref.random_schedule (parks, unparks, restarts
between two frames, retunes of leaves, inner nodes and parked leaves, gain changes), with the launch options rotating by seed.
The reference of a seed -- live_ref.reference: the model tree under the schedule, pinned to the plain-C oracle by
tests/test_live_model.py -- is computed once and shared by every test here.

A tree sdrx_finalize refuses must carry one of the two documented messages; at least 55 of 60 must run."""
import os

import numpy as np
import pytest

import live_ref as lr
import retune_ref as rr
from sdrreceiver_amd.receiver import SdrxError
from test_park_model import NONE

pytestmark = pytest.mark.gpu

N_SEEDS = int(os.environ.get("SDRX_TEST_SEEDS", "60"))
REL_TOL = 1e-5  # test_gpu_parity.py::test_fast_mode_on_random_trees' bar


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _options(seed):
    """The rotation of test_random_trees_against_the_oracle, plus the two launch options it leaves alone."""
    return dict(segments=seed % 5, fuse=seed % 3 != 0, keep_streams=seed % 2 == 0, fuse_late=seed % 7 != 0,
                fuse_demod=seed % 4 >= 2, tail_in_levels=seed % 5 != 3, pipeline=seed % 3 == 1)


def _create(make, seed):
    """The context, or None for a tree the library refuses under a documented restriction."""
    try:
        return make()
    except SdrxError as e:
        assert "fs >= 1024" in str(e) or "last chunk shorter than 256" in str(e), (seed, str(e))
        return None


def _apply_ops(rx, ops):
    for op in ops:  # (every op is one call)
        if op[0] == "park":
            rx.set_active(op[1], [0] * len(op[1]))
        elif op[0] == "unpark":
            rx.set_active(op[1], [1] * len(op[1]))
        elif op[0] == "freq":
            rx.set_mixer_freqs([op[1]], [op[2]])
        else:
            rx.set_gains([op[1]], [op[2]])


def _same_peak(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


def _check_exact(rx, topo, w, f, ctx, streams):
    """One delivered frame against the model's record `w` of frame f, bit for bit, with the delivery rules of a parked leaf."""
    assert [p[0] for p in rx.published] == [p[0] for p in w["published"]], (ctx, f, "topics / publish order")
    assert rx.published == w["published"], (ctx, f, "published rates or payloads")
    leaves = topo.leaves_in_publish_order()
    m = rx.meters(leaves)
    assert [int(v) for v in m["frame"]] == [f] * len(leaves), (ctx, f, m["frame"])
    for k, i in enumerate(leaves):
        pay, want, wm = rx.output(i), w["payload"][i], w["meters"][i]
        got_m = (int(m["n_values"][k]), int(m["sum_sq"][k]), int(m["clipped"][k]))
        if want is None:
            assert pay.size == 0, (ctx, f, i, "a parked leaf has a payload")
            assert got_m == (0, 0, 0) and float(m["peak"][k]) == 0.0, (ctx, f, i, "a parked leaf's meter", got_m)
        else:
            assert np.array_equal(_bits(pay), _bits(want)), (ctx, f, i, "payload")
            assert got_m == (wm["n_values"], wm["sum_sq"], wm["clipped"]), (ctx, f, i, "meter", got_m, wm)
            assert _same_peak(m["peak"][k], wm["peak"]), (ctx, f, i, "peak", m["peak"][k], wm["peak"])
    if streams:
        for i in range(len(topo.vfos)):
            got, want = rx.stream(i, missing_ok=True), w["streams"][i]
            if want is None:
                assert got is None, (ctx, f, i, "a parked leaf has a stream")
            else:
                assert got is None or np.array_equal(_bits(got), _bits(want)), (ctx, f, i, "stream")


def _check_after(rx, topo, sched, want, descs, ctx):
    for i in sorted({op[1] for ops in sched for op in ops if op[0] == "freq"}):
        L = topo.vfos[i].fs
        assert np.array_equal(_bits(rx.nco(i, L - 64, 64)), _bits(rr.table(L, descs[i].mixer_freq)[L - 64:])), (ctx, i, "nco")
    leaves = topo.leaves_in_publish_order()
    st = rx.active(leaves)
    assert [int(v) for v in st["active"]] == [want[-1]["active"][i] for i in leaves], (ctx, "active")
    assert [int(v) for v in st["since_frame"]] == [want[-1]["since"][i] for i in leaves], (ctx, "since_frame")


def _drive(rx, topo, frames, sched, form, check, seed):
    """Feeds the frames in one of three forms and calls check(f, streams) for every delivered frame.  Returns the set of
    delivered frames.  "device": 1-3 frames queued with sdrx_process_device (a change between them drains what is queued), and
    for about every second group the calls of the NEXT frame arrive before the fetch: the frame fetched then ran before them
    and must be delivered in the state it ran in."""
    n = len(frames)
    seen = []
    if form == "process":
        for f in range(n):
            _apply_ops(rx, sched[f])
            rx.process(frames[f])
            check(f, True)
            seen.append(f)
    elif form == "submit":
        done = 0

        def deliver():
            nonlocal done
            rx.wait()
            check(done, rx.in_flight() == 0)  # (stream read-backs wait for the frames in flight)
            seen.append(done)
            done += 1

        for f in range(n):
            if sched[f]:  # the calls refuse while frames are in flight
                while rx.in_flight():
                    deliver()
                _apply_ops(rx, sched[f])
            rx.submit(frames[f])
            if rx.in_flight() == 2:
                deliver()
        while rx.in_flight():
            deliver()
    else:
        import torch
        dev = [torch.from_numpy(iq).cuda() for iq in frames]
        torch.cuda.synchronize()
        rng = np.random.default_rng(40000 + seed)
        applied = set()
        f = 0
        while f < n:
            last = min(n, f + int(rng.integers(1, 4))) - 1
            for g in range(f, last + 1):
                if g not in applied:
                    _apply_ops(rx, sched[g])
                    applied.add(g)
                rx.process_device(dev[g].data_ptr(), topo.frame)
            if last + 1 < n and sched[last + 1] and rng.random() < 0.5:
                _apply_ops(rx, sched[last + 1])
                applied.add(last + 1)
            rx.fetch()
            check(last, True)
            seen.append(last)
            f = last + 1
    return seen


@pytest.mark.parametrize("form", ["process", "submit", "device"])
def test_live_controls_exact(form):
    """Every payload, every readable stream and every meter of every delivered frame equal the model's, parked leaves follow
    the delivery rules of DESIGN.md 4i, and afterwards sdrx_get_nco / sdrx_get_active give the model's tables and states."""
    from sdrreceiver_amd.receiver import Receiver
    ran = 0
    for seed in range(N_SEEDS):
        topo, frames, sched, want, _, descs = lr.reference(seed)
        opts = _options(seed)
        rx = _create(lambda: Receiver.from_topology(topo, exact=True, park=True, meter=True, **opts), seed)
        if rx is None:
            continue
        ctx = (form, seed, opts)
        seen = _drive(rx, topo, frames, sched, form, lambda f, s: _check_exact(rx, topo, want[f], f, ctx, s), seed)
        assert seen and seen[-1] == len(frames) - 1 and (form == "device" or seen == list(range(len(frames)))), (ctx, seen)
        _check_after(rx, topo, sched, want, descs, ctx)
        rx.close()
        ran += 1
    assert ran >= N_SEEDS * 55 // 60, ran


def _check_gate(rx, topo, want, gate, f, ctx):
    leaves = topo.leaves_in_publish_order()
    st, au, eg = rx.squelch(leaves), rx.squelch_auto(leaves), rx.egress()
    n_open = copied = 0
    published = []
    for k, i in enumerate(leaves):
        d, m = topo.vfos[i], gate["gate"][i][f]
        assert int(st["open"][k]) == m["open"], (ctx, f, i, "open")
        assert int(st["hang_left"][k]) == m["hang_left"], (ctx, f, i, "hang_left")
        assert int(au["thr_eff_sum_sq"][k]) == m["thr_eff"], (ctx, f, i, "thr_eff")
        assert int(au["floor_valid"][k]) == int(m["floor"] != NONE), (ctx, f, i, "floor_valid")
        assert int(au["floor_sum_sq"][k]) == (0 if m["floor"] == NONE else m["floor"]), (ctx, f, i, "floor")
        pre, pay = rx.preroll(i), rx.output(i)
        if m["pre"]:
            before = want[f - 1]["payload"][i]
            assert before is not None, (ctx, f, i, "the model pre-rolls a parked frame")
            assert np.array_equal(_bits(pre), _bits(before)), (ctx, f, i, "pre-rolled payload")
            published.append((lr.topic5(d), d.output_rate, before.tobytes()))
            copied += lr.units(before)
        else:
            assert pre.size == 0, (ctx, f, i, "pre-roll")
        if m["open"]:
            assert np.array_equal(_bits(pay), _bits(want[f]["payload"][i])), (ctx, f, i, "payload")
            published.append((lr.topic5(d), d.output_rate, pay.tobytes()))
            copied += lr.units(pay)
        else:
            assert pay.size == 0, (ctx, f, i, "a closed leaf has a payload")
        n_open += m["open"]
    assert (eg["frame"], eg["n_open"], eg["n_leaves"], eg["payload_bytes_copied"]) == (f, n_open, len(leaves), copied), (ctx, f, eg)
    assert rx.published == published, (ctx, f, "what the callback saw")


@pytest.mark.parametrize("form", ["process", "device"])
def test_live_controls_with_the_gate(form):
    """squelch, preroll and squelch_auto on, settings from live_ref.gate_settings (thresholds that are order statistics of the
    leaf's own model sum_sq): open, hang_left, thr_eff, the floor, the pre-rolled payload, n_open and the bytes copied against
    test_park_model.gate_with_parking for every leaf and delivered frame.  In the device form 1-3 frames are queued per
    fetch and the calls arrive between them."""
    from sdrreceiver_amd.receiver import Receiver
    ran = 0
    for seed in range(N_SEEDS):
        topo, frames, sched, want, gate, _ = lr.reference(seed)
        opts = dict(segments=seed % 3, fuse_demod=seed % 2 == 1)
        rx = _create(lambda: Receiver.from_topology(topo, exact=True, park=True, squelch=True, preroll=True, squelch_auto=True,
                                                    **opts), seed)
        if rx is None:
            continue
        leaves = topo.leaves_in_publish_order()
        rx.set_squelch(leaves, [gate["thr"][i] for i in leaves], [gate["hang"][i] for i in leaves])
        rx.set_squelch_auto(leaves, [gate["ratio"][i] for i in leaves], [gate["window"][i] for i in leaves])
        ctx = ("gate", form, seed, opts)
        if form == "process":
            for f, iq in enumerate(frames):
                _apply_ops(rx, sched[f])
                rx.process(iq)
                _check_gate(rx, topo, want, gate, f, ctx)
        else:
            import torch
            dev = [torch.from_numpy(iq).cuda() for iq in frames]
            torch.cuda.synchronize()
            rng = np.random.default_rng(50000 + seed)
            f = 0
            while f < len(frames):
                last = min(len(frames), f + int(rng.integers(1, 4))) - 1
                for g in range(f, last + 1):
                    _apply_ops(rx, sched[g])
                    rx.process_device(dev[g].data_ptr(), topo.frame)
                rx.fetch()
                _check_gate(rx, topo, want, gate, last, ctx)
                f = last + 1
        rx.close()
        ran += 1
    assert ran >= N_SEEDS * 55 // 60, ran


def test_live_controls_on_a_group():
    """Every second seed on sdrx_group_*, 2-5 members on one device (an inner node is replicated on every member that holds
    part of its subtree: every replica must be retuned): what the callback publishes -- topic, rate, bytes, in the reference's
    order over the whole tree -- is the model's, and sdrx_group_get_active agrees."""
    from sdrreceiver_amd.receiver import Group
    seeds = list(range(0, N_SEEDS, 2))
    ran = 0
    for seed in seeds:
        topo, frames, sched, want, _, _ = lr.reference(seed)
        members = int(np.random.default_rng(9000 + seed).integers(2, 6))
        g = _create(lambda: Group.from_topology(topo, [0] * members, park=1), seed)
        if g is None:
            continue
        for f, iq in enumerate(frames):
            _apply_ops(g, sched[f])
            g.process(iq)
            assert [p[0] for p in g.published] == [p[0] for p in want[f]["published"]], (seed, members, f, "topics / order")
            assert g.published == want[f]["published"], (seed, members, f, "published rates or payloads")
            for i in topo.leaves_in_publish_order():
                if want[f]["payload"][i] is None:
                    assert g.output(i).size == 0, (seed, members, f, i)
        leaves = topo.leaves_in_publish_order()
        st = g.active(leaves)
        assert [int(v) for v in st["active"]] == [want[-1]["active"][i] for i in leaves], (seed, members)
        assert [int(v) for v in st["since_frame"]] == [want[-1]["since"][i] for i in leaves], (seed, members)
        g.close()
        ran += 1
    assert ran >= len(seeds) * 5 // 6, ran


def _int8_within_one(got, want, cstyle):
    """compress() keeps the low 8 bits of a truncated float (and cstyle 1 the high nibble of each component): a float within
    the tolerance moves the integer by at most 1, which the wrap can turn into 255 (15 for a nibble)."""
    g, w = got.view(np.uint8).astype(np.int32), want.view(np.uint8).astype(np.int32)
    if cstyle == 1:
        parts = [((g >> 4) - (w >> 4)) % 16, ((g & 15) - (w & 15)) % 16]
        return all(np.isin(p, (0, 1, 15)).all() for p in parts)
    return bool(np.isin((g - w) % 256, (0, 1, 255)).all())


@pytest.mark.parametrize("exact", [0, 2])
def test_live_controls_tolerance(exact):
    """The tolerance arithmetics under the same schedules, every third seed, keep_streams on: every stream within 1e-5 of
    max|model stream|, int16 within 1 LSB, int8 within 1.  No gate and no meter equality: their integers may differ by the LSB."""
    from sdrreceiver_amd.receiver import Receiver
    seeds = list(range(0, N_SEEDS, 3))
    ran, worst = 0, (0.0, None)
    for seed in seeds:
        topo, frames, sched, want, _, _ = lr.reference(seed)
        rx = _create(lambda: Receiver.from_topology(topo, exact=exact, park=True, keep_streams=True, segments=seed % 3), seed)
        if rx is None:
            continue
        for f, iq in enumerate(frames):
            _apply_ops(rx, sched[f])
            rx.process(iq)
            w = want[f]
            for i, d in enumerate(topo.vfos):
                z, got = w["streams"][i], rx.stream(i, missing_ok=True)
                if z is None:
                    assert got is None and rx.output(i).size == 0, (exact, seed, f, i, "a parked leaf")
                    continue
                assert got is not None, (exact, seed, f, i, "keep_streams keeps every stream")
                ratio = float(np.abs(got - z).max()) / float(np.abs(z).max())
                worst = max(worst, (ratio, (seed, f, i)))
                assert ratio <= REL_TOL, (exact, seed, f, i, "stream", ratio)
                if topo.children(i):
                    continue
                pay, ref = rx.output(i), w["payload"][i]
                assert pay.size == ref.size, (exact, seed, f, i)
                if d.demod_usb:
                    assert int(np.abs(pay.astype(np.int32) - ref.astype(np.int32)).max()) <= 1, (exact, seed, f, i, "int16")
                else:
                    assert _int8_within_one(pay, ref, d.cstyle), (exact, seed, f, i, "int8")
        rx.close()
        ran += 1
    print(f"exact = {exact}: worst stream error / max|stream| = {worst[0]:.3e} at (seed, frame, node) = {worst[1]}")
    assert ran >= len(seeds) * 5 // 6, ran
