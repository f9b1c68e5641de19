"""Option "agc" on the device against the closed loop of the whole-tree model (tests/agc_ref.py; what that loop covers is
asserted without a GPU by tests/test_agc_model.py).

The trees: four seeds of live_ref.topology_of, seven of tests/lattice.py and catchup_ref's two small ones, 8 frames each.
Between them: USB leaf counts of 1 .. 25, leaves with one meter record and with several, a leaf whose gain lives in K4Vfo (a
309-tap low-pass), /5 and /6 leaves fused and not, fuse_demod leaves on the last level and off it (records per mix item),
compress() leaves and childless mains.  Every reference is computed once (functools.lru_cache in agc_ref) and shared."""
import dataclasses

import numpy as np
import pytest

import agc_ref as ar
import catchup_ref as cr
import live_ref as lr
from sdrreceiver_amd import _lib, agc
from sdrreceiver_amd.receiver import SdrxError

pytestmark = pytest.mark.gpu

COLS = ("lo_ms", "hi_ms", "silent_ms", "hold_frames", "up", "down", "gain_min", "gain_max")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _f32(x):
    return int(np.float32(x).view(np.uint32))


def _set(rx, sets, ids=None):
    """The initial gains, then the settings, of the leaves `ids` (default: every USB leaf), one call each."""
    ids = list(sets) if ids is None else list(ids)
    rx.set_gains(ids, [sets[i][1] for i in ids])
    rx.set_agc(ids, *[[getattr(sets[i][0], c) for i in ids] for c in COLS])


def _check(rx, topo, w, f, ctx, payloads=True):
    """One delivered frame against the closed loop's record `w` of frame f: the step's record, the meter and the payload of
    every leaf, bit for bit."""
    leaves = topo.leaves_in_publish_order()
    a, m = rx.agc(leaves), rx.meters(leaves)
    assert [int(v) for v in a["frame"]] == [f] * len(leaves) == [int(v) for v in m["frame"]], (ctx, f, a["frame"], m["frame"])
    for k, i in enumerate(leaves):
        d = topo.vfos[i]
        got = (_f32(a["gain_used"][k]), _f32(a["gain_next"][k]), int(a["action"][k]), int(a["quiet_run"][k]))
        if not d.demod_usb:
            assert got == (_f32(d.gain), _f32(d.gain), 0, 0), (ctx, f, i, "a compress() leaf reports its stored gain", got)
        else:
            r = w["agc"][i]
            want = (_f32(r["gain_used"]), _f32(r["gain_next"]), r["action"], r["quiet_run"])
            assert got == want, (ctx, f, i, "agc record", got, want, a["gain_used"][k], r["gain_used"])
        wm = w["meters"][i]
        got_m = (int(m["n_values"][k]), int(m["sum_sq"][k]), int(m["clipped"][k]))
        assert got_m == (wm["n_values"], wm["sum_sq"], wm["clipped"]), (ctx, f, i, "meter", got_m, wm)
        if payloads:
            pay, want_pay = rx.output(i), w["payload"][i]
            if want_pay is None:
                assert pay.size == 0, (ctx, f, i, "a parked leaf has a payload")
            else:
                assert np.array_equal(_bits(pay), _bits(want_pay)), (ctx, f, i, "payload")


def _device_frames(frames):
    import torch
    dev = [torch.from_numpy(np.array(iq, np.float32)).cuda() for iq in frames]
    torch.cuda.synchronize()
    return dev


# ---- 1. exact arithmetic, closed loop -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["process", "submit"])
def test_closed_loop_exact(form):
    """Per frame, agc() and meters() equal the model's and every payload is bit for bit the model's: synchronously, and
    pipelined -- submit(f + 1); wait() -> f with two frames in flight, which a host loop cannot serve."""
    from sdrreceiver_amd.receiver import Receiver
    for k, name in enumerate(ar.TREES):
        topo, frames, sets, want = ar.reference(name)
        opts = dict(fuse_demod=k % 2 == 1, segments=k % 3)
        rx = Receiver.from_topology(topo, exact=True, agc=True, **opts)
        _set(rx, sets)
        ctx = (form, name, opts)
        if form == "process":
            for f, iq in enumerate(frames):
                rx.process(iq)
                _check(rx, topo, want[f], f, ctx)
        else:
            done = 0
            for f, iq in enumerate(frames):
                rx.submit(iq)
                if rx.in_flight() == 2:
                    rx.wait()
                    _check(rx, topo, want[done], done, ctx)
                    done += 1
            while rx.in_flight():
                rx.wait()
                _check(rx, topo, want[done], done, ctx)
                done += 1
            assert done == len(frames)
        rx.close()


DEVICE_FORMS = {
    "default": dict(),  # frame_pipeline and tail_in_levels on: the software pipeline, the demodulation riding in the levels launch
    "fuse0": dict(fuse=False),
    "pipeline": dict(pipeline=True),
    "fuse_demod": dict(fuse_demod=True),
    "fuse_demod_pipeline": dict(fuse_demod=True, pipeline=True),
    "park": dict(park=True),
}


@pytest.mark.parametrize("form", sorted(DEVICE_FORMS))
def test_closed_loop_queued_on_the_device(form):
    """The test of the ordering: the 8 frames queued back to back with sdrx_process_device and ONE fetch at the end.  The last
    frame's payloads, meters and records are those of the whole closed loop only if every step ran behind its frame's
    records and in front of every launch that read a gain for the next frame."""
    from sdrreceiver_amd.receiver import Receiver
    for name in ar.TREES:
        topo, frames, sets, want = ar.reference(name)
        rx = Receiver.from_topology(topo, exact=True, agc=True, **DEVICE_FORMS[form])
        _set(rx, sets)
        dev = _device_frames(frames)
        for t in dev:
            rx.process_device(t.data_ptr(), topo.frame)
        rx.fetch()
        _check(rx, topo, want[-1], len(frames) - 1, (form, name))
        rx.close()


# ---- 2. with park, squelch and catchup ----------------------------------------------------------------------------------------
def test_parking_catchup_and_the_setters():
    """On catchup_ref's flat tree with park, squelch, preroll and catchup on (thresholds 0): a leaf parked over two frames keeps
    gain and quiet_run; unparked it continues from the device's gain with quiet_run = 0; its caught-up frame ran with that gain
    and got no step; a set_gains in mid-run is taken up; a set_agc restarts quiet_run.  Every record against the closed loop on
    catchup_ref.CatchupTree."""
    from sdrreceiver_amd.receiver import Receiver
    topo, frames = ar.tree("small-flat")
    _, _, sets, _ = ar.reference("small-flat")
    held = next(i for i, (c, _, cls) in sets.items() if cls == "cold" and c.hold_frames == 3)
    hot = next(i for i, (c, _, cls) in sets.items() if cls == "hot")
    cold = next(i for i, (c, _, cls) in sets.items() if cls == "cold" and i != held)
    moved = float(np.float32(sets[cold][1] * 40.0))
    sched = {2: [("park", [held, hot])], 3: [("gain", cold, moved)], 4: [("unpark", [held, hot])], 6: [("agc", held, sets[held][0])]}
    model = ar.agc_tree(cr.CatchupTree)(topo)
    rx = Receiver.from_topology(topo, exact=True, agc=True, catchup=True)
    for i, (cfg, g0, _) in sets.items():
        model.set_gain(i, g0)
        model.set_agc(i, cfg)
    _set(rx, sets)
    recs = {held: [], hot: []}
    for f, iq in enumerate(frames):
        for op in sched.get(f, []):
            model.apply([op])
            if op[0] == "park":
                rx.set_active(op[1], [0] * len(op[1]))
            elif op[0] == "unpark":
                rx.set_active(op[1], [1] * len(op[1]))
            elif op[0] == "gain":
                rx.set_gains([op[1]], [op[2]])
            else:
                _set_one = op[2]
                rx.set_agc([op[1]], *[getattr(_set_one, c) for c in COLS])
        w = model.process(iq)
        rx.process(iq)
        _check(rx, topo, w, f, "park")
        for i in recs:
            recs[i].append(w["agc"][i])
        if f == 4:  # the caught-up frame 3: the model's, which ran with the gain the loop had left -- and no step followed it
            for i in (held, hot):
                c = w["caught"][i]
                assert c["frame"] == 3
                got = rx.catchup([i])
                assert (int(got["frame"][0]), int(got["sum_sq"][0]), int(got["clipped"][0])) == (3, c["meter"]["sum_sq"], c["meter"]["clipped"]), (i, got)
                assert np.array_equal(_bits(rx.preroll(i)), _bits(c["payload"])), (i, "the caught-up payload")
    # what the model run must show for the test to mean anything
    for i in (held, hot):
        r = recs[i]
        assert r[2]["action"] == r[3]["action"] == 0 and r[2]["quiet_run"] == r[3]["quiet_run"] == r[1]["quiet_run"], (i, r)
        assert _f32(r[4]["gain_used"]) == _f32(r[1]["gain_next"]), (i, "continues from the gain the device held")
    assert [r["quiet_run"] for r in recs[held]] == [1, 2, 2, 2, 1, 2, 1, 2], recs[held]
    assert recs[hot][1]["action"] == -1 and recs[hot][4]["action"] == -1
    rx.close()


# ---- 3. tolerance and robust arithmetic ----------------------------------------------------------------------------------------
TOL_TREES = ("rnd-24", "lat-sub-4352", "lat-freq", "lat-late0-2400", "small-flat", "small-deep")


@pytest.mark.parametrize("exact", [0, 2])
def test_closed_loop_tolerance(exact):
    """These arithmetics may differ from the model by an LSB in the meters, which can flip a threshold comparison, so the check
    is in two halves that do not depend on it: gain_next == agc.step(...) on the DEVICE's own meter, gain_used and quiet_run,
    for every leaf and frame; and every payload within the tolerance bound of the model run with the device's reported gains.
    The bound: streams are within 1e-5 of max|stream| (test_gpu_live_random's bar), the int16 is trunc(pre) with pre linear in
    the stream, so |got - want| <= 1 + 1e-5 max|pre| -- 1 LSB wherever nothing wraps (max|pre| < 32768), and modulo 2^16
    where the payload wrapped."""
    from sdrreceiver_amd.receiver import Receiver
    loosened = 0  # (leaf, frame) pairs whose payload wrapped: the only ones with a bound above 1 LSB
    for name in TOL_TREES:
        topo, frames, sets, _ = ar.reference(name)
        rx = Receiver.from_topology(topo, exact=exact, agc=True)
        _set(rx, sets)
        model = lr.ModelTree(topo)
        ids = list(sets)
        quiet = {i: 0 for i in ids}
        moved = 0
        for f, iq in enumerate(frames):
            rx.process(iq)
            a, m = rx.agc(ids), rx.meters(ids)
            for k, i in enumerate(ids):
                model.set_gain(i, a["gain_used"][k])
            w = model.process(iq)
            for k, i in enumerate(ids):
                dm = {"sum_sq": int(m["sum_sq"][k]), "n_values": int(m["n_values"][k]), "clipped": int(m["clipped"][k])}
                g2, q, act = agc.step(sets[i][0], quiet[i], a["gain_used"][k], dm)
                got = (_f32(a["gain_next"][k]), int(a["quiet_run"][k]), int(a["action"][k]))
                assert got == (_f32(g2), q, act), (exact, name, f, i, "the step on the device's own meter", got, (g2, q, act), dm)
                quiet[i] = q
                moved += act != 0
                if f:
                    assert _f32(a["gain_used"][k]) == last[i], (exact, name, f, i, "gain_used is the gain the step before left")
                pay, ref = rx.output(i).astype(np.int64), w["payload"][i].astype(np.int64)
                peak = float(np.abs(model.nodes[i].pre).max())
                bound = 1 + int(1e-5 * peak)
                if peak < 32768.0:  # nothing wrapped: the existing 1 LSB bar, no more
                    assert bound == 1, (exact, name, f, i, peak, bound)
                else:
                    loosened += 1
                diff = (pay - ref + 32768) % 65536 - 32768
                assert int(np.abs(diff).max()) <= bound, (exact, name, f, i, "int16", int(np.abs(diff).max()), bound)
            last = {i: _f32(a["gain_next"][k]) for k, i in enumerate(ids)}
        assert moved > 0, (exact, name)
        rx.close()
    print(f"exact = {exact}: {loosened} wrapped (leaf, frame) pairs compared with a bound above 1 LSB")


# ---- 4. off means unchanged ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse_demod", [False, True])
def test_every_leaf_off_is_meter_alone(fuse_demod):
    """agc = 1 with every hi_ms 0 against meter = 1: payloads, meters, streams and what the callback saw identical, frames
    queued on the device included; the step reports the stored gain and action 0."""
    from sdrreceiver_amd.receiver import Receiver
    for name in ("rnd-24", "lat-inner", "small-flat"):
        topo, frames = ar.tree(name)
        leaves = topo.leaves_in_publish_order()
        a = Receiver.from_topology(topo, exact=True, agc=True, keep_streams=True, fuse_demod=fuse_demod)
        b = Receiver.from_topology(topo, exact=True, meter=True, keep_streams=True, fuse_demod=fuse_demod)
        for f, iq in enumerate(frames[:4]):
            a.process(iq)
            b.process(iq)
            assert a.published == b.published, (name, f)
            ma, mb = a.meters(leaves), b.meters(leaves)
            for key in ("frame", "n_values", "sum_sq", "clipped"):
                assert np.array_equal(ma[key], mb[key]), (name, f, key)
            assert np.array_equal(_bits(ma["peak"]), _bits(mb["peak"])), (name, f)
            for i in range(len(topo.vfos)):
                assert np.array_equal(_bits(a.stream(i)), _bits(b.stream(i))), (name, f, i, "stream")
            st = a.agc(leaves)
            assert not st["action"].any() and not st["quiet_run"].any() and not st["hi_ms"].any()
            assert [_f32(v) for v in st["gain_used"]] == [_f32(v) for v in st["gain_next"]] == [_f32(topo.vfos[i].gain) for i in leaves]
        dev = _device_frames(frames[4:])
        for t in dev:
            a.process_device(t.data_ptr(), topo.frame)
            b.process_device(t.data_ptr(), topo.frame)
        a.fetch()
        b.fetch()
        assert a.published == b.published, (name, "device frames")
        a.close()
        b.close()


def test_option_off():
    """agc = 0: both calls return SDRX_ESTATE (before any id or value is looked at), with "meter" on or off."""
    from sdrreceiver_amd.receiver import Receiver
    topo, frames = ar.tree("small-deep")
    for meter in (False, True):
        rx = Receiver.from_topology(topo, exact=True, meter=meter)
        rx.process(frames[0])
        for call in (lambda: rx.agc([0]), lambda: rx.agc([999]), lambda: rx.set_agc([999], 5, 4, 9, 0, 0.0, 2.0, -1.0, 0.0)):
            with pytest.raises(SdrxError) as e:
                call()
            assert e.value.code == _lib.SDRX_ESTATE and '"agc" is off' in str(e.value), str(e.value)
        rx.close()


# ---- 5. validation -------------------------------------------------------------------------------------------------------------
def test_validation_changes_nothing():
    """Every SDRX_EINVAL of the list leaves settings, quiet_run and gain as they were -- the loop goes on as the model's --
    and the checks come in the order of DESIGN.md 4l: option, list shape, ids (range, leaf, listed once), values, frames in
    flight."""
    from sdrreceiver_amd.receiver import Receiver
    topo, frames, sets, want = ar.reference("small-flat")
    leaves = topo.leaves_in_publish_order()
    usb = list(sets)
    iq_leaf = next(i for i in leaves if not topo.vfos[i].demod_usb)
    inner = next(i for i in range(len(topo.vfos)) if topo.children(i))
    good = sets[usb[0]][0]
    r = dataclasses.replace
    bad_cfgs = [r(good, silent_ms=good.lo_ms + 1), r(good, lo_ms=good.hi_ms + 1, silent_ms=0), r(good, hi_ms=(1 << 30) + 1), r(good, up=0.5),
                r(good, down=0.0), r(good, down=1.5), r(good, gain_min=0.0), r(good, gain_min=-1.0), r(good, gain_min=2.0, gain_max=1.0),
                r(good, up=float("inf")), r(good, down=float("nan")), r(good, gain_min=float("nan")), r(good, gain_max=float("inf"))]

    def call(ids, cfgs):
        return lambda: rx.set_agc(ids, *[[getattr(c, k) for c in cfgs] for k in COLS])

    rx = Receiver.from_topology(topo, exact=True, agc=True)
    _set(rx, sets)
    other = r(good, lo_ms=good.lo_ms + 1)  # a good setting riding in front of the bad one: the call is atomic
    for f, iq in enumerate(frames):
        if f == 3:
            for bad in bad_cfgs:
                with pytest.raises(SdrxError) as e:
                    call([usb[1], usb[0]], [other, bad])()
                assert e.value.code == _lib.SDRX_EINVAL, (bad, str(e.value))
            with pytest.raises(SdrxError) as e:  # a compress() leaf with hi_ms > 0
                call([usb[0], iq_leaf], [other, good])()
            assert e.value.code == _lib.SDRX_EINVAL and "USB" in str(e.value), str(e.value)
            for ids, what in (([usb[0], 999], "bad vfo id"), ([usb[0], inner], "has children"), ([usb[0], usb[0]], "listed twice")):
                with pytest.raises(SdrxError) as e:  # (the id is wrong AND the value is: the id decides)
                    call(ids, [other, bad_cfgs[0]])()
                assert e.value.code == _lib.SDRX_EINVAL and what in str(e.value), str(e.value)
            call([iq_leaf], [r(good, hi_ms=0, up=float("nan"))])()  # hi_ms 0: accepted as it is, on any leaf, and stored
            st = rx.agc([iq_leaf])
            assert int(st["hi_ms"][0]) == 0 and int(st["lo_ms"][0]) == good.lo_ms and np.isnan(st["up"][0])
            call([], [])()  # an empty list does nothing
        rx.process(iq)
        _check(rx, topo, want[f], f, "validation")
        st = rx.agc(usb)
        for k, i in enumerate(usb):
            assert tuple(int(st[c][k]) for c in COLS[:4]) == tuple(getattr(sets[i][0], c) for c in COLS[:4]), (f, i)
            assert tuple(_f32(st[c][k]) for c in COLS[4:]) == tuple(_f32(getattr(sets[i][0], c)) for c in COLS[4:]), (f, i)
    # values before frames in flight: with a frame in flight a bad value is SDRX_EINVAL, a good one SDRX_ESTATE; the getter serves
    # the delivered frame meanwhile
    rx.submit(frames[0])
    with pytest.raises(SdrxError) as e:
        call([usb[0]], [bad_cfgs[0]])()
    assert e.value.code == _lib.SDRX_EINVAL
    with pytest.raises(SdrxError) as e:
        call([usb[0]], [good])()
    assert e.value.code == _lib.SDRX_ESTATE and "not yet delivered" in str(e.value), str(e.value)
    assert int(rx.agc(usb)["frame"][0]) == len(frames) - 1
    rx.wait()
    assert int(rx.agc(usb)["frame"][0]) == len(frames)
    rx.close()


# ---- 6. group ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rnd-24", "small-flat"])
def test_group_of_three(name):
    """sdrx_group_set_agc / sdrx_group_get_agc with ids of the whole tree, three members on one GPU: records, meters and
    payloads of every frame are the closed loop's, i.e. the single context's; `frame` counts the group's frames."""
    from sdrreceiver_amd.receiver import Group
    topo, frames, sets, want = ar.reference(name)
    g = Group.from_topology(topo, [0, 0, 0], agc=1)
    _set(g, sets)
    for f, iq in enumerate(frames):
        g.process(iq)
        _check(g, topo, want[f], f, ("group", name))
    with pytest.raises(SdrxError) as e:
        g.set_agc([list(sets)[0]], 5, 4, 0, 0, 2.0, 0.5, 1.0, 2.0)
    assert e.value.code == _lib.SDRX_EINVAL
    g.close()
