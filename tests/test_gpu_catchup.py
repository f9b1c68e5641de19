"""Unpark with catch-up on the device (option "catchup", sdrx_set_active, sdrx_get_catchup and the group forms) against the
model of tests/catchup_ref.py, which tests/test_catchup_model.py pins to the oracle: a leaf unparked before frame K that was
parked in K-1 is a new vfo fed its parent's stream from K-1 on, and frame K delivers its payload of K-1 first."""
import functools

import numpy as np
import pytest

import catchup_ref as cr
import retune_ref as rr
import watch_ref as wr
from sdrreceiver_amd import _lib, watch
from sdrreceiver_amd.receiver import Group, Receiver, SdrxError
from test_gpu_live_random import REL_TOL, _int8_within_one
from test_gpu_park import Drive, _apply_ops

pytestmark = pytest.mark.gpu

METER_KEYS = ("frame", "n_values", "sum_sq", "clipped", "peak")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _close(topo, i, got, ref):
    """the project's bar for the tolerance arithmetics: int16 within 1 LSB, int8 within 1 (modulo the wrap)"""
    d = topo.vfos[i]
    if got.size != ref.size:
        return False
    if d.demod_usb:
        return int(np.abs(got.astype(np.int32) - ref.astype(np.int32)).max()) <= 1
    return _int8_within_one(got, ref, d.cstyle)


def _meter_of(m, k):
    return (int(m["n_values"][k]), int(m["sum_sq"][k]), int(m["clipped"][k]), np.float32(m["peak"][k]).view(np.uint32))


def _want_meter(m):
    return (int(m["n_values"]), int(m["sum_sq"]), int(m["clipped"]), np.float32(m["peak"]).view(np.uint32))


def _run(key, mode, exact=True, keep_streams=True, **opts):
    """keep_streams = False is the library's default: a leaf whose late decimation or demodulation is fused then has no stream
    buffer (sdrx_get_stream fails for it: nothing to compare), every other stream is held to the model as before."""
    topo, want, kinds, gates = cr.reference(key)
    sched = cr.SCHED[key]
    leaves = topo.leaves_in_publish_order()
    tag = (key, mode, exact, keep_streams, opts)
    rx = Receiver.from_topology(topo, exact=exact, keep_streams=keep_streams, catchup=True, **opts)
    applied, seen = set(), []

    def apply(f):
        if f not in sched or f in applied:
            return
        _apply_ops(rx, sched[f])
        applied.add(f)
        # sdrx_get_catchup answers as soon as sdrx_set_active has returned: before frame f runs (and, under "device", before
        # frame f - 1 is fetched)
        cu = rx.catchup(leaves)
        for k, i in enumerate(leaves):
            c = want[f]["caught"].get(i)
            if c is None:
                assert (int(cu["frame"][k]), _meter_of(cu, k)) == (-1, (0, 0, 0, 0)), (tag, f, i, "not caught up")
                continue
            assert int(cu["frame"][k]) == c["frame"] and int(cu["n_values"][k]) == c["meter"]["n_values"], (tag, f, i)
            if exact is True:
                assert _meter_of(cu, k) == _want_meter(c["meter"]), (tag, f, i, "the meter of the caught-up frame")

    def check(f):
        w = want[f]
        pub, n_open, n_pre, nbytes = cr.delivery(topo, want, gates, f)
        if exact is True:
            assert rx.published == pub, (tag, f, "callbacks: order, pre-roll first, bytes")
        else:
            assert [(t, r, len(b)) for t, r, b in rx.published] == [(t, r, len(b)) for t, r, b in pub], (tag, f, "callbacks")
        eg, pc = rx.egress(), rx.preroll_count()
        assert (eg["frame"], eg["n_open"], eg["n_leaves"], eg["payload_bytes_copied"]) == (f, n_open, len(leaves), nbytes), (tag, f, eg)
        assert pc["n_preroll"] == n_pre, (tag, f, pc)
        m = rx.meters(leaves)
        for k, i in enumerate(leaves):
            pay, pre = rx.output(i), rx.preroll(i)
            ref_pay = w["payload"][i]
            ref_pre = cr.preroll_of(want, i, f) if gates[i][f]["pre"] else None
            assert int(m["frame"][k]) == f
            if ref_pay is None:  # parked in f -- also for a K-1 fetched after the unpark: the reports stay "parked"
                assert pay.size == 0 and pre.size == 0, (tag, f, i, "a parked leaf is delivered")
                assert _meter_of(m, k) == (0, 0, 0, 0), (tag, f, i, "a parked leaf has a meter")
                continue
            if exact is True:
                assert np.array_equal(_bits(pay), _bits(ref_pay)), (tag, f, i, "payload")
                assert _meter_of(m, k) == _want_meter(w["meters"][i]), (tag, f, i, "meter")
                assert pre.size == (0 if ref_pre is None else ref_pre.size), (tag, f, i, "pre-roll")
                assert ref_pre is None or np.array_equal(_bits(pre), _bits(ref_pre)), (tag, f, i, "pre-rolled payload")
            else:
                assert _close(topo, i, pay, ref_pay), (tag, f, i, "payload")
                assert pre.size == (0 if ref_pre is None else ref_pre.size) and (ref_pre is None or _close(topo, i, pre, ref_pre)), (tag, f, i, "pre-roll")
        if rx.in_flight() == 0:  # (device read-backs wait for the frames in flight)
            for i, z in w["streams"].items():
                got = rx.stream(i, missing_ok=True)
                if z is None:
                    assert got is None, (tag, f, i, "a parked leaf has a stream")
                elif got is None:
                    assert not keep_streams, (tag, f, i, "keep_streams keeps every stream")
                elif exact is True:
                    assert np.array_equal(_bits(got), _bits(z)), (tag, f, i, "stream")
                else:
                    assert float(np.abs(got - z).max()) <= REL_TOL * float(np.abs(z).max()), (tag, f, i, "stream")
        seen.append(f)

    Drive(rx, topo, cr.frames(key), mode, sched.keys()).run(apply, check)
    queued = {f for f in range(cr.N_FRAMES) if mode == "device" and f + 2 in sched and f not in sched}  # (Drive leaves them in the pipeline)
    assert set(range(2, cr.N_FRAMES)) - queued <= set(seen), seen
    descs = want[-1]["descs"]
    for i in leaves:
        if want[-1]["since"][i]:
            L = topo.vfos[i].fs
            assert np.array_equal(_bits(rx.nco(i, L - 64, 64)), _bits(rr.table(L, descs[i].mixer_freq)[L - 64:])), (tag, i, "nco")
    st = rx.active(leaves)
    assert [int(v) for v in st["since_frame"]] == [want[-1]["since"][i] for i in leaves]  # K, not K-1
    rx.close()


CASES_EXACT = [
    ("flat", "process", dict()),
    ("flat", "submit", dict(fuse_demod=True, tail_in_levels=False)),
    ("flat", "device", dict(fuse_demod=True, tail_in_levels=True)),
    ("flat", "device", dict(fuse_demod=False, tail_in_levels=True, fuse_late=False)),
    ("flat", "device", dict(fuse_demod=False, tail_in_levels=False)),
    ("flat", "process", dict(fuse=False, frame_pipeline=False, fuse_late=False)),
    ("flat", "submit", dict(pipeline=True)),
    ("flat", "submit", dict(pipeline=True, fuse_demod=True)),
    ("flat", "process", dict(segments=1)),
    ("flat", "device", dict(segments=2, fuse_demod=True)),
    ("flat", "submit", dict(segments=3)),
    ("flat", "process", dict(segments=4, fuse_late=False)),
    ("flat", "device", dict(segments=5)),
    ("deep", "process", dict()),
    ("deep", "submit", dict(fuse_demod=True)),
    ("deep", "device", dict(fuse_demod=True, tail_in_levels=True)),
    ("deep", "device", dict(frame_pipeline=False)),
]


@pytest.mark.parametrize("key,mode,opts", CASES_EXACT, ids=[f"{k}-{m}-{'-'.join(f'{a}{int(b)}' for a, b in o.items())}"
                                                            for k, m, o in CASES_EXACT])
def test_catchup_exact(key, mode, opts):
    """exact = 1, bit for bit, through sdrx_process, sdrx_submit / sdrx_wait and queued sdrx_process_device (the sdrx_set_active
    call made before the fetch), in the launch forms tests/test_gpu_park.py rotates and with segments 0 .. 5."""
    _run(key, mode, **opts)


@pytest.mark.parametrize("exact", [False, 2])
@pytest.mark.parametrize("key", ["flat", "deep"])
def test_catchup_tolerance_arithmetics(key, exact):
    """exact = 0 and 2: within 1e-5 of max|model stream| and 1 LSB of the same model."""
    _run(key, "process", exact=exact)


def _collect(rx, topo, frames, sched):
    leaves = topo.leaves_in_publish_order()
    out = []
    for f, iq in enumerate(frames):
        _apply_ops(rx, sched.get(f, []))
        rx.process(iq)
        m = rx.meters(leaves)
        out.append(dict(pub=list(rx.published), pay={i: rx.output(i) for i in leaves}, pre={i: rx.preroll(i) for i in leaves},
                        z={i: rx.stream(i, missing_ok=True) for i in range(len(topo.vfos))},
                        meter={i: [m[k][n].tolist() for k in METER_KEYS] for n, i in enumerate(leaves)}))
    return out


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(_bits(a), _bits(b)))


def _launches(rx):
    return {k: v["launches"] for k, v in rx.kernel_times().items()}


def test_leaves_not_named_and_frames_without_a_catchup_equal_the_option_off():
    """The same schedule with catchup = 1 and with catchup = 0, park = 1, preroll = 1: leaf 1, which is never named, and the
    main's stream are bit for bit the same in every frame, and so is every leaf in the frames before the first catch-up.  And a
    tree with catchup = 1 on which nothing is ever caught up -- parks, a K = 0 unpark, restarts -- equals the option off in
    every frame; device_bytes are equal."""
    topo, want, kinds, _ = cr.reference("flat")
    frames, sched = cr.frames("flat"), cr.SCHED["flat"]
    leaves = topo.leaves_in_publish_order()
    res, dev = {}, {}
    for cu in (False, True):
        rx = Receiver.from_topology(topo, keep_streams=True, park=True, preroll=True, catchup=cu)
        res[cu] = _collect(rx, topo, frames, sched)
        dev[cu] = rx.stats()["device_bytes"]
        rx.close()
    assert dev[True] == dev[False]
    first = min(f for i in leaves for f, s in kinds[i].items() if "c" in s)
    for f, (a, b) in enumerate(zip(res[False], res[True])):
        if f < first:
            assert a["pub"] == b["pub"], f
        for i in [1] + ([] if f >= first else leaves):
            assert _same(a["pay"][i], b["pay"][i]) and _same(a["pre"][i], b["pre"][i]) and _same(a["z"][i], b["z"][i]), (f, i)
            assert a["meter"][i] == b["meter"][i], (f, i)
        assert _same(a["z"][0], b["z"][0]), f
    # nothing caught up: parks and restarts only (K = 0 unpark, park + unpark with no frame between)
    quiet = {0: [("park", [2]), ("unpark", [2])], 2: [("park", [3, 9])], 3: [("park", [4]), ("unpark", [4])]}
    res = {}
    for cu in (False, True):
        rx = Receiver.from_topology(topo, keep_streams=True, park=True, preroll=True, catchup=cu, fuse_demod=True)
        res[cu] = _collect(rx, topo, frames[:5], quiet)
        if cu:
            assert [int(v) for v in rx.catchup(leaves)["frame"]] == [-1] * len(leaves)
        rx.close()
    for f, (a, b) in enumerate(zip(res[False], res[True])):
        assert a["pub"] == b["pub"] and a["meter"] == b["meter"], f
        for i in leaves:
            assert _same(a["pay"][i], b["pay"][i]) and _same(a["pre"][i], b["pre"][i]), (f, i)
        for i in range(len(topo.vfos)):
            assert _same(a["z"][i], b["z"][i]), (f, i)


def test_option_off_is_the_tree_that_was_never_asked():
    """catchup = 0 set explicitly against a context that never heard of the option: device_bytes, launch counts and payloads;
    sdrx_get_catchup returns SDRX_ESTATE."""
    topo = cr.flat_tree()
    frames = cr.frames("flat")[:3]
    got = {}
    for asked in (False, True):
        if not asked:
            rx = Receiver.from_topology(topo, park=True, preroll=True, keep_streams=True)
        else:
            rx = Receiver(park=True, preroll=True, keep_streams=True)
            assert rx.L.sdrx_set_option(rx.h, b"catchup", 0) == 0
            for d in topo.vfos:
                rx.add_vfo(d)
            rx.finalize()
        rx.enable_kernel_timing(True)
        rx.set_active([2], [0])
        rec = []
        for f, iq in enumerate(frames):
            if f == 2:
                rx.set_active([2], [1])
            rx.process(iq)
            rec.append((list(rx.published), [rx.preroll(i).tobytes() for i in topo.leaves_in_publish_order()]))
        got[asked] = (rec, rx.stats()["device_bytes"], _launches(rx))
        with pytest.raises(SdrxError) as e:
            rx.catchup([2])
        assert e.value.code == _lib.SDRX_ESTATE
        rx.close()
    assert got[False] == got[True]
    assert all(p == b"" for _, pre in got[True][0] for p in pre)  # (nothing is pre-rolled at threshold 0 without the option)


def test_threshold_above_the_level_of_k_drops_the_caught_up_payload_and_parking_again_discards_it():
    topo, want, _, _ = cr.reference("flat")
    frames = cr.frames("flat")
    rx = Receiver.from_topology(topo, catchup=True)
    rx.set_active([2, 3], [0, 0])
    rx.process(frames[0])
    rx.process(frames[1])
    rx.set_squelch([2], [1 << 62], [3])  # closed in K whatever it holds; hang_frames does not help
    rx.set_active([2, 3], [1, 1])
    cu = rx.catchup([2, 3])
    assert [int(v) for v in cu["frame"]] == [1, 1] and int(cu["sum_sq"][0]) > 0
    rx.set_active([3], [0])               # parked again before K: discarded
    assert [int(v) for v in rx.catchup([2, 3])["frame"]] == [1, -1]
    rx.process(frames[2])
    assert rx.output(2).size == 0 and rx.preroll(2).size == 0 and rx.output(3).size == 0 and rx.preroll(3).size == 0
    assert rx.preroll_count()["n_preroll"] == 0
    rx.set_squelch([2], [0], [0])
    rx.process(frames[3])                 # opens in K + 1: the ordinary rule pre-rolls frame K, never K - 1
    assert rx.preroll(2).size == rx.output(2).size > 0
    assert int(rx.catchup([2])["frame"][0]) == 1  # (its present active state still began with that catch-up)
    rx.close()


def test_group_of_two_members():
    topo, want, _, gates = cr.reference("flat")
    leaves = topo.leaves_in_publish_order()
    g = Group.from_topology(topo, [0, 0], catchup=1)
    for f, iq in enumerate(cr.frames("flat")):
        _apply_ops(g, cr.SCHED["flat"].get(f, []))
        cu = g.catchup(leaves)
        for k, i in enumerate(leaves):
            c = want[f]["caught"].get(i)
            assert int(cu["frame"][k]) == (-1 if c is None else c["frame"]), (f, i)
            assert c is None or _meter_of(cu, k) == _want_meter(c["meter"]), (f, i)
        g.process(iq)
        pub, n_open, n_pre, nbytes = cr.delivery(topo, want, gates, f)
        assert sorted(g.published) == sorted(pub), f  # (each member publishes its own leaves in order)
        for i in leaves:
            ref = want[f]["payload"][i]
            assert g.output(i).size == 0 if ref is None else np.array_equal(_bits(g.output(i)), _bits(ref)), (f, i)
            if gates[i][f]["pre"]:
                assert np.array_equal(_bits(g.preroll(i)), _bits(cr.preroll_of(want, i, f))), (f, i)
            else:
                assert g.preroll(i).size == 0, (f, i)
        assert g.preroll_count()["n_preroll"] == n_pre and g.egress()["payload_bytes_copied"] == nbytes, f
    with pytest.raises(SdrxError) as e:
        g.catchup([0])
    assert e.value.code == _lib.SDRX_EINVAL
    g.close()


def test_errors():
    topo = cr.flat_tree()
    rx = Receiver(catchup=True)
    for d in topo.vfos:
        rx.add_vfo(d)
    ids = np.array([2], np.int32)
    out = (_lib.MeterC * 2)()
    assert rx.L.sdrx_get_catchup(rx.h, ids.ctypes.data, 1, out) == _lib.SDRX_ESTATE  # before finalize
    rx.finalize()
    for bad in ([99], [-1], [0]):  # out of range; a VFO with children
        with pytest.raises(SdrxError) as e:
            rx.catchup(bad)
        assert e.value.code == _lib.SDRX_EINVAL, bad
    assert rx.L.sdrx_get_catchup(rx.h, ids.ctypes.data, -1, out) == _lib.SDRX_EINVAL
    assert rx.L.sdrx_get_catchup(rx.h, ids.ctypes.data, 1, None) == _lib.SDRX_EINVAL
    assert rx.L.sdrx_get_catchup(rx.h, None, 0, None) == 0  # n == 0 does nothing
    assert int(rx.catchup([2])["frame"][0]) == -1           # good from sdrx_finalize on
    rx.set_active([2], [0])                                  # the option implies "park" ...
    rx.process(cr.frames("flat")[0])
    assert rx.preroll(2).size == 0 and rx.meters([2])["n_values"][0] == 0  # ... "preroll", "squelch" and "meter"
    rx.submit(cr.frames("flat")[1])
    with pytest.raises(SdrxError) as e:  # a frame in flight: sdrx_set_active's rule is unchanged
        rx.set_active([2], [1])
    assert e.value.code == _lib.SDRX_ESTATE
    rx.wait()
    rx.close()


def test_a_burst_that_trips_the_watch_is_delivered_from_its_first_frame():
    """A tone begins mid-frame f = 2 in the band of a parked, watched leaf.  The synchronous loop process -> watch -> wake_list
    -> set_active delivers, with frame 3, a pre-roll whose samples are the model's frame 2: a fresh node fed the main's stream of
    frame 2.  With catchup = 0 the same loop delivers nothing of frame 2."""
    topo = wr.watch_tree()
    leaf, f0 = 3, 2
    raw_hz = wr.tone_for(topo, leaf)
    frames = []
    for f in range(4):
        iq = wr.tone_frame(topo, raw_hz, seed=40 + f, start=f * topo.frame)
        quiet = np.random.default_rng(40 + f).integers(-1, 2, 2 * topo.frame).astype(np.float32)
        if f < f0:
            iq = quiet
        elif f == f0:
            iq[: topo.frame] = quiet[: topo.frame]  # (interleaved: the first half of the frame's samples)
        frames.append(iq)
    heard = {}
    for cu in (True, False):
        rx = Receiver.from_topology(topo, watch=True, park=True, preroll=True, keep_streams=True, catchup=cu)
        ids = list(range(1, 9))
        rx.set_active(ids, [0] * len(ids))
        rx.set_watch(ids, [1] * len(ids))
        woke_at, got_pre, fresh, ref = None, None, rr.Node(topo.vfos[leaf]), None
        for f, iq in enumerate(frames):
            rx.process(iq)
            if woke_at is None:
                wake = watch.wake_list(ids, rx.watch(ids), 100.0)
                if wake:
                    assert wake == [leaf] and f == f0, (f, wake)
                    fresh.process(rx.stream(0))
                    ref = fresh.payload()
                    rx.set_active(wake, [1])
                    woke_at = f
            elif f == woke_at + 1:
                got_pre = rx.preroll(leaf)
                assert rx.output(leaf).size > 0
        assert woke_at == f0
        heard[cu] = got_pre
        if cu:
            assert np.array_equal(_bits(got_pre), _bits(ref)), "the pre-roll of frame f + 1 is the model's frame f"
            assert int(rx.catchup([leaf])["sum_sq"][0]) == int((ref.astype(np.int64) ** 2).sum())
        rx.close()
    assert heard[False].size == 0
    assert int((heard[True].astype(np.int64) ** 2).sum()) > 0 == int((heard[False].astype(np.int64) ** 2).sum())
