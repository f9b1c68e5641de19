"""Device-side wake on the device (option "wake", sdrx_set_wake / sdrx_get_wake and the group forms) against the model of
tests/wake_ref.py, whose decisions tests/test_wake_model.py shows to be a factor 4 from every threshold: a leaf under control
runs in exactly the frames the rule allows, decided on the device from the spectrum of that very frame, and is a new vfo in the
frame it wakes in -- through sdrx_process, through sdrx_submit with two frames in flight and through queued sdrx_process_device,
with no control call between the frames."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import agc_ref
import retune_ref as rr
import wake_ref as kr
import watch_ref as wr
from sdrreceiver_amd import _lib, agc, wake, watch
from sdrreceiver_amd.receiver import Group, Receiver, SdrxError
from test_gpu_live_random import REL_TOL, _int8_within_one
from test_park_model import gate_with_parking

pytestmark = pytest.mark.gpu

WAKE_KEYS = ("frame", "since_frame", "active", "hot", "hold_left", "controlled")
FETCH_AT = {"watch": (2, 5, 7, 8), "deep": (0, 2, 4, 6, 7), "flat": (1, 3, 4, 6)}  # "device": frames queued up to each, then one fetch


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


def set_wake(rx, cfgs):
    ids = sorted(cfgs)
    rx.set_wake(ids, [cfgs[i].min_band_pwr for i in ids], [cfgs[i].contrast_q8 for i in ids], [cfgs[i].hold_frames for i in ids],
                [cfgs[i].on for i in ids])


def start(rx, scn):
    """The calls before frame 0: park, watch, wake.  No control call follows."""
    if scn.parked0:
        rx.set_active(list(scn.parked0), [0] * len(scn.parked0))
    rx.set_watch(scn.controlled, [1] * len(scn.controlled))
    set_wake(rx, scn.cfgs)


def make(scn, exact=True, keep_streams=True, meter=True, **opts):
    rx = Receiver.from_topology(scn.topo, exact=exact, keep_streams=keep_streams, meter=meter, wake=True, **opts)
    start(rx, scn)
    return rx


def check_wake_records(rx, leaves, w, f, tag):
    k = rx.wake(leaves)
    for n, i in enumerate(leaves):
        got = {key: int(k[key][n]) for key in WAKE_KEYS}
        ref = w["wake"].get(i)
        if ref is None:  # not under control: the host's bookkeeping
            ref = dict(frame=f, since_frame=w["since"][i], active=w["active"][i], hot=0, hold_left=0, controlled=0)
        assert got == ref, (tag, f, i, "wake record", got, ref)
    st = rx.active(leaves)
    assert [int(v) for v in st["active"]] == [w["active"][i] for i in leaves], (tag, f, "sdrx_get_active: active")
    assert [int(v) for v in st["since_frame"]] == [w["since"][i] for i in leaves], (tag, f, "sdrx_get_active: since_frame")


def check_frame(rx, scn, w, f, tag, exact=True, keep_streams=True, meter=True, squelch=False):
    topo = scn.topo
    leaves = topo.leaves_in_publish_order()
    if not squelch:
        if exact is True:
            assert rx.published == w["published"], (tag, f, "callbacks: who, in which order, which bytes")
        else:
            assert [(t, r, len(b)) for t, r, b in rx.published] == [(t, r, len(b)) for t, r, b in w["published"]], (tag, f, "callbacks")
        eg = rx.egress()
        assert (eg["frame"], eg["n_open"], eg["n_leaves"]) == (f, sum(w["active"][i] for i in leaves), len(leaves)), (tag, f, eg)
    m = rx.meters(leaves) if meter else None
    for k, i in enumerate(leaves):
        ref = w["payload"][i]
        if ref is None:
            if not squelch:
                assert rx.output(i).size == 0, (tag, f, i, "a parked leaf is delivered")
            assert m is None or _meter_of(m, k) == (0, 0, 0, 0), (tag, f, i, "a parked leaf has a meter")
            continue
        if squelch:
            continue
        pay = rx.output(i)
        if exact is True:
            assert np.array_equal(_bits(pay), _bits(ref)), (tag, f, i, "payload", pay.size, ref.size)
            assert m is None or (int(m["frame"][k]), _meter_of(m, k)) == (f, _want_meter(w["meters"][i])), (tag, f, i, "meter")
        else:
            assert _close(topo, i, pay, ref), (tag, f, i, "payload")
    check_wake_records(rx, leaves, w, f, tag)
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


def drive(rx, scn, mode, check, before=None, fetch_at=None):
    """No control call between the frames.  "process": sdrx_process; "submit": sdrx_submit with two frames in flight; "device":
    sdrx_process_device queued back to back, fetched only at `fetch_at` (FETCH_AT).  `before`: frame -> a control call made
    before that frame, once every frame before it is delivered (a queued run fetches the frame before it)."""
    frames, seen = scn.frames, []
    before = before or {}
    fetch_at = FETCH_AT[scn.name] if fetch_at is None else fetch_at
    if mode == "process":
        for f, iq in enumerate(frames):
            if f in before:
                before[f]()
            rx.process(iq)
            check(f)
            seen.append(f)
    elif mode == "submit":
        for f, iq in enumerate(frames):
            if f in before:
                while rx.in_flight():
                    rx.wait()
                    check(len(seen))
                    seen.append(len(seen))
                before[f]()
            rx.submit(iq)
            if rx.in_flight() == 2:
                rx.wait()
                check(len(seen))
                seen.append(len(seen))
        while rx.in_flight():
            rx.wait()
            check(len(seen))
            seen.append(len(seen))
    else:
        import torch
        dev = [torch.from_numpy(np.array(iq)).cuda() for iq in frames]
        torch.cuda.synchronize()
        for f in range(len(frames)):
            if f in before:
                assert seen and seen[-1] == f - 1, (f, "a control call behind an unfetched frame")
                before[f]()
            rx.process_device(dev[f].data_ptr(), scn.topo.frame)
            if f in fetch_at:
                rx.fetch()
                check(f)
                seen.append(f)
    return seen


def _run(name, mode, exact=True, keep_streams=True, meter=True, **opts):
    scn, want = kr.reference(name)
    tag = (name, mode, exact, keep_streams, opts)
    rx = make(scn, exact=exact, keep_streams=keep_streams, meter=meter, **opts)
    seen = drive(rx, scn, mode, lambda f: check_frame(rx, scn, want[f], f, tag, exact, keep_streams, meter))
    assert seen == (list(FETCH_AT[name]) if mode == "device" else list(range(len(scn.frames)))), seen
    if exact is True:  # a wake replays no oscillator: the checkpoints are those of finalize
        for i in scn.controlled:
            L = scn.topo.vfos[i].fs
            assert np.array_equal(_bits(rx.nco(i, L - 64, 64)), _bits(rr.table(L, scn.topo.vfos[i].mixer_freq)[L - 64:])), (tag, i, "nco")
    rx.close()


# 1 and 3: every path, in the launch forms the issue lists.  "deep" is the per-level fallback (a parent-less leaf, a level-1
# leaf beside level-2 leaves); "flat" the leaf shapes
CASES_EXACT = [
    ("watch", "process", dict()),
    ("watch", "submit", dict()),
    ("watch", "device", dict(tail_in_levels=True)),
    ("watch", "device", dict(frame_pipeline=False)),
    ("watch", "device", dict(tail_in_levels=False, fuse_late=False)),
    ("watch", "process", dict(fuse=False)),
    ("watch", "device", dict(fuse=False)),
    ("watch", "submit", dict(pipeline=True)),
    ("watch", "submit", dict(fuse_late=False, keep_streams=False)),
    ("watch", "process", dict(segments=2)),
    ("watch", "device", dict(segments=5)),
    ("watch", "submit", dict(meter=False)),
    ("flat", "process", dict()),
    ("flat", "submit", dict(fuse_demod=True)),
    ("flat", "submit", dict(pipeline=True, fuse_demod=True)),
    ("flat", "device", dict(tail_in_levels=True)),
    ("flat", "device", dict(fuse_demod=True, tail_in_levels=True)),
    ("flat", "device", dict(fuse_demod=True, frame_pipeline=False, keep_streams=False)),
    ("flat", "process", dict(fuse=False, fuse_late=False)),
    ("flat", "submit", dict(segments=2)),
    ("flat", "device", dict(segments=5, fuse_demod=True)),
    ("flat", "process", dict(keep_streams=False)),
    ("deep", "process", dict()),
    ("deep", "submit", dict(fuse_demod=True)),
    ("deep", "submit", dict(pipeline=True)),
    ("deep", "device", dict(tail_in_levels=True)),
    ("deep", "device", dict(fuse_demod=True, frame_pipeline=False)),
    ("deep", "process", dict(segments=2, fuse=False)),
]


@pytest.mark.parametrize("name,mode,opts", CASES_EXACT, ids=[f"{k}-{m}-{'-'.join(f'{a}{int(b)}' for a, b in o.items())}" for k, m, o in CASES_EXACT])
def test_wake_exact(name, mode, opts):
    """exact = 1, bit for bit against the model: payloads, kept streams, meters, wake records, sdrx_get_active, the callback
    sequence."""
    _run(name, mode, **opts)


# 5
@pytest.mark.parametrize("exact", [False, 2])
@pytest.mark.parametrize("name,mode", [("watch", "submit"), ("flat", "device"), ("deep", "process")])
def test_wake_tolerance_arithmetics(name, mode, exact):
    """exact = 0 and 2: the same decisions and records; payloads within 1 LSB, streams within 1e-5 of max|model stream|."""
    _run(name, mode, exact=exact)


# 2
def test_a_burst_that_begins_mid_frame_is_heard_from_its_own_frame_on():
    """Through submit / wait with two frames in flight and no host call: frame 2's OWN output of leaf 3 is that of a fresh node
    fed the main's stream of frame 2; with hold_frames = 1 the leaf is delivered one frame past the burst's last hot frame, then
    parked.  The same frames without the option, driven by the watch -> wake_list -> set_active loop, deliver nothing of frame 2."""
    scn, want = kr.reference("watch")
    leaf = 3
    assert scn.cfgs[leaf] == wake.Cfg(1e8, 25600, 1)
    fresh = rr.Node(scn.topo.vfos[leaf])
    rx = make(scn)
    out = {}
    drive(rx, scn, "submit", lambda f: out.__setitem__(f, (rx.output(leaf), int(rx.wake([leaf])["hot"][0]))))
    for f in range(2):
        assert out[f][0].size == 0, (f, "parked before the burst")
    for f in (2, 3, 4, 5):
        fresh.process(kr.sources("watch")[f][0])
        assert np.array_equal(out[f][0], fresh.payload()), (f, "not a fresh node on the main's stream from frame 2 on")
    assert np.abs(out[2][0].astype(np.int32)).max() > 100, "the tone is in frame 2's own output"
    assert [out[f][1] for f in range(2, 7)] == [1, 1, 1, 0, 0] and out[5][0].size and not out[6][0].size, "held one frame, then parked"
    rx.close()
    # the host's loop on the same frames: submit(f + 1); wait() -> f; the watch of f names the leaf; set_active needs every
    # submitted frame delivered
    host = Receiver.from_topology(scn.topo, keep_streams=True, park=True, watch=True)
    host.set_active([leaf], [0])
    host.set_watch([leaf], [1])
    got = []

    def deliver():
        host.wait()
        got.append(host.output(leaf))
        if watch.wake_list([leaf], host.watch([leaf]), 100.0) and not int(host.active([leaf])["active"][0]):
            while host.in_flight():
                host.wait()
                got.append(host.output(leaf))
            host.set_active([leaf], [1])

    for iq in scn.frames[:6]:
        host.submit(iq)
        if host.in_flight() == 2:
            deliver()
    while host.in_flight():
        deliver()
    assert len(got) == 6 and got[2].size == 0 and got[3].size == 0 and got[4].size > 0, [v.size for v in got]
    host.close()


# 4
def _gate_records(scn, want, leaves, thr, hang, ratio, window):
    return {i: gate_with_parking([w["meters"][i]["sum_sq"] for w in want], kr.events_of(scn, want, i), thr[i], hang, ratio, window) for i in leaves}


@pytest.mark.parametrize("mode,opts", [("process", dict()), ("submit", dict(squelch_auto=True)), ("device", dict(fuse_demod=True)),
                                       ("submit", dict(pipeline=True, fuse_demod=True))])
def test_with_the_gate_and_the_preroll(mode, opts):
    """squelch + preroll (+ squelch_auto): a woken leaf has the gate state of finalize -- hang_left 0, prev_open 1 (an open first
    frame is NOT pre-rolled), no floor observation -- and a parked frame is no observation; against test_park_model's gate."""
    scn, want = kr.reference("watch")
    topo = scn.topo
    leaves = topo.leaves_in_publish_order()
    auto = bool(opts.get("squelch_auto"))
    # thresholds from the model's own meters: above the quiet frames of every leaf, below its tone frames
    thr = {}
    for i in leaves:
        s = sorted(int(w["meters"][i]["sum_sq"]) for w in want if w["payload"][i] is not None)
        thr[i] = max(1, s[-1] // 8) if s else 1  # (leaf 2 never runs)
    ratio, window = (512, 2) if auto else (0, 0)
    gates = _gate_records(scn, want, leaves, thr, 1, ratio, window)
    rx = Receiver.from_topology(topo, keep_streams=True, wake=True, squelch=True, preroll=True, **opts)
    rx.set_squelch(leaves, [thr[i] for i in leaves], [1] * len(leaves))
    if auto:
        rx.set_squelch_auto(leaves, [ratio] * len(leaves), [window] * len(leaves))
    start(rx, scn)
    tag = ("gate", mode, opts)

    def check(f):
        w = want[f]
        check_frame(rx, scn, w, f, tag, squelch=True)
        sq = rx.squelch(leaves)
        pub = []
        for k, i in enumerate(leaves):
            g = gates[i][f]
            assert (int(sq["open"][k]), int(sq["hang_left"][k])) == (g["open"], g["hang_left"]), (tag, f, i, "gate", g)
            pay, pre = rx.output(i), rx.preroll(i)
            assert pay.size == (w["payload"][i].size if g["open"] else 0), (tag, f, i, "delivered iff open")
            assert pre.size == (want[f - 1]["payload"][i].size if g["pre"] else 0), (tag, f, i, "pre-roll")
            if g["open"]:
                assert np.array_equal(_bits(pay), _bits(w["payload"][i])), (tag, f, i, "payload")
                d = w["descs"][i]
                if g["pre"]:
                    assert np.array_equal(_bits(pre), _bits(want[f - 1]["payload"][i])), (tag, f, i, "pre-rolled payload")
                    pub.append((kr.live_ref.topic5(d), d.output_rate, want[f - 1]["payload"][i].tobytes()))
                pub.append((kr.live_ref.topic5(d), d.output_rate, w["payload"][i].tobytes()))
            if auto:
                a = rx.squelch_auto([i])
                assert (int(a["floor_valid"][0]), int(a["thr_eff_sum_sq"][0])) == (int(g["floor"] != kr.cu.NONE), g["thr_eff"]), (tag, f, i, "floor", g)
        assert rx.published == pub, (tag, f, "callbacks")
        assert rx.egress()["n_open"] == sum(gates[i][f]["open"] for i in leaves) and rx.preroll_count()["n_preroll"] == sum(gates[i][f]["pre"] for i in leaves)

    drive(rx, scn, mode, check)
    # the wake frames: open at once (the tone is above the threshold) and not pre-rolled -- prev_open is 1, as finalize leaves it
    for f, i in ((0, 1), (2, 3), (5, 1), (7, 6), (7, 9)):
        assert gates[i][f]["open"] == 1 and gates[i][f]["pre"] == 0 and want[f]["events"][i] == "u", (f, i, gates[i][f])
    rx.close()


COLS = ("lo_ms", "hi_ms", "silent_ms", "hold_frames", "up", "down", "gain_min", "gain_max")


@pytest.mark.parametrize("mode,opts", [("process", dict()), ("submit", dict()), ("device", dict())])
def test_with_the_agc(mode, opts):
    """agc: a woken leaf keeps the gain the device holds and starts with quiet_run 0; a parked frame is no observation.  Leaf 1
    is cold under its settings with hold_frames 1 -- quiet_run 1, then 2 and a raise, parked, and after its second wake 1 again,
    no raise --, leaf 3 is hot and steps down in every frame it runs.  Against agc_ref's closed loop on the wake model."""
    scn, plain = kr.reference("watch")
    ms = lambda i: [w["meters"][i]["sum_sq"] // w["meters"][i]["n_values"] for w in plain if w["payload"][i] is not None]  # noqa: E731
    sets = {1: agc.Cfg(8 * max(ms(1)), 1 << 30, 0, 1, 1.25, 0.5, 1e-4, 1.0), 3: agc.Cfg(0, max(1, min(ms(3)) // 64), 0, 0, 2.0, 0.75, 1e-5, 1.0)}
    ops = {0: [("agc", i, c) for i, c in sets.items()]}
    want = kr.run(scn, ops=ops, tree_cls=agc_ref.agc_tree(kr.Tree))
    q1 = [w["agc"][1]["quiet_run"] for w in want if w["payload"][1] is not None]
    assert q1 == [1, 2, 1] and [w["agc"][1]["action"] for w in want if w["payload"][1] is not None] == [0, 1, 0], q1
    assert [want[f]["agc"][3]["action"] for f in (2, 3, 4)] == [-1, -1, -1]
    rx = Receiver.from_topology(scn.topo, keep_streams=True, wake=True, agc=True, **opts)
    for i, c in sets.items():
        rx.set_agc([i], *[getattr(c, k) for k in COLS])
    start(rx, scn)
    tag = ("agc", mode, opts)

    def check(f):
        w = want[f]
        check_frame(rx, scn, w, f, tag)
        a = rx.agc(sorted(sets))
        for k, i in enumerate(sorted(sets)):
            r = w["agc"][i]
            got = (np.float32(a["gain_used"][k]).view(np.uint32), np.float32(a["gain_next"][k]).view(np.uint32), int(a["action"][k]), int(a["quiet_run"][k]))
            ref = (np.float32(r["gain_used"]).view(np.uint32), np.float32(r["gain_next"]).view(np.uint32), r["action"], r["quiet_run"])
            assert got == ref, (tag, f, i, "agc record", got, ref)

    drive(rx, scn, mode, check)
    rx.close()


# 6
def _launches(rx):
    return {k: v["launches"] for k, v in rx.kernel_times().items()}


def _collect(rx, topo, frames, ids):
    rx.enable_kernel_timing(True)
    leaves = topo.leaves_in_publish_order()
    out = []
    for iq in frames:
        rx.process(iq)
        out.append(dict(pub=list(rx.published), pay={i: rx.output(i) for i in leaves},
                        z={i: rx.stream(i, missing_ok=True) for i in range(len(topo.vfos))},
                        watch={k: v.tobytes() for k, v in rx.watch(ids).items()} if ids else None))
    return out, rx.stats()["device_bytes"], _launches(rx)


def _same_runs(a, b, what, same_bytes=True):
    assert not same_bytes or a[1] == b[1], (what, "device_bytes", a[1], b[1])
    assert a[2] == b[2], (what, "launch counts", a[2], b[2])
    for f, (x, y) in enumerate(zip(a[0], b[0])):
        assert x["pub"] == y["pub"], (what, f, "callbacks")
        assert x["watch"] == y["watch"], (what, f, "watch records")
        for key in ("pay", "z"):
            for i in x[key]:
                p, q = x[key][i], y[key][i]
                assert (p is None and q is None) or np.array_equal(_bits(p), _bits(q)), (what, f, key, i)


@pytest.mark.parametrize("opts", [dict(), dict(pipeline=True), dict(fuse=False)])
def test_option_off_and_on_with_nothing_controlled(opts):
    scn = kr.scenario("watch")
    topo, frames = scn.topo, scn.frames[:4]
    never = Receiver.from_topology(topo, keep_streams=True, **opts)
    off = Receiver(keep_streams=True, **opts)
    off._chk(off.L.sdrx_set_option(off.h, b"wake", 0))
    for d in topo.vfos:
        off.add_vfo(d)
    off.finalize()
    for call in (lambda: off.set_wake([1], 1e8), lambda: off.wake([1])):
        with pytest.raises(SdrxError) as e:
            call()
        assert e.value.code == _lib.SDRX_ESTATE
    _same_runs(_collect(never, topo, frames, None), _collect(off, topo, frames, None), ("wake = 0", opts))
    # wake = 1 with no leaf under control == park = 1, watch = 1: every frame and record, some leaves parked by the host
    ids = scn.controlled
    res = []
    for kw in (dict(park=True, watch=True), dict(wake=True)):
        rx = Receiver.from_topology(topo, keep_streams=True, **kw, **opts)
        rx.set_active([2, 9], [0, 0])
        rx.set_watch(ids, [1] * len(ids))
        if "wake" in kw:
            before = rx.stats()["device_bytes"]
            rx.set_wake([1], 1e8, on=0)  # switches nothing on: nothing is allocated, no launch is added
            assert rx.stats()["device_bytes"] == before
        res.append(_collect(rx, topo, frames, ids))
        if "wake" in kw:
            st = rx.wake([1, 2])
            assert not st["controlled"].any() and list(st["active"]) == [1, 0] and list(st["frame"]) == [3, 3] and not st["hot"].any()
            rx.set_wake([1], 1e8)  # the first leaf under control: now the tables and the records exist
            assert rx.stats()["device_bytes"] > before
        rx.close()
    # (device_bytes: the arena of wake = 1 holds no k_levels_tail list -- the option plans without tail_in_levels)
    _same_runs(res[0], res[1], ("wake = 1, nothing controlled", opts), same_bytes=False)


# 7
def test_release_in_each_state_then_set_active():
    """on = 0 leaves a leaf in the state its last frame ran in, which sdrx_get_active reads back, and sdrx_set_active works on it
    again.  Leaf 1 is released active (behind frame 1) and then parked by the host; leaf 2 is released parked and then unparked."""
    scn = kr.scenario("watch")
    off = wake.Cfg(1e8, 25600, 0, on=0)
    cfgs = {0: scn.cfgs, 2: {1: off, 2: off}}
    ops = {3: [("park", [1]), ("unpark", [2])]}
    want = kr.run(scn, cfgs=cfgs, ops=ops)
    assert want[2]["payload"][1] is not None and not want[2]["wake"].get(1), "released active, leaf 1 runs on through the cold frame 2"
    rx = make(scn)
    for f, iq in enumerate(scn.frames[:6]):
        if f == 2:
            set_wake(rx, cfgs[2])
            st = rx.active([1, 2])
            assert [int(v) for v in st["active"]] == [1, 0] and [int(v) for v in st["since_frame"]] == [0, 0], st
        if f == 3:
            rx.set_active([1], [0])
            rx.set_active([2], [1])
        rx.process(iq)
        check_frame(rx, scn, want[f], f, "release")
    # released parked BY THE DEVICE: leaf 3 parks in frame 6; released behind it, it is parked for the host too
    rx.process(scn.frames[6])
    set_wake(rx, {3: dataclasses.replace(scn.cfgs[3], on=0)})
    st = rx.active([3])
    assert (int(st["active"][0]), int(st["since_frame"][0])) == (0, 6), st
    rx.process(scn.frames[7])
    assert rx.output(3).size == 0 and int(rx.wake([3])["controlled"][0]) == 0
    rx.set_active([3], [1])
    rx.process(scn.frames[8])
    fresh = rr.Node(scn.topo.vfos[3])
    fresh.process(rx.stream(0))
    assert np.array_equal(rx.output(3), fresh.payload())
    rx.close()


def test_a_retune_of_a_controlled_leaf_moves_its_band_and_its_decisions():
    """Leaf 2 is never hot where it listens.  Retuned onto leaf 3's place before frame 2 (it is parked and controlled), it
    hears leaf 3's burst: hot in 2, 3 and 4, a new vfo at the new frequency from frame 2 on."""
    scn, plain = kr.reference("watch")
    hz = scn.topo.vfos[3].mixer_freq
    want = kr.run(scn, figs=kr.figures("watch", ((2, 2, hz),)), ops={2: [("freq", 2, hz)]})
    assert [w["wake"][2]["hot"] for w in want] == [0, 0, 1, 1, 1, 0, 0, 0, 0] and not any(w["wake"][2]["hot"] for w in plain)
    rx = make(scn)
    for f, iq in enumerate(scn.frames[:7]):
        if f == 2:
            rx.set_mixer_freqs([2], [hz])
        rx.process(iq)
        check_frame(rx, scn, want[f], f, "retune")
        lv = rx.watch([2])
        assert (int(lv["first_bin"][0]), int(lv["n_bins"][0])) == wr.band(want[f]["descs"][2]), f
    rx.close()


# 8
@pytest.mark.parametrize("members", [2, 3])
def test_group_equals_the_model(members):
    scn, want = kr.reference("watch")
    leaves = scn.topo.leaves_in_publish_order()
    grp = Group.from_topology(scn.topo, [0] * members, wake=1, meter=1)
    start(grp, scn)
    for call in (lambda: grp.set_active([4, 1], [0, 1]), lambda: grp.set_watch([3], [0])):  # a controlled leaf, through the group
        with pytest.raises(SdrxError) as e:
            call()
        assert e.value.code == _lib.SDRX_EINVAL
    for f, iq in enumerate(scn.frames):
        grp.process(iq)
        w = want[f]
        assert grp.published == w["published"], (members, f, "callbacks")
        for i in leaves:
            ref = w["payload"][i]
            assert np.array_equal(_bits(grp.output(i)), _bits(ref if ref is not None else np.zeros(0, np.int8))), (members, f, i)
        check_wake_records(grp, leaves, w, f, ("group", members))
    grp.close()


# 9
def test_errors_change_nothing():
    scn, want = kr.reference("watch")
    topo = scn.topo
    rx = make(scn)
    L = rx.L
    bytes0 = rx.stats()["device_bytes"]

    def raw(ids, cfgs, n=None):
        a = np.array(ids, np.int32)
        c = (_lib.WakeCfgC * max(1, len(cfgs)))(*cfgs)
        return L.sdrx_set_wake(rx.h, a.ctypes.data, c, len(ids) if n is None else n)

    good = _lib.WakeCfgC(1.0, 0, 7, 1)  # (would make leaf 4 hot in every frame and hold it)
    rx.set_spectrum(5, True)
    refused = [
        ([4], [good]),                                           # not watched
        ([1, 4], [good, good]),                                  # ... behind a good entry: the batch is atomic
        ([1], [_lib.WakeCfgC(1.0, 0, 0, 2)]),                    # on not 0 or 1
        ([1], [_lib.WakeCfgC(float("nan"), 0, 0, 1)]),
        ([1], [_lib.WakeCfgC(float("inf"), 0, 0, 1)]),
        ([1], [_lib.WakeCfgC(-1.0, 0, 0, 1)]),
        ([1], [_lib.WakeCfgC(1.0, 0, 0, 1, (C.c_uint32 * 3)(0, 0, 1))]),  # a reserved word
        ([1, 1], [good, good]),                                  # listed twice
        ([0], [good]),                                           # not a leaf
        ([99], [good]),
        ([1], [good], -1),
    ]
    for args in refused:
        assert raw(*args) == _lib.SDRX_EINVAL, args
    rx.set_watch([5], [1])
    assert raw([1, 5], [good, good]) == _lib.SDRX_EINVAL  # an enabled spectrum
    rx.set_spectrum(5, False)
    rx.set_watch([5], [0])
    assert L.sdrx_set_wake(rx.h, None, None, 1) == _lib.SDRX_EINVAL
    # the calls a controlled leaf refuses -- and the ones it takes
    for call in (lambda: rx.set_active([1], [1]), lambda: rx.set_active([2, 4], [1, 0]), lambda: rx.set_watch([3], [0]),
                 lambda: rx.set_spectrum(3, True)):
        with pytest.raises(SdrxError) as e:
            call()
        assert e.value.code == _lib.SDRX_EINVAL, e.value
    rx.set_gains([1], [topo.vfos[1].gain])
    rx.set_mixer_freqs([1], [topo.vfos[1].mixer_freq])  # (a retune to where it is: a fresh oscillator for a parked leaf, which its wake restarts anyway)
    rx.set_tap(1)
    rx.set_tap(-1)
    assert rx.stats()["device_bytes"] == bytes0
    rx.submit(scn.frames[0])
    with pytest.raises(SdrxError) as e:
        set_wake(rx, scn.cfgs)
    assert e.value.code == _lib.SDRX_ESTATE  # a submitted frame is undelivered
    rx.wait()
    check_frame(rx, scn, want[0], 0, "errors")
    for f in range(1, 4):  # nothing has changed: the frames are the model's
        rx.process(scn.frames[f])
        check_frame(rx, scn, want[f], f, "errors")
    rx.close()
