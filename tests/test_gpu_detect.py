"""The detector leaves on the device (sdrx_set_detector, detect.hip) against the model sdrreceiver_amd.detect, bit for bit: the
small trees and the crafted streams of tests/detect_ref.py in the three arithmetics, on the device's own leaf stream and (exact) on
the oracle's; every way a frame is handed over; parking, the catch-up and the wake (a leaf that starts again starts from
z[-1] = 0); the gate and the pre-roll on a detector leaf's meter; a gain changed between frames; the callbacks of a mixed tree; off
means off; and the refusals."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import detect_ref as dr
from helpers import bits
from oracle import binding as ob
from sdrreceiver_amd import _lib, detect as dt
from sdrreceiver_amd.receiver import Group, Receiver, SdrxError
from sdrreceiver_amd.topology import Topology

pytestmark = pytest.mark.gpu

METER_KEYS = ("n_values", "sum_sq", "clipped")


def _same(a, b):
    return np.array_equal(bits(np.ascontiguousarray(a)), bits(np.ascontiguousarray(b)))


def _code(call):
    with pytest.raises(SdrxError) as e:
        call()
    return e.value.code


def _launches(rx):
    return {k: v["launches"] for k, v in rx.kernel_times().items()}


def _check_meter(rx, i, want, what):
    m = rx.meters([i])
    for k in METER_KEYS:
        assert int(m[k][0]) == int(want[k]), (what, i, k, int(m[k][0]), int(want[k]))
    assert _same(np.float32(m["peak"][0]), np.float32(want["peak"])), (what, i, "peak")
    assert m["full_scale"][0] == 32768.0


def _check_leaf(rx, topo, i, state, what, meter=True):
    """Leaf i of the last delivered frame against the model on the device's own stream; advances `state`"""
    d = topo.vfos[i]
    z = rx.stream(i)
    assert z.size == d.n_stage_out, (what, i)
    want = dt.run(d.detector, z, rx.descs[i].gain, state)
    got = rx.output(i)
    assert got.dtype == np.int16 and got.size == z.size, (what, i, got.dtype, got.size)
    bad = np.flatnonzero(got != want["payload"])
    assert bad.size == 0, (what, i, "payload", bad.size, int(bad[0]), int(got[bad[0]]), int(want["payload"][bad[0]]))
    if meter:
        _check_meter(rx, i, want, what)
    return want


# ---- 1. the small trees: every leaf-frame length and tree position, the three arithmetics, the oracle's stream ---------------------
@pytest.mark.parametrize("exact", [1, 0, 2])
@pytest.mark.parametrize("key", sorted(dr.TREES))
def test_trees_bit_for_bit(key, exact):
    topo = dr.TREES[key]()
    leaves = dr.detector_leaves(topo)
    rx = Receiver.from_topology(topo, exact=exact, keep_streams=True, meter=True)
    state = {i: dt.State() for i in leaves}
    ostate = {i: dt.State() for i in leaves}
    nodes = roots = None
    if exact == 1:
        nodes, roots = ob.build_tree("port", topo)
    nonzero = 0
    for f, x in enumerate(dr.tree_frames(topo)):
        rx.process(x.view(np.float32))
        if nodes:
            ob.process_roots(roots, np.ascontiguousarray(x).view(np.float32))
        for i in leaves:
            want = _check_leaf(rx, topo, i, state[i], (key, exact, f))
            nonzero += int(np.count_nonzero(want["payload"]))
            if nodes:
                zo = nodes[i].stream().view(np.complex64)
                assert _same(rx.stream(i), zo), (key, f, i, "stream against the oracle")
                on = dt.run(topo.vfos[i].detector, zo, topo.vfos[i].gain, ostate[i])
                assert np.array_equal(rx.output(i), on["payload"]), (key, f, i, "payload on the oracle's stream")
    assert nonzero > 1000
    rx.close()


# ---- 2. the crafted streams ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [1, 0, 2])
@pytest.mark.parametrize("case", dr.crafted(), ids=dr.case_ids())
def test_crafted_case(case, exact):
    topo = dr.tree_pair(dr.N_CRAFT, case.gain_am, case.gain_fm)
    rx = Receiver.from_topology(topo, exact=exact, keep_streams=True, meter=True)
    state = {0: dt.State(), 1: dt.State()}
    for f, x in enumerate(case.frames):
        rx.process(x.view(np.float32))
        for i in (0, 1):
            # the stream is the frame times the oscillator's amplitude, a positive real number: what the case was crafted for stays
            z = rx.stream(i)
            assert np.array_equal(z == 0, x == 0) and np.array_equal(np.signbit(z.real), np.signbit(x.real)), (case.name, f, i)
            assert np.array_equal(np.abs(z.real) == np.abs(z.imag), np.abs(x.real) == np.abs(x.imag)), (case.name, f, i, "diagonals")
            _check_leaf(rx, topo, i, state[i], (case.name, exact, f))
    rx.close()


# ---- 3. every way a frame is handed over -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(key):
    """want[f][leaf] = the model's record on the exact arithmetic's streams, frame by frame through sdrx_process; computed once"""
    topo = dr.TREES[key]()
    leaves = dr.detector_leaves(topo)
    rx = Receiver.from_topology(topo, keep_streams=True)
    state = {i: dt.State() for i in leaves}
    want = []
    for x in dr.tree_frames(topo):
        rx.process(x.view(np.float32))
        want.append({i: dt.run(topo.vfos[i].detector, rx.stream(i), topo.vfos[i].gain, state[i]) for i in leaves})
    rx.close()
    return want


def _check_against(rx, topo, want, what, meter=True):
    for i, w in want.items():
        assert np.array_equal(rx.output(i), w["payload"]), (what, i, "payload")
        if meter:
            _check_meter(rx, i, w, what)


@pytest.mark.parametrize("segments", [0, 1, 2, 3])
@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("mode", ["process", "submit", "device"])
def test_frame_paths(mode, fuse, segments):
    key = "b" if segments < 2 else "a"  # (both trees under every mode; the two-level tree b takes the software pipeline)
    topo = dr.TREES[key]()
    want = _reference(key)
    frames = dr.tree_frames(topo)
    rx = Receiver.from_topology(topo, fuse=bool(fuse), segments=segments, meter=True)
    what = (mode, fuse, segments)
    if mode == "process":
        for f, x in enumerate(frames):
            rx.process(x.view(np.float32))
            _check_against(rx, topo, want[f], what + (f,))
    elif mode == "submit":  # two frames in flight
        delivered = 0
        for x in frames:
            rx.submit(x.view(np.float32))
            if rx.in_flight() == 2:
                rx.wait()
                _check_against(rx, topo, want[delivered], what + (delivered,))
                delivered += 1
        while rx.in_flight():
            rx.wait()
            _check_against(rx, topo, want[delivered], what + (delivered,))
            delivered += 1
        assert delivered == len(frames)
    else:  # four frames queued on the device, no host call between them: z[-1] and the carrier's partials carry on the device
        import torch
        dev = [torch.from_numpy(np.array(x)).cuda() for x in frames]
        torch.cuda.synchronize()
        for d in dev:
            rx.process_device(d.data_ptr(), topo.frame)
        rx.fetch()
        _check_against(rx, topo, want[len(frames) - 1], what + ("last",))
    rx.close()


# ---- 4. park, then unpark: the FM leaf restarts from z[-1] = 0, the AM leaf carries nothing ------------------------------------------
def test_park_then_unpark():
    topo = dr.tree_b()
    am, fm = 3, 4
    frames = dr.tree_frames(topo, 6, seed=1)
    rx = Receiver.from_topology(topo, keep_streams=True, meter=True, park=True)
    state = {i: dt.State() for i in dr.detector_leaves(topo)}
    last_before = None
    for f, x in enumerate(frames):
        if f == 2:
            last_before = complex(rx.stream(fm)[-1])
            rx.set_active([am, fm], [0, 0])
        if f == 4:
            rx.set_active([am, fm], [1, 1])
            state[am], state[fm] = dt.State(), dt.State()  # new vfos
        rx.process(x.view(np.float32))
        for i in dr.detector_leaves(topo):
            if i in (am, fm) and f in (2, 3):
                assert rx.output(i).size == 0 and int(rx.meters([i])["n_values"][0]) == 0, (f, i, "parked")
                continue
            _check_leaf(rx, topo, i, state[i], ("park", f))
        if f == 4:  # what a leaf that kept its z[-1] would have emitted differs in sample 0
            z = rx.stream(fm)
            assert last_before != 0 and dt.fm(z, topo.vfos[fm].gain, last_before)[0] != dt.fm(z, topo.vfos[fm].gain)[0]
            assert rx.output(fm)[0] == 0  # z[0] conj(0) = 0: ANG(0, 0) = 0
    rx.close()


# ---- 5. the catch-up and the wake on one AM and one FM leaf -----------------------------------------------------------------------------
def test_catchup_starts_one_frame_back():
    topo = dr.tree_b()
    am, fm = 3, 4
    frames = dr.tree_frames(topo, 4, seed=2)
    # the twin starts the two leaves as new vfos at frame 2; the caught-up ones are unparked before frame 3 and run frame 2 then
    twin = Receiver.from_topology(topo, keep_streams=True, meter=True, park=True)
    state = {am: dt.State(), fm: dt.State()}
    want = {}
    for f, x in enumerate(frames):
        if f == 1:
            twin.set_active([am, fm], [0, 0])
        if f == 2:
            twin.set_active([am, fm], [1, 1])
        twin.process(x.view(np.float32))
        if f >= 2:
            want[f] = {i: _check_leaf(twin, topo, i, state[i], ("twin", f)) for i in (am, fm)}
    twin.close()
    rx = Receiver.from_topology(topo, meter=True, catchup=True)
    for f, x in enumerate(frames):
        if f == 1:
            rx.set_active([am, fm], [0, 0])
        if f == 3:
            rx.set_active([am, fm], [1, 1])
            m = rx.catchup([am, fm])
            for k, i in enumerate((am, fm)):
                assert int(m["frame"][k]) == 2
                for key in METER_KEYS:
                    assert int(m[key][k]) == int(want[2][i][key]), ("catchup meter", i, key)
        rx.process(x.view(np.float32))
    for i in (am, fm):
        assert np.array_equal(rx.preroll(i), want[2][i]["payload"]), (i, "the caught-up frame leaves through the pre-roll")
        assert np.array_equal(rx.output(i), want[3][i]["payload"]), (i, "frame 3 carries on from it")
        _check_meter(rx, i, want[3][i], "catchup")
    rx.close()


def test_wake_starts_a_new_vfo_inside_the_frame():
    topo = dr.tree_b()
    am, fm = 3, 4
    sig = dr.tree_frames(topo, 4, seed=3)
    zero = dr.ro(np.zeros(topo.frame, np.complex64))
    frames = [sig[0], zero, zero, sig[2], sig[3]]
    rx = Receiver.from_topology(topo, keep_streams=True, meter=True, wake=True)
    state = {am: dt.State(), fm: dt.State()}
    for f, x in enumerate(frames):
        if f == 1:  # frame 0 ran uncontrolled and left its last sample in the FM leaf's slot of parity 1 -- the one frame 3 reads
            assert rx.stream(fm)[-1] != 0
            rx.set_watch([am, fm], [1, 1])
            rx.set_wake([am, fm], 1e-6)
        rx.process(x.view(np.float32))
        w = rx.wake([am, fm])
        if f in (1, 2):
            assert list(w["active"]) == [0, 0] and rx.output(am).size == 0 and rx.output(fm).size == 0, (f, "cold: parked")
            continue
        if f == 3:
            assert list(w["active"]) == [1, 1] and list(w["hot"]) == [1, 1]
            state = {am: dt.State(), fm: dt.State()}  # woken: new vfos, in this very frame
        for i in (am, fm):
            _check_leaf(rx, topo, i, state[i], ("wake", f))
        if f == 3:
            assert rx.output(fm)[0] == 0
    rx.close()


# ---- 6. the gate and the pre-roll driven by a detector leaf's meter ----------------------------------------------------------------------
def test_squelch_gate_and_preroll():
    case = next(c for c in dr.crafted() if c.name == "carrier_step")
    topo = dr.tree_pair(dr.N_CRAFT, case.gain_am, case.gain_fm)
    zero = dr.ro(np.zeros(dr.N_CRAFT, np.complex64))
    frames = [zero, zero, case.frames[0], case.frames[1], zero]
    rx = Receiver.from_topology(topo, keep_streams=True, meter=True, squelch=True, preroll=True)
    rx.set_squelch([0, 1], [1, 1], [0, 0])  # open on any non-zero payload value, no hang
    state = {0: dt.State(), 1: dt.State()}
    prev = {}
    for f, x in enumerate(frames):
        rx.process(x.view(np.float32))
        want = {i: dt.run(topo.vfos[i].detector, rx.stream(i), topo.vfos[i].gain, state[i]) for i in (0, 1)}
        opened = list(rx.squelch([0, 1])["open"])
        assert opened == [int(want[i]["sum_sq"] >= 1) for i in (0, 1)], (f, opened)
        for i in (0, 1):
            if not opened[i]:
                assert rx.output(i).size == 0, (f, i, "closed")
                continue
            assert np.array_equal(rx.output(i), want[i]["payload"]), (f, i)
            pre = rx.preroll(i)
            if f == 2:  # just opened: the frame before, all zeros, first
                assert pre.dtype == np.int16 and np.array_equal(pre, prev[i]["payload"]) and not pre.any(), (f, i, "pre-roll")
            else:
                assert pre.size == 0, (f, i)
        prev = want
    assert rx.squelch([0, 1])["open"].tolist() == [0, 0]  # the zeros behind the signal: AM of zeros is zeros, FM of zeros too
    rx.close()


# ---- 7. sdrx_set_gains between frames ------------------------------------------------------------------------------------------------
def test_set_gains_between_frames():
    topo = dr.tree_b()
    leaves = dr.detector_leaves(topo)
    rx = Receiver.from_topology(topo, keep_streams=True, meter=True)
    state = {i: dt.State() for i in leaves}
    for f, x in enumerate(dr.tree_frames(topo, 3, seed=4)):
        if f == 1:
            rx.set_gains([3, 4, 2], [0.25, 1.75, 0.3])
        if f == 2:
            rx.set_gains([4], [-1.0])
        rx.process(x.view(np.float32))
        for i in leaves:
            _check_leaf(rx, topo, i, state[i], ("gain", f))  # (the model takes rx.descs[i].gain: what set_gains left there)
    assert rx.descs[4].gain == -1.0 and rx.descs[3].gain == 0.25
    rx.close()


# ---- 8. the callbacks of the mixed tree: order, topic, rate, length ------------------------------------------------------------------
def test_mixed_tree_callbacks():
    topo = dr.tree_a()
    rx = Receiver.from_topology(topo)
    rx.process(dr.tree_frames(topo)[0].view(np.float32))
    want = []
    for i in topo.leaves_in_publish_order():
        d = topo.vfos[i]
        if d.demod_usb:
            want.append((d.topic, d.output_rate, 2 * d.n_out))
        elif d.topic:  # an IQ leaf's rule, and a detector leaf's: only with a topic
            want.append((d.topic, d.fs >> d.decimate_count, 2 * d.n_stage_out if d.detector or d.cstyle == 0 else d.n_stage_out))
    got = [(t.rstrip(b"\0").decode(), r, len(b)) for t, r, b in rx.published]
    assert got == want
    kinds = [topo.vfos[i].detector for i in topo.leaves_in_publish_order() if topo.vfos[i].demod_usb or topo.vfos[i].topic]
    assert {0, dt.AM, dt.FM} <= set(kinds)
    for (t, r, b), i in zip(rx.published, [i for i in topo.leaves_in_publish_order() if topo.vfos[i].demod_usb or topo.vfos[i].topic]):
        assert b == rx.output(i).tobytes(), (i, "the callback's bytes are the leaf's payload")
    assert rx.detector(1) == dt.AM and rx.detector(2) == dt.FM and rx.detector(5) == dt.NONE and rx.output_rate(2) == 7680
    rx.close()


# ---- 9. off means off -----------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    """A receiver that never calls sdrx_set_detector, one that sets and takes away a detector on every leaf, and the other leaves
    of one that has detectors: the same launches, the same device bytes, the same payloads"""
    topo = dr.tree_a()
    plain = Topology(fs=topo.fs, frame=topo.frame, vfos=[dataclasses.replace(v, detector=0) for v in topo.vfos])
    frames = dr.tree_frames(topo)

    def run(rx):
        rx.enable_kernel_timing(True)
        out = []
        for x in frames:
            rx.process(x.view(np.float32))
            out.append({i: rx.output(i) for i in range(len(topo.vfos)) if not topo.children(i)})
        rx.sync()
        res = out, _launches(rx), rx.stats()["device_bytes"]
        rx.close()
        return res

    never = Receiver.from_topology(plain, meter=True)
    undone = Receiver(meter=True)
    for i, v in enumerate(plain.vfos):
        undone.add_vfo(v)
        if not v.demod_usb:
            undone.set_detector(i, dt.AM if i & 1 else dt.FM)
            undone.set_detector(i, dt.NONE)
    undone.finalize()
    a, b = run(never), run(undone)
    assert a[1] == b[1] and a[2] == b[2]
    n_iq = sum(1 for i, v in enumerate(plain.vfos) if not v.demod_usb and not plain.children(i))
    assert a[1]["k_compress"] == len(frames) and n_iq == 9
    c = run(Receiver.from_topology(topo, meter=True))
    assert c[1]["k_compress"] == 3 * len(frames)  # (the detector launches are booked with k_compress: its own, the AM and the FM leaves')
    assert {k: v for k, v in c[1].items() if k != "k_compress"} == {k: v for k, v in a[1].items() if k != "k_compress"}
    for f in range(len(frames)):
        for i in a[0][f]:
            assert np.array_equal(a[0][f][i], b[0][f][i]), (f, i)
            if not topo.vfos[i].detector:
                assert np.array_equal(a[0][f][i], c[0][f][i]), (f, i, "a leaf beside detector leaves")
            else:
                assert a[0][f][i].dtype == np.int8 and c[0][f][i].dtype == np.int16 and a[0][f][i].nbytes == c[0][f][i].nbytes


# ---- 10. the refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    topo = dr.tree_a()
    L = _lib.lib()
    rx = Receiver()
    for v in topo.vfos:
        rx.add_vfo(dataclasses.replace(v, detector=0))
    cfg = lambda kind, r=(0, 0, 0): C.byref(_lib.DetectCfgC(kind, (C.c_int32 * 3)(*r)))  # noqa: E731
    assert L.sdrx_set_detector(rx.h, 4, cfg(dt.AM)) == _lib.SDRX_EINVAL  # a USB leaf
    assert L.sdrx_set_detector(rx.h, 1, cfg(3)) == _lib.SDRX_EINVAL and L.sdrx_set_detector(rx.h, 1, cfg(-1)) == _lib.SDRX_EINVAL
    for r in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        assert L.sdrx_set_detector(rx.h, 1, cfg(dt.FM, r)) == _lib.SDRX_EINVAL
    assert L.sdrx_set_detector(rx.h, len(topo.vfos), cfg(dt.AM)) == _lib.SDRX_EINVAL and L.sdrx_set_detector(rx.h, -1, cfg(dt.AM)) == _lib.SDRX_EINVAL
    assert L.sdrx_set_detector(rx.h, 1, None) == _lib.SDRX_EINVAL and L.sdrx_get_detector(rx.h, 1, None) == _lib.SDRX_EINVAL
    assert all(rx.detector(i) == dt.NONE for i in range(len(topo.vfos))), "a refused call changes nothing"
    rx.set_detector(1, dt.AM)
    rx.finalize()
    assert _code(lambda: rx.set_detector(2, dt.FM)) == _lib.SDRX_ESTATE and rx.detector(1) == dt.AM and rx.detector(2) == dt.NONE
    rx.close()
    # a node with children that carries a detector: refused at finalize
    rx = Receiver()
    for v in topo.vfos:
        rx.add_vfo(dataclasses.replace(v, detector=0))
    rx.set_detector(0, dt.AM)
    assert _code(rx.finalize) == _lib.SDRX_EINVAL
    rx.close()
    # groups do not offer it: the wrapper says so, and a member handed out by the group is a finalized context
    with pytest.raises(ValueError):
        Group.from_topology(topo, [0])
    plain = Topology(fs=topo.fs, frame=topo.frame, vfos=[dataclasses.replace(v, detector=0) for v in topo.vfos])
    grp = Group.from_topology(plain, [0, 0])
    ctx, _ = grp.member_context(0)
    assert L.sdrx_set_detector(ctx, 1, cfg(dt.AM)) == _lib.SDRX_ESTATE
    grp.close()


# ---- 11. sdrx_demo needs nothing but the INI -------------------------------------------------------------------------------------------
def _fnv1a(b: bytes) -> int:
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_demo_on_the_ini(tmp_path):
    """host/sdrx_demo on a copy of sdr_25E.ini with an AM and an FM entry: the messages of the C++ host (vfo::setDetector behind the
    INI key) are those of the Python host on the same topology, and the two entries' are int16 at 48 kS/s"""
    import os
    import subprocess
    from oracle import binding as ob
    from sdrreceiver_amd import synth
    from test_detect_model import ROOT, detector_ini
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "sdrx_demo"], stdout=subprocess.DEVNULL)
    text, topo = detector_ini()
    p = tmp_path / "detect.ini"
    p.write_text(text)
    out = subprocess.check_output([os.path.join(ROOT, "host", "sdrx_demo"), str(p), "--frames", "2"], text=True, timeout=120)
    got = [l.split() for l in out.splitlines()]
    rx = Receiver.from_topology(topo)
    lcg = synth.Lcg(1)
    state = np.zeros(2, np.float32)
    want = []
    for f in range(2):
        iq = synth.lcg_frame(topo.frame, lcg)
        if topo.correct_dc:
            ob.dc_correct(iq, state)
        rx.process(iq)
        for topic, rate, payload in rx.published:
            want.append([str(f), topic.rstrip(b"\0").decode(), str(rate), str(len(payload)), f"{_fnv1a(payload):016x}"])
    rx.close()
    assert got == want
    for name in ("AIR01", "AIS01"):
        rows = [r for r in got if r[1] == name]
        assert len(rows) == 2 and all(r[2] == "48000" and r[3] == str(2 * 12000) for r in rows), rows
