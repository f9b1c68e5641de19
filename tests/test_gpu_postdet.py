"""The post-detection filter on the device (sdrx_set_postfilter, postdet.hip) against the model sdrreceiver_amd.postdet, bit for bit:
the small trees and the crafted streams of tests/postdet_ref.py in the three arithmetics, on the device's own leaf stream; every way
a frame is handed over; parking, the catch-up and the wake (a leaf that starts again starts from a zero history); the gate and the
pre-roll on the shorter payloads; a gain changed between frames (the history keeps the old gain's values); the callbacks of a mixed
tree; the identity; off means off; the refusals and the read-back."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import detect_ref as dr
import postdet_ref as pr
from helpers import bits
from sdrreceiver_amd import _lib, detect as dt, postdet as pd
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
    """Detector leaf i of the last delivered frame against the model on the device's own stream; advances `state`"""
    d = rx.descs[i]
    z = rx.stream(i)
    assert z.size == d.n_stage_out, (what, i)
    want = pr.run_leaf(d, z, d.gain, state)
    got = rx.output(i)
    assert got.dtype == np.int16 and got.size == d.n_detect_out, (what, i, got.dtype, got.size)
    bad = np.flatnonzero(got != want["payload"])
    assert bad.size == 0, (what, i, "payload", bad.size, int(bad[0]), int(got[bad[0]]), int(want["payload"][bad[0]]))
    if meter:
        _check_meter(rx, i, want, what)
    return want


# ---- 1. the small trees: every class of leaf-frame, the three arithmetics -----------------------------------------------------------
@pytest.mark.parametrize("exact", [1, 0, 2])
@pytest.mark.parametrize("key", sorted(pr.TREES))
def test_trees_bit_for_bit(key, exact):
    topo = pr.TREES[key]()
    leaves = pr.detector_leaves(topo)
    rx = Receiver.from_topology(topo, exact=exact, keep_streams=True, meter=True)
    state = {i: pd.State() for i in leaves}
    nonzero = 0
    for f, x in enumerate(pr.tree_frames(topo)):
        rx.process(x.view(np.float32))
        for i in leaves:
            want = _check_leaf(rx, topo, i, state[i], (key, exact, f))
            nonzero += int(np.count_nonzero(want["payload"]))
    assert nonzero > 1000
    rx.close()


# ---- 2. the crafted streams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [1, 0, 2])
@pytest.mark.parametrize("case", pr.gpu_cases(), ids=pr.case_ids(pr.gpu_cases()))
def test_crafted_case(case, exact):
    topo = dr.tree_pair(pr.N_CRAFT, pr.gain_of(case, dt.AM), pr.gain_of(case, dt.FM))
    topo.vfos = [dataclasses.replace(v, post_taps=case.taps, post_decim=case.decim) for v in topo.vfos]
    rx = Receiver.from_topology(topo, exact=exact, keep_streams=True, meter=True)
    state = {0: pd.State(), 1: pd.State()}
    for f, x in enumerate(case.frames):
        if case.gain_steps and f:
            rx.set_gains([0, 1], [pr.gain_of(case, dt.AM, f), pr.gain_of(case, dt.FM, f)])
        rx.process(x.view(np.float32))
        for i, kind in ((0, dt.AM), (1, dt.FM)):
            assert rx.descs[i].gain == pr.gain_of(case, kind, f), (case.name, f, i)
            z = rx.stream(i)
            assert np.array_equal(z == 0, x == 0) and np.array_equal(np.signbit(z.real), np.signbit(x.real)), (case.name, f, i)
            _check_leaf(rx, topo, i, state[i], (case.name, exact, f))
    rx.close()


# ---- 3. every way a frame is handed over ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(key):
    """want[f][leaf] = the model's record on the exact arithmetic's streams, frame by frame through sdrx_process; computed once"""
    topo = pr.TREES[key]()
    leaves = pr.detector_leaves(topo)
    rx = Receiver.from_topology(topo, keep_streams=True)
    state = {i: pd.State() for i in leaves}
    want = []
    for x in pr.tree_frames(topo):
        rx.process(x.view(np.float32))
        want.append({i: pr.run_leaf(topo.vfos[i], rx.stream(i), topo.vfos[i].gain, state[i]) for i in leaves})
    rx.close()
    return want


def _check_against(rx, want, what, meter=True):
    for i, w in want.items():
        assert np.array_equal(rx.output(i), w["payload"]), (what, i, "payload")
        if meter:
            _check_meter(rx, i, w, what)


@pytest.mark.parametrize("segments", [0, 1, 2, 3])
@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("mode", ["process", "submit", "device"])
def test_frame_paths(mode, fuse, segments):
    key = "c" if segments < 2 else "a"
    topo = pr.TREES[key]()
    want = _reference(key)
    frames = pr.tree_frames(topo)
    rx = Receiver.from_topology(topo, fuse=bool(fuse), segments=segments, meter=True)
    what = (mode, fuse, segments)
    if mode == "process":
        for f, x in enumerate(frames):
            rx.process(x.view(np.float32))
            _check_against(rx, want[f], what + (f,))
    elif mode == "submit":  # two frames in flight
        delivered = 0
        for x in frames:
            rx.submit(x.view(np.float32))
            if rx.in_flight() == 2:
                rx.wait()
                _check_against(rx, want[delivered], what + (delivered,))
                delivered += 1
        while rx.in_flight():
            rx.wait()
            _check_against(rx, want[delivered], what + (delivered,))
            delivered += 1
        assert delivered == len(frames)
    else:  # four frames queued on the device, no host call between them: the history carries on the device
        import torch
        dev = [torch.from_numpy(np.array(x)).cuda() for x in frames]
        torch.cuda.synchronize()
        for d in dev:
            rx.process_device(d.data_ptr(), topo.frame)
        rx.fetch()
        _check_against(rx, want[len(frames) - 1], what + ("last",))
    rx.close()


# ---- 4. park, then unpark: the leaf restarts from a zero history -----------------------------------------------------------------------
def test_park_then_unpark():
    topo = pr.tree_c()
    am, fm, short = 3, 4, 7
    frames = pr.tree_frames(topo, 6, seed=1)
    rx = Receiver.from_topology(topo, keep_streams=True, meter=True, park=True)
    state = {i: pd.State() for i in pr.detector_leaves(topo)}
    for f, x in enumerate(frames):
        if f == 2:
            rx.set_active([am, fm, short], [0, 0, 0])
        if f == 4:
            rx.set_active([am, fm, short], [1, 1, 1])
            kept = {i: state[i] for i in (am, fm, short)}
            for i in (am, fm, short):
                state[i] = pd.State()  # new vfos
        rx.process(x.view(np.float32))
        for i in pr.detector_leaves(topo):
            if i in (am, fm, short) and f in (2, 3):
                assert rx.output(i).size == 0 and int(rx.meters([i])["n_values"][0]) == 0, (f, i, "parked")
                continue
            _check_leaf(rx, topo, i, state[i], ("park", f))
        if f == 4:  # what a leaf that kept its history would have emitted differs
            for i in (am, fm, short):
                d = topo.vfos[i]
                assert not np.array_equal(pr.run_leaf(d, rx.stream(i), d.gain, kept[i])["payload"], rx.output(i)), i
    rx.close()


# ---- 5. the catch-up and the wake ---------------------------------------------------------------------------------------------------------
def test_catchup_starts_one_frame_back():
    topo = pr.tree_c()
    am, fm = 3, 4
    frames = pr.tree_frames(topo, 4, seed=2)
    twin = Receiver.from_topology(topo, keep_streams=True, meter=True, park=True)
    state = {am: pd.State(), fm: pd.State()}
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
    topo = pr.tree_c()
    am, fm = 3, 4
    sig = pr.tree_frames(topo, 4, seed=3)
    zero = pr.ro(np.zeros(topo.frame, np.complex64))
    frames = [sig[0], zero, zero, sig[2], sig[3]]
    rx = Receiver.from_topology(topo, keep_streams=True, meter=True, wake=True)
    state = {am: pd.State(), fm: pd.State()}
    for f, x in enumerate(frames):
        if f == 1:  # frame 0 ran uncontrolled and left its history in the slot of parity 1 -- the one frame 3 reads
            assert state[am].hist.any() and state[fm].hist.any()
            rx.set_watch([am, fm], [1, 1])
            rx.set_wake([am, fm], 1e-6)
        rx.process(x.view(np.float32))
        if f == 0:
            for i in (am, fm):
                _check_leaf(rx, topo, i, state[i], ("wake", f))
            continue
        w = rx.wake([am, fm])
        if f in (1, 2):
            assert list(w["active"]) == [0, 0] and rx.output(am).size == 0 and rx.output(fm).size == 0, (f, "cold: parked")
            continue
        if f == 3:
            assert list(w["active"]) == [1, 1] and list(w["hot"]) == [1, 1]
            state = {am: pd.State(), fm: pd.State()}  # woken: new vfos, in this very frame
        for i in (am, fm):
            _check_leaf(rx, topo, i, state[i], ("wake", f))
    rx.close()


# ---- 6. the gate and the pre-roll on the shorter payloads ---------------------------------------------------------------------------------
def test_squelch_gate_and_preroll():
    case = next(c for c in pr.crafted() if c.name == "gain_step")
    topo = dr.tree_pair(pr.N_CRAFT, case.gain_am, case.gain_fm)
    topo.vfos = [dataclasses.replace(v, post_taps=case.taps, post_decim=case.decim) for v in topo.vfos]
    zero = pr.ro(np.zeros(pr.N_CRAFT, np.complex64))
    frames = [zero, zero, case.frames[0], case.frames[1], zero, zero]
    rx = Receiver.from_topology(topo, keep_streams=True, meter=True, squelch=True, preroll=True)
    rx.set_squelch([0, 1], [1, 1], [0, 0])  # open on any non-zero payload value, no hang
    state = {0: pd.State(), 1: pd.State()}
    prev = {}
    n_out = pr.N_CRAFT // case.decim
    seen_open = 0
    for f, x in enumerate(frames):
        rx.process(x.view(np.float32))
        want = {i: pr.run_leaf(topo.vfos[i], rx.stream(i), topo.vfos[i].gain, state[i]) for i in (0, 1)}
        opened = list(rx.squelch([0, 1])["open"])
        assert opened == [int(want[i]["sum_sq"] >= 1) for i in (0, 1)], (f, opened)
        for i in (0, 1):
            if not opened[i]:
                assert rx.output(i).size == 0, (f, i, "closed")
                continue
            seen_open += 1
            assert rx.output(i).size == n_out and np.array_equal(rx.output(i), want[i]["payload"]), (f, i)
            pre = rx.preroll(i)
            if f == 2:  # just opened: the frame before, all zeros, first -- n / R values of it
                assert pre.dtype == np.int16 and pre.size == n_out and np.array_equal(pre, prev[i]["payload"]) and not pre.any(), (f, i, "pre-roll")
            else:
                assert pre.size == 0, (f, i)
        prev = want
    assert seen_open >= 4 and opened == [0, 0]  # (frame 4 still drains the history; frame 5 is zeros)
    rx.close()


# ---- 7. sdrx_set_gains between frames: the history keeps the old gain's values -------------------------------------------------------------
def test_set_gains_between_frames():
    topo = pr.tree_c()
    leaves = pr.detector_leaves(topo)
    rx = Receiver.from_topology(topo, keep_streams=True, meter=True)
    state = {i: pd.State() for i in leaves}
    for f, x in enumerate(pr.tree_frames(topo, 3, seed=4)):
        if f == 1:
            rx.set_gains([3, 4, 2, 6], [0.25, 1.75, 0.3, 0.1])
        if f == 2:
            rx.set_gains([4, 7], [-1.0, 2.0])
        rx.process(x.view(np.float32))
        for i in leaves:
            _check_leaf(rx, topo, i, state[i], ("gain", f))  # (the model takes rx.descs[i].gain: what set_gains left there)
    assert rx.descs[4].gain == -1.0 and rx.descs[3].gain == 0.25
    rx.close()


# ---- 8. the callbacks of the mixed tree: order, topic, rate, length ------------------------------------------------------------------------
def test_mixed_tree_callbacks():
    for key in sorted(pr.TREES):
        topo = pr.TREES[key]()
        rx = Receiver.from_topology(topo)
        rx.process(pr.tree_frames(topo)[0].view(np.float32))
        want, ids = [], []
        for i in topo.leaves_in_publish_order():
            d = topo.vfos[i]
            if d.demod_usb:
                want.append((d.topic, d.output_rate, 2 * d.n_out))
            elif d.topic and d.detector:
                want.append((d.topic, d.detect_rate, 2 * d.n_detect_out))
            elif d.topic:
                want.append((d.topic, d.fs >> d.decimate_count, 2 * d.n_stage_out if d.cstyle == 0 else d.n_stage_out))
            else:
                continue
            ids.append(i)
        got = [(t.rstrip(b"\0").decode(), r, len(b)) for t, r, b in rx.published]
        assert got == want
        for (t, r, b), i in zip(rx.published, ids):
            assert b == rx.output(i).tobytes(), (i, "the callback's bytes are the leaf's payload")
            assert rx.output_rate(i) == r
        rx.close()
    assert ("AM0", 15360 // 6, 2 * 2560) in want and ("FM3", 7680 // 2 // 16, 2 * 240) in want and ("AM3", 7680, 2 * 7680) in want


# ---- 9. the identity: T = 1, h = {1.0f}, R = 1 against the unfiltered leaf ---------------------------------------------------------------------
def test_identity_against_the_unfiltered_leaf():
    plain = dr.tree_b()
    same = Topology(fs=plain.fs, frame=plain.frame, vfos=[dataclasses.replace(v, post_taps=(1.0,), post_decim=1) if v.detector else v for v in plain.vfos])
    a, b = Receiver.from_topology(plain, meter=True), Receiver.from_topology(same, meter=True)
    leaves = dr.detector_leaves(plain)
    for f, x in enumerate(dr.tree_frames(plain)):
        a.process(x.view(np.float32))
        b.process(x.view(np.float32))
        ma, mb = a.meters(leaves), b.meters(leaves)
        for k, i in enumerate(leaves):
            assert np.array_equal(a.output(i), b.output(i)) and a.output(i).any(), (f, i)
            for key in METER_KEYS:
                assert int(ma[key][k]) == int(mb[key][k]), (f, i, key)
            assert _same(np.float32(ma["peak"][k]), np.float32(mb["peak"][k])), (f, i)
    a.close()
    b.close()


# ---- 10. off means off ---------------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    """A receiver that never calls sdrx_set_postfilter and one that sets and takes away a filter on every detector leaf: the same
    launches, the same device bytes, the same payloads; and the leaves without a filter of a tree that has some emit what they
    emit in a tree that has none"""
    topo = pr.tree_c()
    plain = Topology(fs=topo.fs, frame=topo.frame, vfos=[dataclasses.replace(v, post_taps=(), post_decim=1) for v in topo.vfos])
    frames = pr.tree_frames(topo)

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
        if v.detector:
            undone.set_postfilter(i, pr.taps_random(64, i), 2)
            undone.set_postfilter(i, None)
    undone.finalize()
    a, b = run(never), run(undone)
    assert a[1] == b[1] and a[2] == b[2]
    assert a[1]["k_compress"] == 3 * len(frames)  # its own, the AM and the FM leaves'
    c = run(Receiver.from_topology(topo, meter=True))
    assert c[1]["k_compress"] == 5 * len(frames)  # ... and the filtered AM and FM leaves' (booked with k_compress)
    assert {k: v for k, v in c[1].items() if k != "k_compress"} == {k: v for k, v in a[1].items() if k != "k_compress"}
    for f in range(len(frames)):
        for i in a[0][f]:
            assert np.array_equal(a[0][f][i], b[0][f][i]), (f, i)
            if not len(topo.vfos[i].post_taps):
                assert np.array_equal(a[0][f][i], c[0][f][i]), (f, i, "a leaf beside filtered leaves")
            else:
                assert c[0][f][i].size * topo.vfos[i].post_decim == a[0][f][i].size


# ---- 11. the refusals and the read-back ---------------------------------------------------------------------------------------------------
def test_refusals_and_read_back():
    topo = pr.tree_a()
    L = _lib.lib()
    rx = Receiver()
    for v in topo.vfos:
        rx.add_vfo(dataclasses.replace(v, post_taps=(), post_decim=1))
    h = np.asarray(pr.taps_random(64, 1), np.float32)
    big = np.zeros(300, np.float32)
    cfg = lambda decim, ntaps, r=(0, 0): C.byref(_lib.PostfilterCfgC(decim, ntaps, (C.c_int32 * 2)(*r)))  # noqa: E731
    info = _lib.PostfilterInfoC()
    for decim, ntaps in ((0, 64), (17, 64), (-1, 64), (1, 257), (1, -1)):
        assert L.sdrx_set_postfilter(rx.h, 1, cfg(decim, ntaps), big.ctypes.data) == _lib.SDRX_EINVAL, (decim, ntaps)
    for r in ((1, 0), (0, 1)):
        assert L.sdrx_set_postfilter(rx.h, 1, cfg(2, 64, r), h.ctypes.data) == _lib.SDRX_EINVAL
        assert L.sdrx_set_postfilter(rx.h, 1, cfg(0, 0, r), None) == _lib.SDRX_EINVAL
    assert L.sdrx_set_postfilter(rx.h, len(topo.vfos), cfg(2, 64), h.ctypes.data) == _lib.SDRX_EINVAL
    assert L.sdrx_set_postfilter(rx.h, -1, cfg(2, 64), h.ctypes.data) == _lib.SDRX_EINVAL
    assert L.sdrx_set_postfilter(rx.h, 1, None, h.ctypes.data) == _lib.SDRX_EINVAL and L.sdrx_set_postfilter(rx.h, 1, cfg(2, 64), None) == _lib.SDRX_EINVAL
    assert L.sdrx_get_postfilter(rx.h, 1, None, None, 0) == _lib.SDRX_EINVAL and L.sdrx_get_postfilter(rx.h, -1, C.byref(info), None, 0) == _lib.SDRX_EINVAL
    assert all(_code(lambda i=i: rx.postfilter(i)) == _lib.SDRX_ESTATE for i in range(len(topo.vfos))), "a refused call changes nothing"
    # sdrx_set_detector's refusal of non-zero reserved words stays
    assert L.sdrx_set_detector(rx.h, 1, C.byref(_lib.DetectCfgC(dt.FM, (C.c_int32 * 3)(0, 1, 0)))) == _lib.SDRX_EINVAL
    # read-back before finalize: the taps, bit for bit; out_len not known yet
    rx.set_postfilter(1, h, 2)
    rx.set_postfilter(2, h[:17], 16)
    rx.set_postfilter(2, None)  # taken away again
    got = rx.postfilter(1)
    assert (got["decim"], got["ntaps"], got["out_len"], got["delay_samples"], got["pass_hz"], got["stop_hz"]) == (2, 64, 0, 31.5, 0.0, 0.0)
    assert _same(got["taps"], h) and _code(lambda: rx.postfilter(2)) == _lib.SDRX_ESTATE
    few = np.full(8, 7.0, np.float32)
    assert L.sdrx_get_postfilter(rx.h, 1, C.byref(info), few.ctypes.data, 5) == 0 and _same(few[:5], h[:5]) and np.all(few[5:] == 7.0)
    rx.finalize()
    assert rx.postfilter(1)["out_len"] == 4096 and rx.output_rate(1) == 15360 // 2
    assert _code(lambda: rx.set_postfilter(2, h, 2)) == _lib.SDRX_ESTATE and _code(lambda: rx.set_postfilter(1, None)) == _lib.SDRX_ESTATE
    assert rx.postfilter(1)["ntaps"] == 64
    rx.close()
    # a post filter without a detector (an IQ leaf, a USB leaf, a node with children): refused at finalize
    for i in (5, 4, 0):
        rx = Receiver()
        for v in topo.vfos:
            rx.add_vfo(dataclasses.replace(v, post_taps=(), post_decim=1))
        rx.set_postfilter(i, h, 2)
        assert _code(rx.finalize) == _lib.SDRX_EINVAL, i
        assert b"no detector" in L.sdrx_last_error(rx.h) or i == 0
        rx.close()
    # n % R != 0: SDRX_EUNSUPPORTED at finalize, with the reason
    rx = Receiver()
    for v in topo.vfos:
        rx.add_vfo(dataclasses.replace(v, post_taps=(), post_decim=1))
    rx.set_postfilter(1, h, 3)  # 8192 % 3
    assert _code(rx.finalize) == _lib.SDRX_EUNSUPPORTED and b"not a multiple of the post-detection decimation 3" in L.sdrx_last_error(rx.h)
    rx.close()
    # groups do not offer it: the wrapper says so, and a member handed out by the group is a finalized context
    with pytest.raises(ValueError):
        Group.from_topology(topo, [0])
    plain = Topology(fs=topo.fs, frame=topo.frame, vfos=[dataclasses.replace(v, detector=0, post_taps=(), post_decim=1) for v in topo.vfos])
    grp = Group.from_topology(plain, [0, 0])
    ctx, _ = grp.member_context(0)
    assert L.sdrx_set_postfilter(ctx, 1, cfg(2, 64), h.ctypes.data) == _lib.SDRX_ESTATE
    grp.close()


# ---- 12. sdrx_demo needs nothing but the INI ---------------------------------------------------------------------------------------------
def _fnv1a(b: bytes) -> int:
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_demo_on_the_ini(tmp_path):
    """host/sdrx_demo on a copy of sdr_25E.ini with a filtered AM, a filtered FM and an unfiltered FM entry: the messages of the
    C++ host (vfo::setPostFilter behind the INI keys) are those of the Python host on the same topology; the filtered entries'
    are int16 at 48 kS/s / post_decim"""
    import os
    import subprocess
    from oracle import binding as ob
    from sdrreceiver_amd import synth
    from test_postdet_model import ROOT, postfilter_ini
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "sdrx_demo"], stdout=subprocess.DEVNULL)
    text, topo = postfilter_ini()
    p = tmp_path / "postdet.ini"
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
    for name, rate, nbytes in (("AIR01", 8000, 2 * 2000), ("AIS01", 48000, 2 * 12000), ("POC01", 48000, 2 * 12000)):
        rows = [r for r in got if r[1] == name]
        assert len(rows) == 2 and all(r[2] == str(rate) and r[3] == str(nbytes) for r in rows), rows
