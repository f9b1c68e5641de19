"""Output meters (option "meter"): on every leaf, every launch path and every arithmetic the device's figures equal
meters_from_payload of the payload the leaf delivered (exact equality); metering changes no payload bit; the records
travel with the payloads (in flight, groups); suggest_gains + set_gains closes the loop."""
import numpy as np
import pytest

from sdrreceiver_amd import _lib, meter, synth, topology as tp
from helpers import tree_mixed

pytestmark = pytest.mark.gpu

N_FRAMES = 3


@pytest.fixture(scope="module")
def R():
    from sdrreceiver_amd.receiver import Receiver
    return Receiver


TREES = {"config3": lambda: tp.config3(1024), "config4": lambda: tp.config4(256), "mixed": tree_mixed}


def leaves(topo):
    parents = {v.parent for v in topo.vfos}
    return [i for i in range(len(topo.vfos)) if i not in parents]


def same_peak(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


def check(rx, topo, ctx, frame=None, vids=None):
    """every leaf's meter equals the reference definition on what the leaf delivered"""
    vids = leaves(topo) if vids is None else vids
    m = rx.meters(vids)
    for k, v in enumerate(vids):
        d = topo.vfos[v]
        ref = meter.meters_from_payload(d, rx.output(v), rx.prequant(v) if d.demod_usb else rx.stream(v))
        got = (int(m["n_values"][k]), int(m["sum_sq"][k]), int(m["clipped"][k]))
        assert got == (ref["n_values"], ref["sum_sq"], ref["clipped"]), (ctx, v, got, ref)
        assert same_peak(m["peak"][k], ref["peak"]), (ctx, v, m["peak"][k], ref["peak"])
        if frame is not None:
            assert m["frame"][k] == frame, (ctx, v)
    return m


def frames(topo, n=N_FRAMES, seed=5, u8=False):
    lcg = synth.Lcg(seed)
    return [(synth.lcg_frame_u8 if u8 else synth.lcg_frame)(topo.frame, lcg) for _ in range(n)]


PATHS = ["process", "process_u8_dc", "submit_wait", "device_tail", "device_no_tail", "fuse_demod", "no_fuse_late"]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("exact", [1, 0, 2])
@pytest.mark.parametrize("tree", list(TREES))
def test_meters_equal_the_payload_definition(R, tree, exact, path):
    topo = TREES[tree]()
    kw = dict(device=0, exact=exact, keep_prequant=True, meter=True)
    kw.update({"device_tail": dict(tail_in_levels=True), "device_no_tail": dict(tail_in_levels=False),
               "fuse_demod": dict(fuse_demod=True), "no_fuse_late": dict(fuse_late=False)}.get(path, {}))
    rx = R.from_topology(topo, **kw)
    ctx = (tree, exact, path)
    if path == "process_u8_dc":
        for f, b in enumerate(frames(topo, u8=True)):
            rx.process_u8(b, correct_dc=True)
            check(rx, topo, ctx + (f,), frame=f)
    elif path == "submit_wait":
        fr = frames(topo)
        rx.submit(fr[0])
        for f in range(1, len(fr)):
            rx.submit(fr[f])
            rx.wait()
        rx.wait()
        check(rx, topo, ctx, frame=len(fr) - 1)
    elif path.startswith("device"):
        import torch
        t = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() for x in frames(topo)]
        torch.cuda.synchronize()
        for x in t:
            rx.process_device(x.data_ptr(), topo.frame)
        check(rx, topo, ctx, frame=len(t) - 1)  # meters() runs what the software pipeline holds, then fetches
        rx.process_device(t[0].data_ptr(), topo.frame)
        rx.fetch()
        check(rx, topo, ctx, frame=len(t))
    else:
        for f, x in enumerate(frames(topo)):
            rx.process(x)
            check(rx, topo, ctx + (f,), frame=f)
    rx.close()


@pytest.mark.parametrize("exact", [1, 0])
def test_wrapped_samples_are_counted_and_payloads_unchanged(R, exact):
    topo = tree_mixed()
    on = R.from_topology(topo, device=0, exact=exact, keep_prequant=True, meter=True)
    off = R.from_topology(topo, device=0, exact=exact, keep_prequant=True)
    loud = [2, 4, 6]
    fr = frames(topo, 4, seed=9)
    for f, x in enumerate(fr):
        if f == 1:
            for rx in (on, off):
                rx.set_gains(loud, [topo.vfos[v].gain * 3000.0 for v in loud])
        on.process(x)
        off.process(x)
        m = check(on, topo, ("wrap", exact, f), frame=f)
        for v in leaves(topo):
            assert np.array_equal(on.output(v).view(np.uint8), off.output(v).view(np.uint8)), (f, v)
        if f >= 1:
            lv = leaves(topo)
            assert all(m["clipped"][lv.index(v)] > 0 for v in loud), m["clipped"]
    on.close()
    off.close()


def test_config3_payloads_bit_identical_with_meter_off(R):
    topo = tp.config3(1024)
    on = R.from_topology(topo, device=0, meter=True)
    off = R.from_topology(topo, device=0)
    plain = R.from_topology(topo, device=0, meter=False)
    from sdrreceiver_amd.receiver import SdrxError
    with pytest.raises(SdrxError) as e:
        off.meters([2])
    assert e.value.code == _lib.SDRX_ESTATE
    with pytest.raises(SdrxError) as e:
        on.meters([2])  # nothing delivered yet
    assert e.value.code == _lib.SDRX_ESTATE
    for f, x in enumerate(frames(topo, 3, seed=3)):
        for rx in (on, off, plain):
            rx.process(x)
        for v in leaves(topo):
            assert np.array_equal(on.output(v), off.output(v)), (f, v)
    with pytest.raises(SdrxError) as e:
        off.meters([2])
    assert e.value.code == _lib.SDRX_ESTATE
    for bad in ([0], [1], [len(topo.vfos)], [-1]):  # mains have children: no meter
        with pytest.raises(SdrxError) as e:
            on.meters(bad)
        assert e.value.code == _lib.SDRX_EINVAL
    assert on.meters([])["frame"].size == 0
    # (measured after frames of the same form: the host-frame staging is allocated by the first one)
    assert off.stats()["device_bytes"] == plain.stats()["device_bytes"] < on.stats()["device_bytes"]
    for rx in (on, off, plain):
        rx.close()


def test_in_flight_meters_belong_to_the_delivered_frame(R):
    topo = tp.config3(1024)
    fr = frames(topo, 4, seed=13)
    sync = R.from_topology(topo, device=0, meter=True)
    ref = []
    for x in fr:
        sync.process(x)
        ref.append((sync.meters(leaves(topo)), [sync.output(v) for v in leaves(topo)]))
    pipe = R.from_topology(topo, device=0, meter=True)
    pipe.submit(fr[0])
    pipe.wait()
    for f in range(1, len(fr)):
        pipe.submit(fr[f])  # frame f in flight: frame f - 1 is what output() and meters() serve
        m = pipe.meters(leaves(topo))
        rm, rout = ref[f - 1]
        assert (m["frame"] == f - 1).all()
        for key in ("n_values", "sum_sq", "clipped"):
            assert np.array_equal(m[key], rm[key]), (f, key)
        assert np.array_equal(m["peak"].view(np.uint32), rm["peak"].view(np.uint32))
        for k, v in enumerate(leaves(topo)):
            assert np.array_equal(pipe.output(v), rout[k]), (f, v)
        pipe.wait()
    for rx in (sync, pipe):
        rx.close()


def test_group_reports_the_single_context_meters(R):
    from sdrreceiver_amd.receiver import Group
    topo = tp.config3(1024)
    single = R.from_topology(topo, device=0, meter=True)
    grp = Group.from_topology(topo, devices=[0, 0, 0, 0], meter=1)
    lv = leaves(topo)
    assert len({grp.locate(v)[0] for v in lv}) == 4
    for f, x in enumerate(frames(topo, 2, seed=17)):
        single.process(x)
        grp.process(x)
        a, b = single.meters(lv), grp.meters(lv)
        for key in ("frame", "n_values", "sum_sq", "clipped"):
            assert np.array_equal(a[key], b[key]), (f, key)
        assert np.array_equal(a["peak"].view(np.uint32), b["peak"].view(np.uint32))
        assert (b["frame"] == f).all()
    single.close()
    grp.close()


def test_closed_loop_reaches_the_target(R):
    topo = tp.config3(1024)
    rx = R.from_topology(topo, device=0, meter=True)
    x = frames(topo, 1, seed=23)[0]  # the same frame every time: the level moves only with the gain
    for _ in range(2):
        rx.process(x)
    lv = leaves(topo)
    m = rx.meters(lv)
    target = min(float(np.median(m["rms_dbfs"])) + 2.0, -20.0)
    pick = [k for k in range(len(lv)) if abs(m["rms_dbfs"][k] - target) < 5.0 and m["clipped"][k] == 0]
    assert len(pick) >= 100, (target, np.percentile(m["rms_dbfs"], [5, 50, 95]))
    vids = [lv[k] for k in pick]
    g0 = np.array([topo.vfos[v].gain for v in vids], np.float32)
    g1 = meter.suggest_gains(g0, {k: val[pick] for k, val in m.items()}, target_rms_dbfs=target)
    rx.set_gains(vids, g1)
    for _ in range(2):
        rx.process(x)
    after = rx.meters(vids)
    assert np.abs(after["rms_dbfs"] - target).max() < 0.2, np.abs(after["rms_dbfs"] - target).max()
    assert (after["clipped"] == 0).all()
    rx.close()
