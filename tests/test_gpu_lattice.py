"""The HIP path on the lattice of tests/lattice.py: the decimation depths and tree positions no other test tree draws.

What runs here and nowhere else: the shaped d = 5 body on parent streams of 3, 4, 5 and 8 chunks with and without a partial
last one (every parity of its chunk pairing, every "finish this chunk alone" exit); leaves at d = 6, 7, 8 below a tiled parent
(the generic half-band stages with 16, 8 and 4 outputs per chunk against a 16-entry carry, warm-ups of 630 to 2 550 samples);
inner nodes at d = 4, 5, 6 (the tile layout written out of the LDS stages); the /5 and /6 late decimation behind d = 1 ... 8
and fused on leaf frames of 2 to 5 late-chunks; compress() dividing by 3, 5, 7, 10 and 100; mixers at 0, next to and beyond
Nyquist.  References (lattice.oracle_frames: the plain-C oracle, pinned to the real reference build on exactly these trees by
tests/test_lattice_model.py; lattice.model_frames: live_ref.ModelTree under lattice.schedule) are computed once per tree and
shared.

Bars: the exact arithmetic bit for bit; the tolerance and the robust arithmetic within 1e-5 of max|reference| per VFO-frame
and int16 within 1 LSB (BASELINE north star) -- test_gpu_parity.py's own checkers.  On these inputs the reference's -O2 and
-Ofast builds differ by at most 4.3e-7 (tests/golden/lattice.npz, provenance).

sdrx_finalize takes every lattice tree: no cell ends as a documented refusal."""
import numpy as np
import pytest

import lattice as lt
from sdrreceiver_amd import meter
from test_gpu_live_random import REL_TOL, _apply_ops, _check_after, _drive, _int8_within_one
from test_gpu_live_random import _check_exact as _check_model
from test_gpu_parity import _check_exact, _check_tolerance

pytestmark = pytest.mark.gpu

TREES = lt.trees()
NAMES = sorted(TREES)
SEGMENTS = [0, 1, 2, 3, 5]


@pytest.fixture(scope="module")
def Receiver():
    from sdrreceiver_amd.receiver import Receiver as R
    return R


@pytest.fixture(scope="module")
def device_frames():
    """name -> the raw frames on the device (uploaded once)."""
    import torch
    dev = {name: [torch.from_numpy(np.array(iq)).cuda() for iq in lt.frames(name)] for name in NAMES}
    torch.cuda.synchronize()
    return dev


def _published(topo, snaps):
    out = []
    for i in topo.leaves_in_publish_order():
        d = topo.vfos[i]
        out.append((d.topic.encode()[:5].ljust(5, b"\0"), d.output_rate, (snaps[i].usb() if d.demod_usb else snaps[i].iq()).tobytes()))
    return out


# ------------------------------------------------------------------------------ exact arithmetic
@pytest.mark.parametrize("segments", SEGMENTS)
def test_exact_process(Receiver, segments):
    for name in NAMES:
        topo, want = TREES[name], lt.oracle_frames(name)
        rx = Receiver.from_topology(topo, exact=True, segments=segments)
        for f, iq in enumerate(lt.frames(name)):
            rx.process(iq)
            _check_exact(rx, want[f], topo, (name, segments, f))
            assert rx.published == _published(topo, want[f]), (name, segments, f)
        rx.close()


def test_exact_submit_wait_two_in_flight(Receiver):
    for k, name in enumerate(NAMES):
        topo, want, frames = TREES[name], lt.oracle_frames(name), lt.frames(name)
        rx = Receiver.from_topology(topo, exact=True, segments=SEGMENTS[k % 5])
        rx.submit(frames[0])
        for f in range(1, len(frames)):
            rx.submit(frames[f])
            assert rx.in_flight() == 2
            rx.wait()
            assert rx.published == _published(topo, want[f - 1]), (name, f - 1)
        rx.wait()
        assert rx.in_flight() == 0 and rx.published == _published(topo, want[-1]), name
        _check_exact(rx, want[-1], topo, (name, "submit"))
        rx.close()


QUEUED = {"defaults": dict(), "separate kernels": dict(fuse=False), "demodulation in the wave": dict(fuse_demod=True)}


@pytest.mark.parametrize("mode", sorted(QUEUED))
@pytest.mark.parametrize("segments", SEGMENTS)
def test_exact_queued_device_frames(Receiver, device_frames, mode, segments):
    """sdrx_process_device back to back (the software pipeline of k_mix_levels and the leaf tail inside it, by default), a
    fetch after the third frame and one at the end."""
    for name in NAMES:
        topo, want = TREES[name], lt.oracle_frames(name)
        rx = Receiver.from_topology(topo, exact=True, segments=segments, **QUEUED[mode])
        for f, d in enumerate(device_frames[name]):
            rx.process_device(d.data_ptr(), topo.frame)
            if f == 2:
                rx.fetch()
                _check_exact(rx, want[2], topo, (name, mode, segments, "middle"))
        rx.fetch()
        _check_exact(rx, want[-1], topo, (name, mode, segments, "end"))
        rx.close()


@pytest.mark.parametrize("fuse_late", [True, False])
@pytest.mark.parametrize("segments", SEGMENTS)
def test_exact_late_trees_keeping_streams(Receiver, device_frames, fuse_late, segments):
    """keep_streams = 1: every late leaf keeps decimate[d], fused or not, so the stream in front of the decimating low-pass is
    compared too.  Synchronous frames, then the same context queued."""
    for name in lt.LATE_TREES:
        topo, want = TREES[name], lt.oracle_frames(name)
        rx = Receiver.from_topology(topo, exact=True, segments=segments, keep_streams=True, fuse_late=fuse_late)
        for f, iq in enumerate(lt.frames(name)[:3]):
            rx.process(iq)
            assert all(rx.stream(i) is not None for i in range(len(topo.vfos))), (name, "keep_streams")
            _check_exact(rx, want[f], topo, (name, fuse_late, segments, f))
        for d in device_frames[name][3:]:
            rx.process_device(d.data_ptr(), topo.frame)
        rx.fetch()
        _check_exact(rx, want[-1], topo, (name, fuse_late, segments, "queued"))
        rx.close()


# ------------------------------------------------------------------------------ tolerance and robust arithmetic
@pytest.mark.parametrize("form", ["process", "queued"])
@pytest.mark.parametrize("arith", ["tolerance", "robust"])
def test_tolerance_arithmetics(Receiver, device_frames, arith, form):
    for k, name in enumerate(NAMES):
        topo, want = TREES[name], lt.oracle_frames(name)
        rx = Receiver.from_topology(topo, exact=arith, keep_prequant=True, keep_streams=k % 2 == 0, segments=SEGMENTS[k % 5])
        if form == "process":
            for f, iq in enumerate(lt.frames(name)):
                rx.process(iq)
                _check_tolerance(rx, want[f], topo, (name, arith, f))
        else:
            for f, d in enumerate(device_frames[name]):
                rx.process_device(d.data_ptr(), topo.frame)
                if f == 2:
                    rx.fetch()
                    _check_tolerance(rx, want[2], topo, (name, arith, "queued, middle"))
            rx.fetch()
            _check_tolerance(rx, want[-1], topo, (name, arith, "queued, end"))
        for i, d in enumerate(topo.vfos):  # (the checker above leaves the int8 payloads alone)
            if not topo.children(i) and not d.demod_usb:
                assert _int8_within_one(rx.output(i), want[-1][i].iq(), d.cstyle), (name, arith, i, "int8")
        rx.close()


# ------------------------------------------------------------------------------ options on the deep cells
def _same_peak(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


def test_meters_on_the_lattice(Receiver):
    """meter = 1: every leaf's record equals meter.meters_from_payload of the oracle's payload (and pre-quantisation values),
    and no payload or stream changes."""
    for k, name in enumerate(NAMES):
        topo, want = TREES[name], lt.oracle_frames(name)
        leaves = topo.leaves_in_publish_order()
        rx = Receiver.from_topology(topo, exact=True, meter=True, segments=SEGMENTS[k % 5])
        for f, iq in enumerate(lt.frames(name)):
            rx.process(iq)
            _check_exact(rx, want[f], topo, (name, "meter", f))
            m = rx.meters(leaves)
            for q, i in enumerate(leaves):
                d, w = topo.vfos[i], want[f][i]
                ref = meter.meters_from_payload(d, w.usb(), w.usb_prequant().astype(np.float32)) if d.demod_usb else \
                    meter.meters_from_payload(d, w.iq(), w.stream())
                got = (int(m["n_values"][q]), int(m["sum_sq"][q]), int(m["clipped"][q]))
                assert got == (ref["n_values"], ref["sum_sq"], ref["clipped"]) and int(m["frame"][q]) == f, (name, f, i, got, ref)
                assert _same_peak(m["peak"][q], ref["peak"]), (name, f, i, m["peak"][q], ref["peak"])
        rx.close()


def test_park_with_nothing_parked_changes_nothing(Receiver, device_frames):
    """park = 1 selects the PARK instantiations of the kernels; with every leaf active they compute what the option off does."""
    for k, name in enumerate(NAMES):
        topo, want = TREES[name], lt.oracle_frames(name)
        rx = Receiver.from_topology(topo, exact=True, park=True, segments=SEGMENTS[k % 5])
        for f, iq in enumerate(lt.frames(name)[:3]):
            rx.process(iq)
            _check_exact(rx, want[f], topo, (name, "park", f))
            assert rx.published == _published(topo, want[f]), (name, f)
        for d in device_frames[name][3:]:
            rx.process_device(d.data_ptr(), topo.frame)
        rx.fetch()
        _check_exact(rx, want[-1], topo, (name, "park", "queued"))
        rx.close()


@pytest.mark.parametrize("form", ["process", "device"])
def test_live_controls_exact(Receiver, form):
    """lattice.schedule -- a retune of the deepest sub leaf and of the deepest inner node, a gain change, a d >= 6 leaf, a late
    leaf and an IQ leaf parked and unparked -- against live_ref.ModelTree: payloads, streams, meters, publish order, bit for
    bit, and the oscillator tables and park states afterwards."""
    for k, name in enumerate(NAMES):
        topo = TREES[name]
        want, descs = lt.model_frames(name)
        sched = lt.schedule(topo)
        rx = Receiver.from_topology(topo, exact=True, park=True, meter=True, segments=SEGMENTS[k % 5], keep_streams=k % 2 == 1)
        ctx = (name, form)
        seen = _drive(rx, topo, [np.array(iq) for iq in lt.frames(name)], sched, form, lambda f, s: _check_model(rx, topo, want[f], f, ctx, s), k)
        assert seen and seen[-1] == lt.N_FRAMES - 1, (ctx, seen)
        _check_after(rx, topo, sched, want, descs, ctx)
        rx.close()


def test_live_controls_robust(Receiver):
    """The same schedule once in the robust arithmetic: streams within 1e-5 of max|model stream|, int16 within 1 LSB, int8
    within 1; a parked leaf delivers nothing."""
    for k, name in enumerate(NAMES):
        topo = TREES[name]
        want, _ = lt.model_frames(name)
        sched = lt.schedule(topo)
        rx = Receiver.from_topology(topo, exact=2, park=True, keep_streams=True, segments=SEGMENTS[k % 5])
        for f, iq in enumerate(lt.frames(name)):
            _apply_ops(rx, sched[f])
            rx.process(iq)
            w = want[f]
            for i, d in enumerate(topo.vfos):
                z, got = w["streams"][i], rx.stream(i, missing_ok=True)
                if z is None:
                    assert got is None and rx.output(i).size == 0, (name, f, i, "a parked leaf")
                    continue
                assert got is not None, (name, f, i)
                ratio = float(np.abs(got - z).max()) / float(np.abs(z).max())
                assert ratio <= REL_TOL, (name, f, i, "stream", ratio)
                if topo.children(i):
                    continue
                pay, ref = rx.output(i), w["payload"][i]
                assert pay.size == ref.size, (name, f, i)
                if d.demod_usb:
                    assert int(np.abs(pay.astype(np.int32) - ref.astype(np.int32)).max()) <= 1, (name, f, i, "int16")
                else:
                    assert _int8_within_one(pay, ref, d.cstyle), (name, f, i, "int8")
        rx.close()


def test_squelch_with_zero_thresholds_changes_nothing(Receiver):
    """squelch = 1, every threshold 0: every leaf is open in every frame, and the gated egress delivers what the option off
    does -- on the widest tree (d = 0 ... 8 USB leaves, IQ leaves at d = 5 ... 8)."""
    name = lt.WIDEST
    topo, want = TREES[name], lt.oracle_frames(name)
    leaves = topo.leaves_in_publish_order()
    rx = Receiver.from_topology(topo, exact=True, squelch=True)
    rx.set_squelch(leaves, [0] * len(leaves), [0] * len(leaves))
    for f, iq in enumerate(lt.frames(name)):
        rx.process(iq)
        assert rx.published == _published(topo, want[f]), (name, f)
        assert [int(v) for v in rx.squelch(leaves)["open"]] == [1] * len(leaves), (name, f)
        for i in leaves:
            assert np.array_equal(rx.output(i), want[f][i].usb() if topo.vfos[i].demod_usb else want[f][i].iq()), (name, f, i)
    rx.close()


def test_group_of_three_equals_the_single_context():
    """The widest tree on sdrx_group_* with 3 members on one device (its one main is replicated on each): what the callback
    publishes, in the reference's order over the whole tree, is the oracle's -- which is what the single context gives."""
    from sdrreceiver_amd.receiver import Group
    name = lt.WIDEST
    topo, want = TREES[name], lt.oracle_frames(name)
    g = Group.from_topology(topo, [0, 0, 0])
    assert len({g.locate(i)[0] for i in topo.leaves_in_publish_order()}) == 3
    for f, iq in enumerate(lt.frames(name)):
        g.process(iq)
        assert [p[0] for p in g.published] == [p[0] for p in _published(topo, want[f])], (f, "topics / order")
        assert g.published == _published(topo, want[f]), (f, "payloads")
    g.close()
