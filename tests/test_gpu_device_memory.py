"""Who owns the device memory of a context, seen from outside: sdrx_get_stats().device_bytes is a sum over the buffers the
options hold, so it follows them as they grow and is the same however a context reached its state; the job lists of the
setters grow without being counted; and a context that has made every first use gives all of it back when it is destroyed.
(What an allocation that FAILS leaves behind is walked on the host: tests/test_device_memory_host.py.)"""
import numpy as np
import pytest

import drift_ref as dr
import watch_ref as wr
from helpers import golden_topology
from sdrreceiver_amd import synth
from sdrreceiver_amd.receiver import SPECTRUM_RAW, Receiver

pytestmark = pytest.mark.gpu

SCAN = dict(cell_bins=4, frames=1, floor_permille=500, ratio_q8=16 * 256, min_cells=1)
AGC = dict(lo_ms=100, hi_ms=10000, silent_ms=1, hold_frames=2, up=1.25, down=0.8, gain_min=0.001, gain_max=1.0)


def _bytes(rx):
    return rx.stats()["device_bytes"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _along(topo, opts, steps):
    """device_bytes of one context after each of `steps` (functions of the receiver), each checked against a fresh context that
    is brought to the same state in one go by `fresh` -- the steps' second entry -- alone"""
    rx = Receiver.from_topology(topo, **opts)
    seen = [_bytes(rx)]
    for k, (step, fresh) in enumerate(steps):
        step(rx)
        seen.append(_bytes(rx))
        twin = Receiver.from_topology(topo, **opts)
        assert _bytes(twin) == seen[0], k
        fresh(twin)
        assert _bytes(twin) == seen[-1], (k, seen)
        twin.close()
    return rx, seen


def test_device_bytes_follows_the_watch_and_the_wake_as_they_grow():
    topo = wr.watch_tree()
    leaves = topo.leaves_in_publish_order()
    on = [1] * len(leaves)
    iq = wr.tone_frame(topo, wr.tone_for(topo, 1), seed=3)

    def watch_all(rx):
        rx.set_watch(leaves, on)

    def watch_all_wake_one(rx):
        watch_all(rx)
        rx.set_wake([1], 0.0)

    def watch_all_wake_all(rx):
        watch_all(rx)
        rx.set_wake(leaves, 0.0)

    rx, seen = _along(topo, dict(wake=True), [
        (lambda r: r.set_watch([1], [1]), lambda r: r.set_watch([1], [1])),
        (watch_all, watch_all),                                      # (one source on this tree: the data stays as large)
        (lambda r: r.set_wake([1], 0.0), watch_all_wake_one),
        (lambda r: r.set_wake(leaves, 0.0), watch_all_wake_all),     # the fill list of every leaf: it grows
    ])
    assert seen[0] < seen[1] <= seen[2] < seen[3] < seen[4], seen
    rx.process(iq)
    assert _bytes(rx) == seen[4] + 10 * topo.frame  # (the host-fed frame's buffers, as the figure has always counted them)
    held = _bytes(rx)
    rx.set_wake(leaves, 0.0, on=0)
    rx.set_watch(leaves, [0] * len(leaves))
    assert _bytes(rx) == held  # the state stays allocated
    rx.process(iq)
    assert _bytes(rx) == held
    rx.close()


def test_device_bytes_follows_the_analyses_of_two_sources():
    topo = dr.drift_tree(8704)
    a, b = dr.DT_PARENT_LEAF, dr.DT_RAW_LEAF  # a leaf of the main's stream, a leaf of the raw frame
    iq = dr.raw_frame(topo, 0.0, seed=5)

    def both(rx):
        rx.set_watch([a, b], [1, 1])

    def both_a(rx):
        both(rx)
        rx.set_drift(a, max_shift=8)
        rx.set_scan(a, **SCAN)

    def both_ab(rx):
        both_a(rx)
        rx.set_drift(b, max_shift=8)
        rx.set_scan(b, **SCAN)

    def only_a(rx):
        rx.set_watch([a], [1])
        rx.set_drift(a, max_shift=8)
        rx.set_scan(a, **SCAN)

    rx, seen = _along(topo, dict(watch=True), [
        (lambda r: r.set_watch([a], [1]), lambda r: r.set_watch([a], [1])),
        (lambda r: (r.set_drift(a, max_shift=8), r.set_scan(a, **SCAN)), only_a),
        (lambda r: r.set_watch([b], [1]), both_a),                   # another source joins: the data buffer grows
        (lambda r: (r.set_drift(b, max_shift=8), r.set_scan(b, **SCAN)), both_ab),
    ])
    assert seen[0] < seen[1] < seen[2] < seen[3] < seen[4], seen
    rx.process(iq)
    assert rx.drift(a)["measured"] == 1 and rx.scan(b)["measured"] == 1  # (the grown buffers are the ones the frame used)
    held = _bytes(rx)
    for leaf in (a, b):
        rx.set_drift(leaf, max_shift=0)
        rx.set_scan(leaf, cell_bins=0)
    rx.set_watch([a, b], [0, 0])
    assert _bytes(rx) == held  # the state stays allocated
    rx.process(iq)
    assert _bytes(rx) == held
    rx.close()


def test_job_lists_grow_without_being_counted():
    """Every setter with a job list, for one leaf and then for all of them (the list grows): device_bytes does not move, and the
    next frame is that of a fresh context that was given the lists at their full length at once."""
    topo = wr.watch_tree()
    leaves = topo.leaves_in_publish_order()
    usb = [i for i in leaves if topo.vfos[i].demod_usb]
    iq = wr.tone_frame(topo, wr.tone_for(topo, 2), seed=7)
    gains = [float(np.float32(0.002 + 0.0005 * k)) for k in range(len(usb))]
    active = [0 if i in (1, 3, 5) else 1 for i in leaves]
    opts = dict(meter=True, squelch=True, agc=True, park=True)

    def settle(rx, ids_usb, ids):
        rx.set_gains(ids_usb, [gains[usb.index(i)] for i in ids_usb])
        rx.set_squelch(ids, [1] * len(ids), [2] * len(ids))
        rx.set_agc(ids_usb, **AGC)
        rx.set_active(ids, [active[leaves.index(i)] for i in ids])

    grown, fresh = Receiver.from_topology(topo, **opts), Receiver.from_topology(topo, **opts)
    for rx in (grown, fresh):
        rx.process(iq)
    held = _bytes(grown)
    settle(grown, usb[:1], leaves[:1])
    assert _bytes(grown) == held
    settle(grown, usb, leaves)
    assert _bytes(grown) == held == _bytes(fresh)
    settle(fresh, usb, leaves)
    for rx in (grown, fresh):
        rx.process(iq)
    assert [int(v) for v in grown.active(leaves)["active"]] == active
    for i in leaves:
        assert np.array_equal(_bits(grown.output(i)), _bits(fresh.output(i))), i
        assert grown.output(i).size == (0 if i in (1, 3, 5) else fresh.output(i).size)
    mg, mf = grown.meters(leaves), fresh.meters(leaves)
    for key in mg:
        assert np.array_equal(_bits(mg[key]), _bits(mf[key])), key
    ag, af = grown.agc(usb), fresh.agc(usb)
    for key in ag:
        assert np.array_equal(_bits(ag[key]), _bits(af[key])), key
    assert _bytes(grown) == held
    grown.close()
    fresh.close()


def test_contexts_that_made_every_first_use_do_not_leak_device_memory():
    """test_gpu_parity.py::test_contexts_do_not_leak_device_memory -- the same tree, 30 cycles and bound -- with a cycle that makes
    the context allocate everything it can: integer frames of both sample sizes with DC removal, a VFO's and the raw spectrum,
    two taps on fused leaves (the second gets a buffer of its own), watch, drift, scan and wake, a catch-up, an NCO read."""
    import torch
    topo = golden_topology("profile_25e")
    iq = synth.lcg_frame(topo.frame, synth.Lcg(2))
    u8, s8, s16 = (iq + 127).astype(np.uint8), iq.astype(np.int8), (iq * 100).astype(np.int16)
    fused = [i for i, v in enumerate(topo.vfos) if v.parent >= 0 and v.decimate_count == 2 and v.filter_bw == 0][:2]
    assert len(fused) == 2

    def cycle():
        rx = Receiver.from_topology(topo, fuse_demod=True, wake=True, catchup=True)
        rx.set_spectrum(2)
        rx.set_spectrum(SPECTRUM_RAW)
        for i in fused:
            rx.add_tap(i)
        rx.set_watch([3, 16], [1, 1])  # a leaf of either main: two sources
        rx.set_drift(3, max_shift=4)
        rx.set_scan(16, **SCAN)
        rx.set_wake([3], 0.0)
        rx.set_active([4], [0])
        rx.process(iq)
        rx.process_u8(u8, correct_dc=True)
        rx.set_active([4], [1])
        assert int(rx.catchup([4])["frame"][0]) == 1  # (caught up in the frame before the one it was unparked for)
        rx.process_fmt(s8, correct_dc=True)
        rx.process_fmt(s16, correct_dc=True)
        assert rx.stream(fused[1]).size == topo.vfos[fused[1]].samples_per_buffer // 4
        rx.nco(2, 0, 64)
        rx.close()

    cycle()  # one-time allocations of the runtime (code objects, scratch) happen here
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(30):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 << 20, (free0, free1)  # a context of this profile holds ~30 MB: 30 leaked ones would show
