"""Channel watch on the device (option "watch", sdrx_set_watch / sdrx_get_watch / sdrx_get_watch_psd and their group forms)
against the numpy model tests/watch_ref.py.

The PSD is compared BIT FOR BIT on the stream the device itself holds (Receiver.stream(parent) / Receiver.raw() / the device
frame); band_pwr and total_pwr against math.fsum over the returned PSD within n_terms * 2^-53 relative (every term is
non-negative: any summation order lies inside that)."""
import dataclasses
import functools
import math

import numpy as np
import pytest

import lattice
import retune_ref as rr
import watch_ref as wr
from sdrreceiver_amd import _lib, synth, watch
from sdrreceiver_amd.receiver import Group, Receiver, SdrxError
from sdrreceiver_amd.topology import Topology, VfoDesc

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


def _leaves(topo):
    return [i for i in range(len(topo.vfos)) if not topo.children(i)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def small_tree(n_parent: int) -> Topology:
    """A main at d = 3 whose stream has n_parent samples per frame, two USB subs and a compress sub below it, and two
    parent-less leaves (sources: the parent's tile-layout stream and the raw frame of 8 n_parent samples)."""
    n = 8 * n_parent
    t = Topology(fs=4 * n, frame=n, name=f"watch-{n_parent}")
    t.vfos.append(VfoDesc(parent=-1, fs=4 * n, decimate_count=3, mixer_freq=float(n // 3 + 37), demod_usb=False, cstyle=1,
                          samples_per_buffer=n))
    s = dict(parent=0, fs=n // 2, samples_per_buffer=n_parent, cstyle=1)
    t.vfos.append(VfoDesc(topic="S1", decimate_count=2, mixer_freq=float(n // 16 + 11), gain=0.01, **s))
    t.vfos.append(VfoDesc(topic="S2", decimate_count=2, mixer_freq=-1234.625, filter_bw=n // 64, gain=0.01, **s))
    t.vfos.append(VfoDesc(topic="S3", decimate_count=3, mixer_freq=float(-n // 8), demod_usb=False, scalecomp=4, **s))
    t.vfos.append(VfoDesc(topic="R1", parent=-1, fs=4 * n, decimate_count=4, mixer_freq=float(n + 5), gain=0.01, cstyle=1,
                          samples_per_buffer=n))
    t.vfos.append(VfoDesc(topic="R2", parent=-1, fs=4 * n, decimate_count=3, mixer_freq=float(-n // 2), demod_usb=False, cstyle=0,
                          samples_per_buffer=n))
    return t


@functools.lru_cache(maxsize=None)
def _frames(n, count=4, seed=7):
    lcg = synth.Lcg(seed)
    return [synth.lcg_frame(n, lcg) for _ in range(count)]


@functools.lru_cache(maxsize=None)
def _model_psd(key):
    """cache by the stream's bytes (several leaves share a source)"""
    return wr.psd(np.frombuffer(key, np.complex64))


def model_psd(stream):
    return _model_psd(np.ascontiguousarray(stream, np.complex64).tobytes())


def check_levels(rx, topo, ids, frame, psd_of=None):
    """The records of `ids` for the delivered frame: bins and segments exactly the model's, the sums within the bound of the
    exact sum over the PSD the device returns."""
    lv = rx.watch(ids)
    for k, i in enumerate(ids):
        d = topo.vfos[i]
        fb, nb = wr.band(d)
        n_src = topo.frame if d.parent < 0 else topo.vfos[d.parent].n_stage_out
        assert int(lv["watched"][k]) == 1 and int(lv["frame"][k]) == frame, (i, lv["watched"][k], lv["frame"][k], frame)
        assert (int(lv["first_bin"][k]), int(lv["n_bins"][k]), int(lv["segments"][k])) == (fb, nb, wr.segments(n_src)[0]), (i, d)
        if psd_of is not None:
            band, total = wr.levels(psd_of(i), fb, nb)
            print(f"leaf {i}: band {lv['band_pwr'][k]!r} vs {band!r}, total {lv['total_pwr'][k]!r} vs {total!r}")
            assert abs(lv["band_pwr"][k] - band) <= nb * EPS * band, (i, lv["band_pwr"][k], band)
            assert abs(lv["total_pwr"][k] - total) <= 8192 * EPS * total, (i, lv["total_pwr"][k], total)
    return lv


def check_psd(rx, topo, ids, frame, raw):
    """watch_psd of every leaf of `ids` == the model on the device's own source stream, bit for bit.  `raw`: the raw frame the
    device holds (complex64).  Returns leaf -> PSD."""
    out = {}
    for i in ids:
        p, f = rx.watch_psd(i)
        parent = topo.vfos[i].parent
        src = raw if parent < 0 else rx.stream(parent)
        want = model_psd(src)
        assert f == frame, (i, f, frame)
        assert np.array_equal(_bits(p), _bits(want)), (topo.name, i, "PSD", int((p != want).sum()), float(np.abs(p - want).max()))
        out[i] = p
    return out


# n below, equal to and above 8 192 per parent stream; 8 704 keeps one segment, 24 832 has three whose starts (8 277 apart) are
# no multiple of the tile; the raw frames (8 n) run from 7 to 16 segments, 198 656 > 16 * 8 192 samples among them
@pytest.mark.parametrize("n_parent", [7680, 8192, 8704, 24832])
@pytest.mark.parametrize("exact", [1, 0, 2])
def test_psd_and_levels_f32(n_parent, exact):
    topo = small_tree(n_parent)
    rx = Receiver.from_topology(topo, exact=exact, watch=True)
    ids = _leaves(topo)
    rx.set_watch(ids, [1] * len(ids))
    for f, iq in enumerate(_frames(topo.frame, 2)):
        rx.process(iq)
        psd = check_psd(rx, topo, ids, f, rx.raw())
        check_levels(rx, topo, ids, f, psd.__getitem__)


@pytest.mark.parametrize("kind", ["u8", "u8_dc", "device"])
def test_psd_raw_kinds(kind):
    """The raw source as dongle bytes, as the tile-layout frame the DC-bias removal leaves, and as a caller's device frame."""
    topo = small_tree(8704)
    rx = Receiver.from_topology(topo, watch=True)
    ids = _leaves(topo)
    rx.set_watch(ids, [1] * len(ids))
    lcg = synth.Lcg(3)
    for f in range(2):
        if kind == "device":
            import torch
            iq = synth.lcg_frame(topo.frame, lcg)
            dev = torch.from_numpy(iq).cuda()
            torch.cuda.synchronize()
            rx.process_device(dev.data_ptr(), topo.frame)
            rx.fetch()
            raw = iq.view(np.complex64)
        else:
            rx.process_u8(synth.lcg_frame_u8(topo.frame, lcg), correct_dc=kind == "u8_dc")
            raw = rx.raw()
        psd = check_psd(rx, topo, ids, f, raw)
        check_levels(rx, topo, ids, f, psd.__getitem__)


@functools.lru_cache(maxsize=None)
def _inner_reference():
    """lattice's "inner" tree (leaves on levels 1 and 2), every leaf watched, frame by frame through sdrx_process: the records
    per frame, each checked against the model.  Shared by the launch-form tests (nobody writes into it)."""
    topo = lattice.trees()["inner"]
    frames = list(lattice.frames("inner"))[:4]
    rx = Receiver.from_topology(topo, watch=True)
    ids = _leaves(topo)
    rx.set_watch(ids, [1] * len(ids))
    recs = []
    for f, iq in enumerate(frames):
        rx.process(iq)
        psd = check_psd(rx, topo, ids, f, rx.raw())
        recs.append(check_levels(rx, topo, ids, f, psd.__getitem__))
    return topo, frames, ids, recs


def _same_records(got, want, what):
    for key in ("frame", "band_pwr", "total_pwr", "first_bin", "n_bins", "segments", "watched"):
        assert np.array_equal(_bits(got[key]), _bits(want[key])), (what, key, got[key], want[key])


def test_frame_bookkeeping_submit():
    """Two frames in flight: the records delivered with frame f are frame f's, readable while f + 1 is in flight."""
    topo, frames, ids, recs = _inner_reference()
    assert {lattice.level(topo, i) for i in ids} >= {1, 2}
    rx = Receiver.from_topology(topo, watch=True)
    rx.set_watch(ids, [1] * len(ids))
    delivered = 0
    for f, iq in enumerate(frames):
        rx.submit(iq)
        if rx.in_flight() == 2:
            rx.wait()
            _same_records(check_levels(rx, topo, ids, delivered), recs[delivered], ("submit", delivered))
            with pytest.raises(SdrxError) as e:
                rx.watch_psd(ids[0])
            assert e.value.code == _lib.SDRX_ESTATE
            delivered += 1
    while rx.in_flight():
        rx.wait()
        _same_records(check_levels(rx, topo, ids, delivered), recs[delivered], ("submit", delivered))
        delivered += 1
    assert delivered == len(frames)


@pytest.mark.parametrize("opts", [dict(), dict(frame_pipeline=False), dict(pipeline=True), dict(tail_in_levels=False)])
def test_frame_bookkeeping_device_frames(opts):
    """sdrx_process_device queues frames inside the software pipeline (level l holds frame k - l): three frames queued, then
    fetched, then a fourth."""
    import torch
    topo, frames, ids, recs = _inner_reference()
    rx = Receiver.from_topology(topo, watch=True, **opts)
    rx.set_watch(ids, [1] * len(ids))
    dev = [torch.from_numpy(np.array(iq)).cuda() for iq in frames]
    torch.cuda.synchronize()
    for f in range(3):
        rx.process_device(dev[f].data_ptr(), topo.frame)
    rx.fetch()
    _same_records(check_levels(rx, topo, ids, 2), recs[2], ("device", opts, 2))
    psd = check_psd(rx, topo, ids, 2, frames[2].view(np.complex64))
    check_levels(rx, topo, ids, 2, psd.__getitem__)
    rx.process_device(dev[3].data_ptr(), topo.frame)
    rx.fetch()
    _same_records(check_levels(rx, topo, ids, 3), recs[3], ("device", opts, 3))


def test_independence_of_parking_and_of_everything_else():
    """A watched leaf reports the same figures parked and active, and a tree with leaves watched delivers what its unwatched
    twin does: payloads, meters, squelch decisions."""
    topo = wr.watch_tree()
    ids = _leaves(topo)
    kw = dict(park=True, meter=True, squelch=True)
    a = Receiver.from_topology(topo, watch=True, **kw)   # watched, some parked
    b = Receiver.from_topology(topo, watch=True, **kw)   # watched, all active
    c = Receiver.from_topology(topo, **kw)               # the unwatched twin of b
    parked = [2, 6, 9]
    a.set_active(parked, [0] * len(parked))
    a.set_watch(ids, [1] * len(ids))
    b.set_watch(ids, [1] * len(ids))
    for rx in (a, b, c):
        rx.set_squelch(ids, [10 ** 7] * len(ids), [1] * len(ids))
    for f in range(3):
        iq = wr.tone_frame(topo, wr.tone_for(topo, 1 + f), seed=f, start=f * topo.frame)
        for rx in (a, b, c):
            rx.process(iq)
        _same_records(a.watch(ids), b.watch(ids), ("parked vs active", f))
        check_levels(a, topo, ids, f)
        for i in ids:
            assert np.array_equal(b.output(i), c.output(i)), (f, i, "payload")
            if i not in parked:
                assert np.array_equal(a.output(i), c.output(i)), (f, i, "payload beside parked leaves")
        mb, mc = b.meters(ids), c.meters(ids)
        sb, sc = b.squelch(ids), c.squelch(ids)
        for key in mb:
            assert np.array_equal(_bits(mb[key]), _bits(mc[key])), (f, "meter", key)
        for key in sb:
            assert np.array_equal(_bits(sb[key]), _bits(sc[key])), (f, "squelch", key)
        assert b.published == c.published, (f, "callbacks")
        assert int(sc["open"].sum()) >= 1  # (the gate decides something: the tone opens a leaf)


def test_retune_then_wake():
    """A parked, watched leaf is retuned onto a tone: its band moves and its contrast rises; wake_list names it; unparked, its
    payload equals a fresh node's from the next frame on (tests/retune_ref.py, pinned to the oracle by test_park_model.py)."""
    topo = wr.watch_tree()
    ids = list(range(1, 9))
    rx = Receiver.from_topology(topo, watch=True, park=True, keep_streams=True)
    rx.set_active(ids, [0] * len(ids))
    rx.set_watch(ids, [1] * len(ids))
    new_f = 11000.0  # a place no sub listens at: band [-11 000, -10 040] of the parent's stream
    spare = 3
    moved = dataclasses.replace(topo.vfos[spare], mixer_freq=new_f)
    lo, hi = wr.band_hz(moved)
    raw_hz = (lo + hi) / 2 - topo.vfos[0].mixer_freq
    rx.process(wr.tone_frame(topo, raw_hz, seed=1))
    before = rx.watch(ids)
    assert watch.wake_list(ids, before, 100.0) == [], watch.contrast(before)
    rx.set_mixer_freqs([spare], [new_f])
    rx.process(wr.tone_frame(topo, raw_hz, seed=2, start=topo.frame))
    after = check_levels(rx, dataclasses.replace(topo, vfos=[moved if i == spare else v for i, v in enumerate(topo.vfos)]), ids, 1,
                         lambda i: rx.watch_psd(i)[0])
    k = ids.index(spare)
    assert (int(after["first_bin"][k]), int(after["n_bins"][k])) == wr.band(moved) != (int(before["first_bin"][k]), int(before["n_bins"][k]))
    assert watch.wake_list(ids, after, 100.0) == [spare], watch.contrast(after)
    rx.set_active([spare], [1])
    fresh = rr.Node(moved)
    for f in (2, 3):
        rx.process(wr.tone_frame(topo, raw_hz, seed=1 + f, start=f * topo.frame))
        fresh.process(rx.stream(0))
        assert np.array_equal(rx.output(spare), fresh.payload()), (f, "the unparked leaf is not a fresh node")
        assert rx.output(1).size == 0


def _launches(rx):
    return {k: v["launches"] for k, v in rx.kernel_times().items()}


def test_option_off_and_errors():
    topo = wr.watch_tree()
    ids = _leaves(topo)
    frames = [wr.tone_frame(topo, wr.tone_for(topo, 2), seed=f, start=f * topo.frame) for f in range(2)]
    off = Receiver.from_topology(topo)
    for call in (lambda: off.set_watch([1], [1]), lambda: off.watch([1]), lambda: off.watch_psd(1)):
        with pytest.raises(SdrxError) as e:
            call()
        assert e.value.code == _lib.SDRX_ESTATE
    on = Receiver.from_topology(topo, watch=True)  # the option on, nothing watched
    for rx in (off, on):
        rx.enable_kernel_timing(True)
    for iq in frames:
        off.process(iq)
        on.process(iq)
        for i in ids:
            assert np.array_equal(off.output(i), on.output(i)), i
    assert off.stats()["device_bytes"] == on.stats()["device_bytes"]
    assert _launches(off) == _launches(on)
    lv = on.watch(ids)
    assert not lv["watched"].any() and not lv["band_pwr"].any() and not lv["total_pwr"].any() and not lv["segments"].any()
    assert [(int(a), int(b)) for a, b in zip(lv["first_bin"], lv["n_bins"])] == [wr.band(topo.vfos[i]) for i in ids]
    assert (lv["frame"] == 1).all()
    on.set_watch([], [])  # n == 0 does nothing
    assert off.stats()["device_bytes"] == on.stats()["device_bytes"]
    with pytest.raises(SdrxError) as e:
        on.watch_psd(1)
    assert e.value.code == _lib.SDRX_EINVAL  # not watched
    on.set_watch([1, 2], [1, 1])
    assert on.stats()["device_bytes"] > off.stats()["device_bytes"]
    on.process(frames[0])
    good = on.watch(ids)
    assert list(good["watched"]) == [1, 1] + [0] * (len(ids) - 2)
    L = on.L
    for bad_ids, bad_on, n in (([1, 99], [0, 0], 2), ([1, 1], [0, 0], 2), ([0], [1], 1), ([1, 2], [0, 2], 2), ([1], [0], -1)):
        a, o = np.array(bad_ids, np.int32), np.array(bad_on, np.int32)
        assert L.sdrx_set_watch(on.h, a.ctypes.data, o.ctypes.data, n) == _lib.SDRX_EINVAL, (bad_ids, bad_on, n)
        on.process(frames[0])
        assert list(on.watch(ids)["watched"]) == list(good["watched"]), "a refused list changed the selection"
    on.submit(frames[1])
    with pytest.raises(SdrxError) as e:
        on.set_watch([1], [0])
    assert e.value.code == _lib.SDRX_ESTATE  # a submitted frame is undelivered
    on.wait()
    on.set_watch([1], [0])
    on.process(frames[1])
    assert list(on.watch([1, 2])["watched"]) == [0, 1]


@pytest.mark.parametrize("members", [2, 3])
def test_group_equals_single_context(members):
    topo = wr.watch_tree()
    ids = _leaves(topo)
    one = Receiver.from_topology(topo, watch=True)
    grp = Group.from_topology(topo, [0] * members, watch=1)
    one.set_watch(ids, [1] * len(ids))
    grp.set_watch(ids, [1] * len(ids))
    for f in range(2):
        iq = wr.tone_frame(topo, wr.tone_for(topo, 4), seed=f, start=f * topo.frame)
        one.process(iq)
        grp.process(iq)
        _same_records(grp.watch(ids), one.watch(ids), ("group", members, f))
        for i in (1, 5, 9):
            pg, fg = grp.watch_psd(i)
            po, fo = one.watch_psd(i)
            assert fg == fo == f and np.array_equal(_bits(pg), _bits(po)), (members, f, i)
