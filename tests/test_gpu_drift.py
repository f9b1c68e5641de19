"""Drift estimate on the device (sdrx_set_drift / sdrx_get_drift / sdrx_get_drift_profile and their group forms, k_watch_drift)
against the numpy model tests/drift_ref.py.

The profile is compared with the model's on the PSD THE DEVICE returns (sdrx_get_watch_psd, itself held bit for bit to the
watch's model by test_gpu_watch.py) within (N + 4) 2^-53 relative -- the bound include/sdrx.h derives; `shift` must be the
model's, on inputs whose runner-up lies at or below (1 - 1e-6) x the peak (asserted here on the device's PSD, and without a
GPU by test_drift_model.py); peak, left, right and zero are the device's own profile values, bit for bit."""
import functools

import numpy as np
import pytest

import drift_ref as dr
import lattice
import watch_ref as wr
from sdrreceiver_amd import _lib, drift
from sdrreceiver_amd.receiver import Group, Receiver, SdrxError

pytestmark = pytest.mark.gpu
N = dr.N


def _leaves(topo):
    return [i for i in range(len(topo.vfos)) if not topo.children(i)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _code(call):
    with pytest.raises(SdrxError) as e:
        call()
    return e.value.code


def check_record(rec, prof, frame, captured=0):
    """The record against the device's own profile: the first maximum in the defined order and the values beside it."""
    want = dr.record(prof)
    K = want["max_shift"]
    assert (rec["measured"], rec["captured"], rec["frame"], rec["max_shift"]) == (1, captured, frame, K), (rec, frame)
    assert rec["shift"] == want["shift"], (rec, want)
    for key in ("peak", "left", "right", "zero"):
        assert np.array_equal(_bits(np.float64(rec[key])), _bits(np.float64(want[key]))), (key, rec, want)


def check_source(rx, leaf, T, K, frame, shift=None, captured=0):
    """Profile and record of the source of `leaf` after `frame` against the model on the device's PSD with template T."""
    psd, f = rx.watch_psd(leaf)
    prof, fp = rx.drift_profile(leaf)
    assert f == fp == frame and prof.shape == (2 * K + 1,)
    model = dr.profile(T, psd, K)
    err = np.abs(prof - model)
    worst = float((err / np.where(model > 0, model, 1.0)).max())
    print(f"leaf {leaf} frame {frame}: worst relative difference {worst:.3e} (bound {dr.BOUND:.3e}), separation {dr.separation(model):.6f}")
    assert (err <= dr.BOUND * model).all(), (leaf, frame, worst)
    assert dr.separation(model) <= dr.SEPARATION, (leaf, frame, dr.separation(model))
    rec = rx.drift(leaf)
    check_record(rec, prof, frame, captured)
    assert rec["shift"] == dr.argmax(model)
    if shift is not None:
        assert rec["shift"] == shift, (leaf, frame, rec, shift)
    return psd, rec


# ---- indexing, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 7, 64, 1024])
def test_indexing_bit_for_bit(K):
    """A template that is 1.0 at bin i0 and 0 elsewhere: profile[s] = PSD[(i0 + s) mod N] exactly -- the wrap on both sides, and
    the shift blocks' remainders (16 shifts per workgroup: 2K + 1 = 3, 15, 129 = 8 x 16 + 1, 2049 = 128 x 16 + 1)."""
    topo = wr.watch_tree()
    rx = Receiver.from_topology(topo, watch=True)
    rx.set_watch([1], [1])
    for f, i0 in enumerate([0, 3, 8191, 4096]):
        T = np.zeros(N)
        T[i0] = 1.0
        rx.set_drift(1, T, K)
        rx.process(dr.wt_frame(topo, 0.0, seed=20 + f, start=f * topo.frame))
        psd, fp = rx.watch_psd(1)
        prof, fd = rx.drift_profile(1)
        assert fp == fd == f
        want = psd[(i0 + np.arange(-K, K + 1)) % N]
        assert np.array_equal(_bits(prof), _bits(want)), (K, i0, int((prof != want).sum()))
        check_record(rx.drift(1), prof, f)


# ---- profile and record against the model -------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [1, 0, 2])
def test_watch_tree_against_the_model(exact):
    """A source of 7 680 samples (zero-padded, one segment): template uploaded from frame 0's PSD, then +45 Hz = 12 bins and
    -26.25 Hz = -7 bins."""
    topo = wr.watch_tree()
    rx = Receiver.from_topology(topo, exact=exact, watch=True)
    ids = _leaves(topo)
    rx.set_watch(ids, [1] * len(ids))
    rx.process(dr.wt_frame(topo, 0.0, seed=5))
    T, _ = rx.watch_psd(1)
    rx.set_drift(9, T, dr.WT_K)  # (any watched leaf of the source names it)
    for f, (hz, seed) in enumerate(((0.0, 5), (dr.WT_DRIFT_HZ, 6), (-26.25, 7)), start=1):
        rx.process(dr.wt_frame(topo, hz, seed=seed))
        _, rec = check_source(rx, 1, T, dr.WT_K, f, shift=round(hz / 3.75))
        est = drift.estimate_hz(rec, topo.vfos[1].fs)
        assert abs(est - hz) <= 3.75, (hz, est)
        assert rx.drift(5) == rec  # the record is the source's, whichever leaf asks


@pytest.mark.parametrize("exact", [1, 0, 2])
def test_sources_above_n_against_the_model(exact):
    """drift_tree(24 832): the parent's stream has S = 3 segments, the raw frame (198 656 samples) S = 16; both sources at once."""
    topo = dr.drift_tree(24832)
    rx = Receiver.from_topology(topo, exact=exact, watch=True)
    leaves = [dr.DT_PARENT_LEAF, dr.DT_RAW_LEAF]
    rx.set_watch(leaves, [1, 1])
    rx.process(dr.raw_frame(topo, 0.0, seed=1))
    T = {i: rx.watch_psd(i)[0] for i in leaves}
    for i in leaves:
        rx.set_drift(i, T[i], dr.RAW_K)
    rx.process(dr.raw_frame(topo, dr.RAW_DRIFT_BINS * topo.fs / N, seed=2))
    assert rx.watch(leaves)["segments"].tolist() == [3, 16]
    check_source(rx, dr.DT_PARENT_LEAF, T[dr.DT_PARENT_LEAF], dr.RAW_K, 1, shift=8 * dr.RAW_DRIFT_BINS)
    check_source(rx, dr.DT_RAW_LEAF, T[dr.DT_RAW_LEAF], dr.RAW_K, 1, shift=dr.RAW_DRIFT_BINS)


@pytest.mark.parametrize("kind", ["f32", "u8", "u8_dc", "device"])
def test_raw_frame_kinds(kind):
    """The raw frame as source: host floats, dongle bytes, the tile-layout frame the DC-bias removal leaves, and a caller's
    device frame (the raw source's PSD does not depend on the arithmetic)."""
    topo = dr.drift_tree(8704)
    rx = Receiver.from_topology(topo, watch=True)
    leaf = dr.DT_RAW_LEAF
    rx.set_watch([leaf], [1])
    keep = []

    def run(iq):
        if kind == "device":
            import torch
            dev = torch.from_numpy(iq).cuda()
            torch.cuda.synchronize()
            keep.append(dev)
            rx.process_device(dev.data_ptr(), topo.frame)
            rx.fetch()
        elif kind == "f32":
            rx.process(iq)
        else:
            rx.process_u8((iq + 127).astype(np.uint8), correct_dc=kind == "u8_dc")

    run(dr.raw_frame(topo, 0.0, seed=1))
    T, _ = rx.watch_psd(leaf)
    rx.set_drift(leaf, T, dr.RAW_K)
    run(dr.raw_frame(topo, dr.RAW_DRIFT_BINS * topo.fs / N, seed=2))
    check_source(rx, leaf, T, dr.RAW_K, 1, shift=dr.RAW_DRIFT_BINS)


# ---- capture ------------------------------------------------------------------------------------------------------------
def test_capture():
    topo = wr.watch_tree()
    rx = Receiver.from_topology(topo, watch=True)
    rx.set_watch([1, 2], [1, 1])
    K = dr.WT_K
    rx.set_drift(1, None, K)
    rx.process(dr.wt_frame(topo, 0.0, seed=5))
    T, _ = rx.watch_psd(1)
    _, rec = check_source(rx, 1, T, K, 0, shift=0, captured=1)  # the frame correlates with itself
    energy = dr.profile(T, T, 0)[0]
    assert abs(rec["peak"] - energy) <= dr.BOUND * energy and rec["zero"] == rec["peak"]
    for f, (hz, seed) in enumerate(((dr.WT_DRIFT_HZ, 6), (-26.25, 7)), start=1):  # later frames: the captured template, no new capture
        rx.process(dr.wt_frame(topo, hz, seed=seed))
        check_source(rx, 1, T, K, f, shift=round(hz / 3.75), captured=0)
    rx.set_drift(2, None, 8)  # a second capture replaces the template, from the next measured frame
    rx.process(dr.wt_frame(topo, dr.WT_DRIFT_HZ, seed=8))
    T2, _ = rx.watch_psd(2)
    assert not np.array_equal(T, T2)
    check_source(rx, 1, T2, 8, 3, shift=0, captured=1)
    rx.process(dr.wt_frame(topo, dr.WT_DRIFT_HZ + 3 * 3.75, seed=9))
    check_source(rx, 1, T2, 8, 4, shift=3)
    rx.set_drift(1, T, K)  # an upload calls a pending capture off
    rx.set_drift(1, None, K)
    rx.set_drift(1, T, K)
    rx.process(dr.wt_frame(topo, dr.WT_DRIFT_HZ, seed=6))
    check_source(rx, 1, T, K, 5, shift=12, captured=0)


# ---- frame bookkeeping --------------------------------------------------------------------------------------------------
BK_K = 16


def _one_leaf_per_source(topo):
    out = {}
    for i in _leaves(topo):
        out.setdefault(topo.vfos[i].parent, i)
    return [out[p] for p in sorted(out)]


def _bk_setup(rx, topo):
    ids = _leaves(topo)
    rx.set_watch(ids, [1] * len(ids))
    picks = _one_leaf_per_source(topo)
    for i in picks:
        rx.set_drift(i, None, BK_K)
    return picks


@functools.lru_cache(maxsize=None)
def _inner_reference():
    """lattice's "inner" tree (leaves on levels 1 and 2, so sources on two levels), every source with a captured template, frame
    by frame through sdrx_process: the records per frame, each checked against the model.  Shared; nobody writes into it."""
    topo = lattice.trees()["inner"]
    frames = list(lattice.frames("inner"))[:4]
    rx = Receiver.from_topology(topo, watch=True)
    picks = _bk_setup(rx, topo)
    assert len({lattice.level(topo, i) for i in picks}) >= 2
    recs, T = [], {}
    for f, iq in enumerate(frames):
        rx.process(iq)
        row = []
        for i in picks:
            if f == 0:
                T[i] = rx.watch_psd(i)[0]
            prof, _ = rx.drift_profile(i)
            model = dr.profile(T[i], rx.watch_psd(i)[0], BK_K)
            assert (np.abs(prof - model) <= dr.BOUND * model).all(), (f, i)
            rec = rx.drift(i)
            check_record(rec, prof, f, captured=int(f == 0))
            row.append(rec)
        recs.append(row)
    return topo, frames, picks, recs


def test_frame_bookkeeping_submit():
    """Two frames in flight: the record delivered with frame f carries f and is frame f's, readable while f + 1 is in flight."""
    topo, frames, picks, recs = _inner_reference()
    rx = Receiver.from_topology(topo, watch=True)
    _bk_setup(rx, topo)
    delivered = 0
    for iq in frames:
        rx.submit(iq)
        if rx.in_flight() == 2:
            rx.wait()
            assert [rx.drift(i) for i in picks] == recs[delivered], ("submit", delivered)
            assert _code(lambda: rx.drift_profile(picks[0])) == _lib.SDRX_ESTATE
            assert _code(lambda: rx.set_drift(picks[0], None, 4)) == _lib.SDRX_ESTATE
            delivered += 1
    while rx.in_flight():
        rx.wait()
        assert [rx.drift(i) for i in picks] == recs[delivered], ("submit", delivered)
        delivered += 1
    assert delivered == len(frames)


@pytest.mark.parametrize("opts", [dict(), dict(frame_pipeline=False), dict(pipeline=True), dict(tail_in_levels=False)])
def test_frame_bookkeeping_device_frames(opts):
    """sdrx_process_device queues frames inside the software pipeline (level l holds frame k - l): three frames queued, one
    fetch, then a fourth -- each source's record carries the frame its stream held."""
    import torch
    topo, frames, picks, recs = _inner_reference()
    rx = Receiver.from_topology(topo, watch=True, **opts)
    _bk_setup(rx, topo)
    dev = [torch.from_numpy(np.array(iq)).cuda() for iq in frames]
    torch.cuda.synchronize()
    for f in range(3):
        rx.process_device(dev[f].data_ptr(), topo.frame)
    rx.fetch()
    assert [rx.drift(i) for i in picks] == recs[2], ("device", opts, 2)
    rx.process_device(dev[3].data_ptr(), topo.frame)
    rx.fetch()
    assert [rx.drift(i) for i in picks] == recs[3], ("device", opts, 3)


# ---- template survival and measured = 0 ----------------------------------------------------------------------------------
def test_template_survives_and_unmeasured_frames():
    topo = dr.drift_tree(8704)
    rx = Receiver.from_topology(topo, watch=True, park=True)
    leaf, other, raw_leaf = dr.DT_PARENT_LEAF, 2, dr.DT_RAW_LEAF
    rx.set_watch([leaf], [1])
    rx.set_drift(leaf, None, dr.RAW_K)
    hz = dr.RAW_DRIFT_BINS * topo.fs / N
    rx.process(dr.raw_frame(topo, 0.0, seed=1))
    T, _ = rx.watch_psd(leaf)
    check_source(rx, leaf, T, dr.RAW_K, 0, shift=0, captured=1)
    bytes_before = rx.stats()["device_bytes"]
    # a retune of the leaf, a park and an unpark: the source's PSD does not change, nor does the template
    rx.set_mixer_freqs([leaf], [topo.vfos[leaf].mixer_freq + 500.0])
    rx.set_active([leaf], [0])
    rx.process(dr.raw_frame(topo, hz, seed=2))
    check_source(rx, leaf, T, dr.RAW_K, 1, shift=8 * dr.RAW_DRIFT_BINS)
    rx.set_active([leaf], [1])
    # the watched set grows by a leaf of ANOTHER source, which comes first in the watch's buffers: they move and are cleared
    rx.set_watch([raw_leaf, other], [1, 1])
    assert rx.stats()["device_bytes"] > bytes_before
    rx.process(dr.raw_frame(topo, hz, seed=3))
    check_source(rx, other, T, dr.RAW_K, 2, shift=8 * dr.RAW_DRIFT_BINS)
    assert rx.drift(raw_leaf) == dict(frame=2, peak=0.0, left=0.0, right=0.0, zero=0.0, shift=0, max_shift=0, measured=0, captured=0)
    # no leaf of the source watched: no record (and no launch); watched again: the template is still there
    rx.set_watch([leaf, other], [0, 0])
    rx.process(dr.raw_frame(topo, hz, seed=4))
    assert rx.drift(leaf) == dict(frame=3, peak=0.0, left=0.0, right=0.0, zero=0.0, shift=0, max_shift=0, measured=0, captured=0)
    rx.set_watch([other], [1])
    assert rx.drift(other)["measured"] == 0  # (still frame 3)
    rx.process(dr.raw_frame(topo, hz, seed=5))
    check_source(rx, other, T, dr.RAW_K, 4, shift=8 * dr.RAW_DRIFT_BINS)
    # off and on again with an upload
    rx.set_drift(other, None, 0)
    rx.process(dr.raw_frame(topo, hz, seed=6))
    assert rx.drift(other)["measured"] == 0 and rx.drift(other)["frame"] == 5
    assert _code(lambda: rx.drift_profile(other)) == _lib.SDRX_EINVAL
    rx.set_drift(other, T, 5)
    assert _code(lambda: rx.drift_profile(other)) == _lib.SDRX_ESTATE  # no frame under this setting yet
    rx.process(dr.raw_frame(topo, 0.0, seed=7))
    check_source(rx, other, T, 5, 6, shift=0)


# ---- off state and errors ------------------------------------------------------------------------------------------------
def _launches(rx):
    return {k: v["launches"] for k, v in rx.kernel_times().items()}


def test_off_state_and_errors():
    topo = wr.watch_tree()
    ids = _leaves(topo)
    frames = [dr.wt_frame(topo, 0.0, seed=f) for f in range(2)]
    off = Receiver.from_topology(topo)
    for call in (lambda: off.set_drift(1, None, 4), lambda: off.drift(1), lambda: off.drift_profile(1)):
        assert _code(call) == _lib.SDRX_ESTATE  # option "watch" is off
    a = Receiver.from_topology(topo, watch=True, meter=True)  # watched, drift never set
    b = Receiver.from_topology(topo, watch=True, meter=True)  # its twin, on which the drift calls are made
    for rx in (a, b):
        rx.set_watch([1, 2], [1, 1])
        rx.enable_kernel_timing(True)
    assert _code(lambda: b.drift(1)) == _lib.SDRX_ESTATE  # no frame delivered yet
    b.set_drift(1, None, 0)  # switching off what is off: nothing happens
    for iq in frames:
        a.process(iq)
        b.process(iq)
    assert a.stats()["device_bytes"] == b.stats()["device_bytes"]
    assert _launches(a) == _launches(b)
    assert b.drift(1) == dict(frame=1, peak=0.0, left=0.0, right=0.0, zero=0.0, shift=0, max_shift=0, measured=0, captured=0)
    good = np.ones(N)
    L = b.L
    bad_nan, bad_neg, bad_inf = good.copy(), good.copy(), good.copy()
    bad_nan[77], bad_neg[8191], bad_inf[0] = np.nan, -1e-300, np.inf
    for leaf, templ, K in ((3, good, 4), (1, good, -1), (1, good, 1025), (1, None, 1025), (1, bad_nan, 4), (1, bad_neg, 4),
                           (1, bad_inf, 4), (0, good, 4), (99, good, 4)):
        rc = L.sdrx_set_drift(b.h, leaf, None if templ is None else templ.ctypes.data, K)
        assert rc == _lib.SDRX_EINVAL, (leaf, K, rc)
    assert _code(lambda: b.drift_profile(3)) == _lib.SDRX_EINVAL  # not watched
    assert _code(lambda: b.drift_profile(1)) == _lib.SDRX_EINVAL  # no drift on its source
    assert a.stats()["device_bytes"] == b.stats()["device_bytes"], "a refused call allocated something"
    b.set_drift(1, np.zeros(N), 1024)  # an all-zero template
    assert b.stats()["device_bytes"] > a.stats()["device_bytes"]
    assert _code(lambda: b.drift_profile(1)) == _lib.SDRX_ESTATE  # no frame measured yet
    for iq in frames:
        a.process(iq)
        b.process(iq)
        for i in ids:
            assert np.array_equal(a.output(i), b.output(i)), i
        ma, mb = a.meters(ids), b.meters(ids)
        wa, wb = a.watch(ids), b.watch(ids)
        for key in ma:
            assert np.array_equal(_bits(ma[key]), _bits(mb[key])), ("meter", key)
        for key in wa:
            assert np.array_equal(_bits(wa[key]), _bits(wb[key])), ("watch", key)
    assert _launches(a) == _launches(b)  # (k_watch_drift is not bracketed: SDRX_NKERNELS kinds, as before)
    assert b.drift(1) == dict(frame=3, peak=0.0, left=0.0, right=0.0, zero=0.0, shift=0, max_shift=1024, measured=1, captured=0)
    prof, f = b.drift_profile(2)
    assert f == 3 and prof.shape == (2049,) and not prof.any()
    b.submit(frames[0])
    assert _code(lambda: b.set_drift(1, None, 4)) == _lib.SDRX_ESTATE  # a submitted frame is undelivered
    assert _code(lambda: b.drift_profile(1)) == _lib.SDRX_ESTATE
    assert b.drift(1)["frame"] == 3  # the delivered frame's record, while the next is in flight
    b.wait()
    assert b.drift(1)["frame"] == 4


# ---- groups ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [2, 3])
def test_group_equals_single_context(members):
    topo = wr.watch_tree()
    ids = _leaves(topo)
    one = Receiver.from_topology(topo, watch=True)
    grp = Group.from_topology(topo, [0] * members, watch=1)
    picks = (1, 5, 9)  # (on a group every member that holds one of them keeps its own template of the source)
    for rx in (one, grp):
        rx.set_watch(ids, [1] * len(ids))
        for i in picks:
            rx.set_drift(i, None, dr.WT_K)
    for f, (hz, seed) in enumerate(((0.0, 5), (dr.WT_DRIFT_HZ, 6))):
        iq = dr.wt_frame(topo, hz, seed=seed)
        one.process(iq)
        grp.process(iq)
        for i in picks:
            assert grp.drift(i) == one.drift(i), (members, f, i)
            pg, fg = grp.drift_profile(i)
            po, fo = one.drift_profile(i)
            assert fg == fo == f and np.array_equal(_bits(pg), _bits(po)), (members, f, i)
        assert one.drift(1)["shift"] == round(hz / 3.75) and one.drift(1)["captured"] == int(f == 0)
    assert _code(lambda: grp.set_drift(99, None, 4)) == _lib.SDRX_EINVAL
