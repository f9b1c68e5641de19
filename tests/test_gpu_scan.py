"""Band scan on the device (sdrx_set_scan / sdrx_get_scan / sdrx_get_scan_hits / sdrx_get_scan_cells and their group forms,
k_watch_scan) against the numpy model tests/scan_ref.py.

Every record, hit list and cell array is compared BIT FOR BIT with the model evaluated on the PSDs THE DEVICE returned
(sdrx_get_watch_psd, itself held bit for bit to the watch's model by test_gpu_watch.py) for the integrated frames.  No
tolerance appears anywhere."""
import dataclasses
import functools

import numpy as np
import pytest

import drift_ref as dr
import lattice
import retune_ref as rr
import scan_ref as sc
import watch_ref as wr
from sdrreceiver_amd import _lib, scan
from sdrreceiver_amd.receiver import Group, Receiver, SdrxError

pytestmark = pytest.mark.gpu
N = sc.N
UNMEASURED = dict(frame=0, floor=0.0, thr=0.0, n_hits=0, n_stored=0, n_hot=0, integrated=0, frames=0, cell_bins=0, measured=0, complete=0)


def _leaves(topo):
    return [i for i in range(len(topo.vfos)) if not topo.children(i)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _code(call):
    with pytest.raises(SdrxError) as e:
        call()
    return e.value.code


def _same_record(got, want):
    assert set(got) == set(want) == set(sc.RECORD_KEYS)
    for k in sc.RECORD_KEYS:
        if k in ("floor", "thr"):
            assert np.array_equal(_bits(np.float64(got[k])), _bits(np.float64(want[k]))), (k, got, want)
        else:
            assert got[k] == want[k], (k, got, want)


def _same_hits(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert {k: g[k] for k in ("first_cell", "n_cells", "peak_cell")} == {k: w[k] for k in ("first_cell", "n_cells", "peak_cell")}, (g, w)
        assert np.array_equal(_bits(np.float64(g["peak_pwr"])), _bits(np.float64(w["peak_pwr"]))), (g, w)


def check_evaluation(rx, leaf, it, frame):
    """Record, hits and cells of the source of `leaf` after `frame` -- on which the model `it` (an Integrator fed the device's PSDs)
    completed an evaluation."""
    assert it.eval_frame == frame
    hits, fh = rx.scan_hits(leaf)
    cells, fc = rx.scan_cells(leaf)
    assert fh == fc == frame
    _same_hits(hits, it.hits)
    assert cells.shape == it.cells.shape and np.array_equal(_bits(cells), _bits(it.cells)), int((cells != it.cells).sum())


def run_scan(rx, leaf, c, frames, feed=None, first_frame=0):
    """set_scan(c) on the source of `leaf`, then `frames` one after the other: every frame's record against the model on the
    device's PSD, and every completed evaluation.  Returns the model."""
    feed = feed or rx.process
    rx.set_scan(leaf, **c)
    it = sc.Integrator(c)
    for f, iq in enumerate(frames, start=first_frame):
        feed(iq)
        psd, fp = rx.watch_psd(leaf)
        assert fp == f
        want = it.step(psd, f)
        _same_record(rx.scan(leaf), want)
        if want["complete"]:
            check_evaluation(rx, leaf, it, f)
    return it


# ---- cells, floor, threshold and hits ---------------------------------------------------------------------------------------
RATIO = {1: 4 * 256, 4: 16 * 256, 256: 2 * 256}


@pytest.mark.parametrize("exact", [1, 0, 2])
def test_watch_tree_against_the_model(exact):
    """w x q x M on the main's stream of watch_tree() (7 680 samples, zero-padded): C = 8192, 2048 and 32 cells -- sixteen cells, four
    cells and fewer cells than threads per thread."""
    topo = wr.watch_tree()
    frames = sc.wt_frames(topo)
    rx = Receiver.from_topology(topo, exact=exact, watch=True)
    rx.set_watch([sc.WT_LEAF, 9], [1, 1])
    f = 0
    for w in (1, 4, 256):
        for q in (0, 500, 1000):
            for M in (1, 3):
                it = run_scan(rx, 9 if w == 4 else sc.WT_LEAF, sc.cfg(w, M, q, RATIO[w]), frames[:M], first_frame=f)
                f += M
                assert it.eval_frame == f - 1
                if q == 1000:
                    assert it.hits == []
                if (w, q, exact) == (4, 500, 1):  # (the exact arithmetic is the oracle's: the condition test_scan_model.py checks)
                    assert len(it.hits) == 8 and all(a["first_cell"] <= t < a["first_cell"] + a["n_cells"]
                                                     for a, t in zip(it.hits, sorted(sc.wt_tone_cells(topo, 4))))
    rx.close()


def test_min_cells_truncation_and_zeros():
    topo = wr.watch_tree()
    frames = sc.wt_frames(topo)
    rx = Receiver.from_topology(topo, watch=True)
    rx.set_watch([sc.WT_LEAF], [1])
    one = run_scan(rx, sc.WT_LEAF, sc.WT_NOISE, frames[:1])
    three = run_scan(rx, sc.WT_LEAF, dict(sc.WT_NOISE, min_cells=3), frames[:1], first_frame=1)
    assert 100 < len(one.hits) < 512 and 0 < len(three.hits) < len(one.hits)
    assert all(h["n_cells"] >= 3 for h in three.hits) and any(h["n_cells"] < 3 for h in one.hits)
    run_scan(rx, sc.WT_LEAF, sc.WT_TRUNCATED, frames[:1], first_frame=2)
    rec = rx.scan(sc.WT_LEAF)
    assert rec["n_hits"] > 512 and rec["n_stored"] == 512
    few, _ = rx.scan_hits(sc.WT_LEAF, max_hits=10)
    all_, _ = rx.scan_hits(sc.WT_LEAF)
    assert len(all_) == 512 and few == all_[:10] and rx.scan_hits(sc.WT_LEAF, max_hits=0)[0] == []
    rx.close()
    rx = Receiver.from_topology(topo, watch=True)  # a fresh tree: with frames of zeros from the start its streams are zeros
    rx.set_watch([sc.WT_LEAF], [1])
    for f, w in enumerate((1, 4, 256)):  # every cell ties, floor 0, no hit
        it = run_scan(rx, sc.WT_LEAF, sc.cfg(w, 1, 500, 16 * 256), [np.zeros(2 * topo.frame, np.float32)], first_frame=f)
        rec = rx.scan(sc.WT_LEAF)
        assert (rec["floor"], rec["thr"], rec["n_hits"], rec["n_hot"]) == (0.0, 0.0, 0, 0) and not it.cells.any()
    rx.close()


# ---- the raw frame: a tone at -fs/2, and the ways a raw frame arrives -----------------------------------------------------------
def _two_hits_at_the_edges(hits, C):
    assert len(hits) == 2 and hits[0]["first_cell"] == 0 and hits[1]["first_cell"] + hits[1]["n_cells"] == C, hits


@pytest.mark.parametrize("kind", ["f32", "u8", "u8_dc", "device"])
def test_raw_frame_kinds_and_the_edge_tone(kind):
    """One tone at -fs/2 of the raw frame: its skirt lands in cell 0 and in cell C - 1 and gives two hits, never one."""
    topo = dr.drift_tree(8704)
    rx = Receiver.from_topology(topo, watch=True)
    leaf = dr.DT_RAW_LEAF
    rx.set_watch([leaf], [1])
    keep = []

    def feed(iq):
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

    iq = sc.edge_tone_frame(topo)
    for f, (w, M) in enumerate(((4, 1), (1, 1))):
        it = run_scan(rx, leaf, sc.cfg(w, M, 500, 64 * 256), [iq], feed=feed, first_frame=f)
        _two_hits_at_the_edges(it.hits, N // w)
    rx.close()


@pytest.mark.parametrize("exact", [1, 0])
def test_sources_above_n(exact):
    """drift_tree(24 832): the parent's stream has S = 3 segments, the raw frame S = 16; both sources scanned in one launch, with
    different settings."""
    topo = dr.drift_tree(24832)
    rx = Receiver.from_topology(topo, exact=exact, watch=True)
    a, b = dr.DT_PARENT_LEAF, dr.DT_RAW_LEAF
    rx.set_watch([a, b], [1, 1])
    ca, cb = sc.cfg(16, 2, 250, 3 * 256, 2), sc.cfg(4, 1, 500, 64 * 256)
    rx.set_scan(a, **ca)
    rx.set_scan(b, **cb)
    ia, ib = sc.Integrator(ca), sc.Integrator(cb)
    for f, iq in enumerate((sc.edge_tone_frame(topo), dr.raw_frame(topo, 0.0, seed=1))):
        rx.process(iq)
        for leaf, it in ((a, ia), (b, ib)):
            want = it.step(rx.watch_psd(leaf)[0], f)
            _same_record(rx.scan(leaf), want)
            if want["complete"]:
                check_evaluation(rx, leaf, it, f)
        if f == 0:
            _two_hits_at_the_edges(ib.hits, N // 4)
    assert rx.watch([a, b])["segments"].tolist() == [3, 16] and ia.eval_frame == 1
    rx.close()


# ---- integration ------------------------------------------------------------------------------------------------------------
def test_integration_over_frames():
    topo = wr.watch_tree()
    frames = sc.wt_frames(topo)
    rx = Receiver.from_topology(topo, watch=True)
    leaf = sc.WT_LEAF
    rx.set_watch([leaf], [1])
    c = sc.cfg(4, 3, 500, 16 * 256)
    rx.set_scan(leaf, **c)
    it = sc.Integrator(c)
    assert _code(lambda: rx.scan_hits(leaf)) == _lib.SDRX_ESTATE  # no evaluation has completed yet
    seen = []

    def frame(f, iq, watched=True):
        rx.process(iq)
        want = it.step(rx.watch_psd(leaf)[0] if watched else None, f)
        got = rx.scan(5)  # (any leaf of the source, watched or not)
        _same_record(got, want)
        seen.append((got["integrated"], got["measured"], got["complete"]))

    frame(0, frames[0])
    frame(1, frames[1])
    assert _code(lambda: rx.scan_hits(leaf)) == _lib.SDRX_ESTATE
    rx.set_watch([leaf], [0])  # a frame with the watch off: no observation
    frame(2, frames[2], watched=False)
    rx.set_watch([leaf], [1])
    frame(3, frames[2])
    assert seen == [(1, 1, 0), (2, 1, 0), (0, 0, 0), (3, 1, 1)]
    check_evaluation(rx, leaf, it, 3)
    first = (rx.scan_hits(leaf), rx.scan_cells(leaf)[0])
    frame(4, frames[0])  # the next round: the last completed evaluation is still served, with its frame
    frame(5, frames[1])
    assert seen[4:] == [(1, 1, 0), (2, 1, 0)]
    again = (rx.scan_hits(leaf), rx.scan_cells(leaf)[0])
    assert again[0] == first[0] and again[0][1] == 3 and np.array_equal(_bits(again[1]), _bits(first[1]))
    rx.set_scan(leaf, **c)  # in mid-integration: restarts it, and the evaluation before is not this setting's
    it = sc.Integrator(c)
    assert _code(lambda: rx.scan_hits(leaf)) == _lib.SDRX_ESTATE
    rx.set_mixer_freqs([leaf], [topo.vfos[leaf].mixer_freq + 100.0])  # a retune of a leaf restarts nothing
    frame(6, frames[2])
    frame(7, frames[0])
    frame(8, frames[1])
    assert seen[6:] == [(1, 1, 0), (2, 1, 0), (3, 1, 1)]
    check_evaluation(rx, leaf, it, 8)
    rx.close()


# ---- launch forms -------------------------------------------------------------------------------------------------------------
BK = sc.cfg(4, 2, 500, 3 * 256)


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
        rx.set_scan(i, **BK)
    return picks


@functools.lru_cache(maxsize=None)
def _inner_reference():
    """lattice's "inner" tree (sources on two levels), every source scanned with M = 2, frame by frame through sdrx_process: the
    records per frame and the evaluations, each checked against the model.  Shared; nobody writes into it."""
    topo = lattice.trees()["inner"]
    frames = list(lattice.frames("inner"))[:4]
    rx = Receiver.from_topology(topo, watch=True)
    picks = _bk_setup(rx, topo)
    assert len({lattice.level(topo, i) for i in picks}) >= 2
    its = {i: sc.Integrator(BK) for i in picks}
    recs, evals = [], []
    for f, iq in enumerate(frames):
        rx.process(iq)
        row = []
        for i in picks:
            want = its[i].step(rx.watch_psd(i)[0], f)
            _same_record(rx.scan(i), want)
            if want["complete"]:
                check_evaluation(rx, i, its[i], f)
            row.append(rx.scan(i))
        recs.append(row)
        evals.append([(rx.scan_hits(i), rx.scan_cells(i)[0].tobytes()) for i in picks] if f % 2 == 1 else None)
    rx.close()
    return topo, frames, picks, recs, evals


def _evaluations(rx, picks):
    return [(rx.scan_hits(i), rx.scan_cells(i)[0].tobytes()) for i in picks]


def test_submit_wait_pipelined():
    """Two frames in flight: the record delivered with frame f is frame f's, readable while f + 1 is in flight."""
    topo, frames, picks, recs, evals = _inner_reference()
    rx = Receiver.from_topology(topo, watch=True)
    _bk_setup(rx, topo)
    delivered = 0
    for iq in frames:
        rx.submit(iq)
        if rx.in_flight() == 2:
            rx.wait()
            assert [rx.scan(i) for i in picks] == recs[delivered], ("submit", delivered)
            assert _code(lambda: rx.scan_hits(picks[0])) == _lib.SDRX_ESTATE
            assert _code(lambda: rx.scan_cells(picks[0])) == _lib.SDRX_ESTATE
            assert _code(lambda: rx.set_scan(picks[0], **BK)) == _lib.SDRX_ESTATE
            delivered += 1
    while rx.in_flight():
        rx.wait()
        assert [rx.scan(i) for i in picks] == recs[delivered], ("submit", delivered)
        delivered += 1
    assert delivered == len(frames) and _evaluations(rx, picks) == evals[3]
    rx.close()


@pytest.mark.parametrize("opts", [dict(), dict(frame_pipeline=False), dict(pipeline=True)])
def test_device_frames_queued_back_to_back(opts):
    """sdrx_process_device queues frames inside the software pipeline (level l holds frame k - l): three frames queued, one
    fetch, then a fourth -- each source's record carries the frame its stream held."""
    import torch
    topo, frames, picks, recs, evals = _inner_reference()
    rx = Receiver.from_topology(topo, watch=True, **opts)
    _bk_setup(rx, topo)
    dev = [torch.from_numpy(np.array(iq)).cuda() for iq in frames]
    torch.cuda.synchronize()
    for f in range(3):
        rx.process_device(dev[f].data_ptr(), topo.frame)
    rx.fetch()
    assert [rx.scan(i) for i in picks] == recs[2], ("device", opts, 2)
    assert [r["frame"] for r in recs[2]] == [2] * len(picks)
    assert _evaluations(rx, picks) == evals[1]
    rx.process_device(dev[3].data_ptr(), topo.frame)
    rx.fetch()
    assert [rx.scan(i) for i in picks] == recs[3], ("device", opts, 3)
    assert _evaluations(rx, picks) == evals[3]
    rx.close()


def test_group_of_two_members_on_one_device():
    topo = wr.watch_tree()
    ids = _leaves(topo)
    one = Receiver.from_topology(topo, watch=True)
    grp = Group.from_topology(topo, [0, 0], watch=1)
    picks = (1, 5, 9)  # (every member that holds one of them keeps its own scan of the source)
    c = sc.cfg(4, 2, 500, 16 * 256)
    for rx in (one, grp):
        rx.set_watch(ids, [1] * len(ids))
        for i in picks:
            rx.set_scan(i, **c)
    for f, iq in enumerate(sc.wt_frames(topo)[:2]):
        one.process(iq)
        grp.process(iq)
        for i in picks:
            assert grp.scan(i) == one.scan(i), (f, i)
    assert one.scan(1)["complete"] == 1 and one.scan(1)["n_hits"] >= 8
    for i in picks:
        assert grp.scan_hits(i) == one.scan_hits(i) and grp.scan_hits(i)[1] == 1
        assert grp.scan_cells(i)[0].tobytes() == one.scan_cells(i)[0].tobytes()
    assert _code(lambda: grp.set_scan(99, **c)) == _lib.SDRX_EINVAL
    grp.submit(sc.wt_frames(topo)[2])
    assert _code(lambda: grp.scan_hits(1)) == _lib.SDRX_ESTATE and _code(lambda: grp.set_scan(1, **c)) == _lib.SDRX_ESTATE
    assert grp.scan(1)["frame"] == 1
    grp.wait()
    assert grp.scan(1)["frame"] == 2
    grp.close()
    one.close()


# ---- scan and drift together ---------------------------------------------------------------------------------------------------
def test_scan_and_drift_on_one_source():
    topo = wr.watch_tree()
    frames = sc.wt_frames(topo)
    c = sc.cfg(4, 2, 500, 16 * 256)
    rxs = {k: Receiver.from_topology(topo, watch=True) for k in ("scan", "drift", "both")}
    for k, rx in rxs.items():
        rx.set_watch([1], [1])
        if k != "drift":
            rx.set_scan(1, **c)
        if k != "scan":
            rx.set_drift(1, None, 64)
    for iq in frames:
        for rx in rxs.values():
            rx.process(iq)
        assert rxs["both"].scan(1) == rxs["scan"].scan(1) and rxs["both"].scan(1)["measured"] == 1
        assert rxs["both"].drift(1) == rxs["drift"].drift(1) and rxs["both"].drift(1)["measured"] == 1
        assert rxs["both"].drift_profile(1)[0].tobytes() == rxs["drift"].drift_profile(1)[0].tobytes()
    assert rxs["both"].scan_hits(1) == rxs["scan"].scan_hits(1) and rxs["both"].scan_hits(1)[1] == 1
    assert rxs["both"].scan_cells(1)[0].tobytes() == rxs["scan"].scan_cells(1)[0].tobytes()
    for rx in rxs.values():
        rx.close()


# ---- off means off, and the errors -----------------------------------------------------------------------------------------------
def _launches(rx):
    return {k: v["launches"] for k, v in rx.kernel_times().items()}


def _same_payloads(a, b, ids):
    for i in ids:
        assert np.array_equal(a.output(i), b.output(i)), i
    ma, mb = a.meters(ids), b.meters(ids)
    wa, wb = a.watch(ids), b.watch(ids)
    for key in ma:
        assert np.array_equal(_bits(ma[key]), _bits(mb[key])), ("meter", key)
    for key in wa:
        assert np.array_equal(_bits(wa[key]), _bits(wb[key])), ("watch", key)


def test_off_means_off():
    topo = wr.watch_tree()
    ids = _leaves(topo)
    frames = sc.wt_frames(topo)
    a = Receiver.from_topology(topo, watch=True, meter=True)  # watched, the scan never set
    b = Receiver.from_topology(topo, watch=True, meter=True)  # its twin, on which the scan calls are made
    for rx in (a, b):
        rx.set_watch([1, 2], [1, 1])
        rx.enable_kernel_timing(True)
    b.set_scan(1, cell_bins=0)  # switching off what is off: nothing happens
    b.L.sdrx_set_scan(b.h, 1, None)
    for iq in frames[:2]:
        a.process(iq)
        b.process(iq)
        _same_payloads(a, b, ids)
    assert a.stats()["device_bytes"] == b.stats()["device_bytes"]
    assert _launches(a) == _launches(b)
    assert b.scan(1) == dict(UNMEASURED, frame=1)
    b.set_scan(1, **sc.WT_CARRIERS)
    assert b.stats()["device_bytes"] > a.stats()["device_bytes"]
    for iq in frames[:2]:
        a.process(iq)
        b.process(iq)
        _same_payloads(a, b, ids)  # the payloads with the scan on are those with it off
    assert _launches(a) == _launches(b)  # (k_watch_scan is not bracketed: SDRX_NKERNELS kinds, as before)
    assert b.scan(1)["measured"] == 1 and b.scan(1)["complete"] == 1 and b.scan(1)["frame"] == 3
    bytes_on = b.stats()["device_bytes"]
    b.set_scan(1, cell_bins=0)
    assert b.scan(1)["measured"] == 1  # (still frame 3, which ran with the scan on)
    assert _code(lambda: b.scan_hits(1)) == _lib.SDRX_EINVAL and _code(lambda: b.scan_cells(1)) == _lib.SDRX_EINVAL
    a.process(frames[2])
    b.process(frames[2])
    _same_payloads(a, b, ids)
    assert b.scan(1) == dict(UNMEASURED, frame=4) and b.stats()["device_bytes"] == bytes_on  # the state stays allocated
    a.close()
    b.close()


def test_errors_in_the_one_check_order():
    topo = wr.watch_tree()
    good = _lib.ScanCfgC(4, 3, 500, 16 * 256, 1)
    out, n, f = _lib.ScanLevelC(), _lib.C.c_int(), _lib.C.c_int64()
    hits = (_lib.ScanHitC * 4)()
    off = Receiver.from_topology(topo)
    L = off.L
    byref = _lib.C.byref
    for rc in (L.sdrx_set_scan(off.h, 1, byref(good)), L.sdrx_get_scan(off.h, 1, byref(out)), L.sdrx_get_scan_hits(off.h, 1, hits, 4, byref(n), byref(f)),
               L.sdrx_get_scan_cells(off.h, 1, None, byref(f))):
        assert rc == _lib.SDRX_ESTATE  # option "watch" is off
    off.close()
    rx = Receiver(watch=True)
    for d in topo.vfos:
        rx.add_vfo(d)
    assert L.sdrx_set_scan(rx.h, 1, byref(good)) == _lib.SDRX_ESTATE  # before finalize
    assert L.sdrx_get_scan(rx.h, 1, byref(out)) == _lib.SDRX_ESTATE
    rx.finalize()
    assert L.sdrx_set_scan(None, 1, byref(good)) == _lib.SDRX_EINVAL
    assert L.sdrx_set_scan(rx.h, 1, byref(good)) == _lib.SDRX_EINVAL  # not watched
    rx.set_watch([1, 2], [1, 1])
    assert L.sdrx_get_scan(rx.h, 1, byref(out)) == _lib.SDRX_ESTATE  # no frame delivered yet
    assert L.sdrx_get_scan(rx.h, 1, None) == _lib.SDRX_EINVAL
    before = rx.stats()["device_bytes"]

    def cfg(**kw):
        c = _lib.ScanCfgC(4, 3, 500, 16 * 256, 1)
        for k, v in kw.items():
            if k.startswith("reserved"):
                c.reserved[int(k[-1])] = v
            else:
                setattr(c, k, v)
        return c

    bad = [cfg(cell_bins=3), cfg(cell_bins=512), cfg(cell_bins=-4), cfg(frames=0), cfg(frames=65537), cfg(floor_permille=-1),
           cfg(floor_permille=1001), cfg(ratio_q8=0), cfg(min_cells=0), cfg(min_cells=2049), cfg(cell_bins=256, min_cells=33),
           cfg(reserved0=1), cfg(reserved1=-1), cfg(reserved2=7), cfg(cell_bins=0, reserved1=1)]
    for c in bad:
        assert L.sdrx_set_scan(rx.h, 1, byref(c)) == _lib.SDRX_EINVAL, [getattr(c, k) for k, _ in c._fields_[:5]] + list(c.reserved)
    for leaf in (3, 0, 99, -1):  # not watched; not a leaf; out of range
        assert L.sdrx_set_scan(rx.h, leaf, byref(good)) == _lib.SDRX_EINVAL, leaf
    assert rx.stats()["device_bytes"] == before, "a refused call allocated something"
    assert _code(lambda: rx.scan_hits(3)) == _lib.SDRX_EINVAL  # not watched
    assert _code(lambda: rx.scan_hits(1)) == _lib.SDRX_EINVAL  # no scan on its source
    for c in (cfg(cell_bins=1, min_cells=8192), cfg(cell_bins=256, min_cells=32), cfg(frames=65536, ratio_q8=2 ** 32 - 1), good):  # the table's corners
        assert L.sdrx_set_scan(rx.h, 2, byref(c)) == 0
    assert _code(lambda: rx.scan_hits(1)) == _lib.SDRX_ESTATE  # before the first completed evaluation
    assert L.sdrx_get_scan_hits(rx.h, 1, None, 4, byref(n), byref(f)) == _lib.SDRX_EINVAL  # a null array beside the id
    assert L.sdrx_get_scan_hits(rx.h, 1, hits, -1, byref(n), byref(f)) == _lib.SDRX_EINVAL
    frames = sc.wt_frames(topo)
    rx.process(frames[0])
    assert rx.scan(1)["integrated"] == 1 and _code(lambda: rx.scan_hits(1)) == _lib.SDRX_ESTATE
    rx.submit(frames[1])
    assert L.sdrx_set_scan(rx.h, 1, byref(cfg(cell_bins=3))) == _lib.SDRX_EINVAL  # the values come before what the call waits for
    assert _code(lambda: rx.set_scan(1, **sc.WT_CARRIERS)) == _lib.SDRX_ESTATE  # a submitted frame is undelivered
    assert _code(lambda: rx.scan_hits(1)) == _lib.SDRX_ESTATE
    assert rx.scan(1)["frame"] == 0  # the delivered frame's record, while the next is in flight
    rx.wait()
    assert rx.scan(1)["frame"] == 1 and rx.scan(1)["integrated"] == 2
    rx.close()


# ---- end to end: a carrier nobody is tuned to ------------------------------------------------------------------------------------
def test_a_spare_leaf_is_assigned_to_the_carrier_the_scan_found():
    """watch_tree() with sub 3 parked and mistuned by +7 kHz while its tone is still in the input.  One scan at w = 4; `unassigned`
    against the bands of the seven active subs leaves exactly one hit; `mixer_for` gives the sub's own mixer within one cell
    (15 Hz) plus the 0.5 Hz of the rounding; retuned and unparked, the leaf's caught-up frame and its next frame are what a
    fresh node with that mixer gives (the comparison of test_gpu_catchup.py's burst test)."""
    topo = wr.watch_tree()
    leaf = sc.PARKED_SUB
    usb = list(range(1, 9))
    fs_source = topo.vfos[leaf].fs
    rx = Receiver.from_topology(topo, watch=True, park=True, preroll=True, keep_streams=True, catchup=True)
    rx.set_mixer_freqs([leaf], [topo.vfos[leaf].mixer_freq + sc.PARKED_OFF_HZ])
    rx.set_active([leaf], [0])
    rx.set_watch(usb, [1] * len(usb))
    rx.set_scan(1, **sc.WT_CARRIERS)
    frames = sc.wt_frames(topo)
    rx.process(frames[0])
    rec = rx.scan(leaf)
    assert rec["complete"] == 1 and rec["n_hits"] == 8
    hits, f = rx.scan_hits(1)
    assert f == 0
    bands = [scan.leaf_band_hz(topo.vfos[i]) for i in usb if i != leaf]
    free = scan.unassigned(hits, 4, fs_source, bands)
    assert len(free) == 1, free
    lo, hi, peak = scan.hit_hz(free[0], 4, fs_source)
    mixer = scan.mixer_for(topo.vfos[leaf], peak)
    print(f"hit {free[0]}: {lo:.1f} .. {hi:.1f} Hz, peak {peak:.2f} Hz -> mixer {mixer} (the sub's own: {wr.WT_USB_MIXERS[leaf - 1]})")
    assert abs(mixer - wr.WT_USB_MIXERS[leaf - 1]) <= 4 * fs_source / N + 0.5
    fresh = rr.Node(dataclasses.replace(topo.vfos[leaf], mixer_freq=float(mixer)))
    fresh.process(rx.stream(0))
    caught_up = fresh.payload()
    rx.set_mixer_freqs([leaf], [float(mixer)])
    rx.set_active([leaf], [1])
    rx.process(frames[1])
    assert np.array_equal(_bits(rx.preroll(leaf)), _bits(caught_up)), "the caught-up frame is the fresh node's frame 0"
    fresh.process(rx.stream(0))
    assert np.array_equal(_bits(rx.output(leaf)), _bits(fresh.payload())), "the next frame is the fresh node's frame 1"
    assert int((caught_up.astype(np.int64) ** 2).sum()) > 0
    rx.close()
