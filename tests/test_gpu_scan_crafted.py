"""Band scan on the device (k_watch_scan) on CRAFTED spectra: ties for the radix select, runs that cross threads and waves for the
segmented scan, hit counts at and beyond the list's limit, and all nine cell widths.

The source is the raw frame of drift_ref.drift_tree(8704), watched through a parent-less leaf: its PSD is the Hann-windowed FFT of
samples the test chooses (tests/scan_ref.py builds them; tests/test_scan_model.py asserts their conditions without a GPU).  As in
test_gpu_scan.py every record, hit list and cell array is compared BIT FOR BIT with the model evaluated on the PSD THE DEVICE
returned -- no tolerance appears -- and each test asserts its condition (these cells tie, this run crosses three waves, n_hits ==
513) on that same device PSD or on the model's result from it.

One arithmetic is enough: the raw frame's PSD is computed from the input samples as they arrive (watch.hip reads the frame, no
stage of the chain lies before it), so option `exact` has no bearing on anything this file feeds the scan."""
import numpy as np
import pytest

import scan_ref as sc
from sdrreceiver_amd.receiver import Receiver
from test_gpu_scan import _bits, check_evaluation, run_scan  # (run_scan: _same_record on every frame, check_evaluation on a completed one)

pytestmark = pytest.mark.gpu
N = sc.N
LEAF = 4  # drift_ref.DT_RAW_LEAF: parent-less, so its source is the raw frame


def _patterns(a):
    return np.unique(np.ascontiguousarray(a, np.float64).view(np.uint64))


class Crafted:
    """One receiver on crafted_tree() with the raw frame watched; `run` is one setting on one or more frames."""

    def __init__(self):
        self.topo = sc.crafted_tree()
        self.rx = Receiver.from_topology(self.topo, watch=True)
        self.rx.set_watch([LEAF], [1])
        self.f = 0

    def run(self, c, *frames):
        """-> (the model fed the device's PSDs, the device's record, the device's PSD of the last frame)"""
        assert len(frames) == c["frames"]
        it = run_scan(self.rx, LEAF, c, list(frames), first_frame=self.f)
        self.f += len(frames)
        assert it.eval_frame == self.f - 1
        return it, self.rx.scan(LEAF), self.rx.watch_psd(LEAF)[0]

    def close(self):
        self.rx.close()


@pytest.fixture
def dev():
    d = Crafted()
    yield d
    d.close()


def test_comb_ties_at_the_rank_and_the_first_of_equal_largest(dev):
    """Two bit patterns, 4096 cells each: the rank on the last low cell (q = 500) and on a high one (q = 501), with 4096
    candidates and a nonzero rank through all eight passes; 4096 hits, the most there can be.  Folded, every cell ties: nothing is
    hot at ratio 1, and at 255/256 the one run of C cells has the FIRST of C equal largest as its peak."""
    iq = sc.comb_frame(dev.topo)
    for q in sc.COMB_LOW_Q:
        it, rec, psd = dev.run(sc.cfg(1, floor_permille=q, ratio_q8=sc.COMB_RATIO_Q8), iq)
        assert _patterns(psd).size == 2 and _patterns(psd[0::2]).size == 1 and _patterns(psd[1::2]).size == 1 and psd[1] < psd[0]
        assert (rec["floor"], rec["n_hits"], rec["n_stored"], rec["n_hot"]) == (psd[1], 4096, 512, 4096)
        assert [h["first_cell"] for h in it.hits] == list(range(0, 1024, 2))
    it, rec, psd = dev.run(sc.cfg(1, floor_permille=sc.COMB_HIGH_Q, ratio_q8=sc.COMB_RATIO_Q8), iq)
    assert (rec["floor"], rec["n_hits"], rec["n_hot"]) == (psd[0], 0, 0) and it.hits == []
    for w in sc.WIDTHS[1:]:
        C = N // w
        it, rec, psd = dev.run(sc.cfg(w, floor_permille=500, ratio_q8=256), iq)
        assert _patterns(it.cells).size == 1 and (rec["n_hits"], rec["n_hot"]) == (0, 0), w
        it, rec, psd = dev.run(sc.cfg(w, floor_permille=500, ratio_q8=255), iq)
        assert it.hits == [dict(first_cell=0, n_cells=C, peak_cell=0, peak_pwr=float(it.cells[0]))] and rec["n_hot"] == C, w


def test_everything_hot_is_one_run_at_every_width(dev):
    """thr = the smallest cell / 256: one run over all C cells, carried through every thread and wave, its peak the argmax; kept at
    min_cells = C."""
    iq = sc.all_hot_frame(dev.topo)
    for w in sc.WIDTHS:
        C = N // w
        for min_cells in (1, C) + ((32,) if w == 256 else ()):
            it, rec, psd = dev.run(sc.all_hot_cfg(w, min_cells), iq)
            assert psd.min() > 0.0 and (rec["n_hits"], rec["n_hot"]) == (1, C), (w, min_cells, rec)
            assert it.hits == [dict(first_cell=0, n_cells=C, peak_cell=int(np.argmax(it.cells)), peak_pwr=float(it.cells.max()))]
            if C >= sc.THREADS:  # the peak lies in an inner wave: it reaches the run's end through the waves' totals
                assert 0 < it.hits[0]["peak_cell"] // (64 * sc.per_thread(w)) < 7, w


def test_ruler_at_every_width(dev):
    """The ruler of each width: a run that is one thread's cells, two-cell runs across a thread and across a wave boundary, a run
    over more than three waves that begins and ends mid-thread with its peak in an inner wave, runs at a wave's first and last
    cell, at cell 0 and at C - 1.  Then min_cells one above the second-longest run: the long run alone."""
    for w in sc.WIDTHS:
        iq = sc.ruler_for(dev.topo, w)
        it, rec, psd = dev.run(sc.ruler_cfg(w), iq)
        cond = sc.ruler_conditions(it.hits, w) if w in sc.RULER_WIDTHS else sc.wide_conditions(it.hits, w)
        assert all(cond.values()) and rec["n_hits"] == len(it.hits) >= 6, (w, cond, it.hits)
        if w in sc.RULER_WIDTHS:
            assert ("one_thread" in cond and "thread_straddle" in cond) == (w < 16)
            assert max(h["n_cells"] for h in it.hits) >= 3 * 64 * sc.per_thread(w)
        longest = max(it.hits, key=lambda h: h["n_cells"])
        one, rec1, _ = dev.run(sc.ruler_cfg(w, min_cells=sc.second_longest_plus_one(it.hits)), iq)
        assert one.hits == [longest] and rec1["n_hits"] == 1 and rec1["n_hot"] == rec["n_hot"], w


def test_ruler_integrated_over_two_different_frames(dev):
    """M = 2: ACC is the sum of two rulers that each carry half of the plateaus; the runs are those of the sum."""
    a, b = sc.ruler2_frames(dev.topo)
    c = sc.ruler_cfg(sc.RULER2_W, frames=2)
    it, rec, _ = dev.run(c, a, b)
    assert rec["integrated"] == 2 and all(sc.ruler_conditions(it.hits, sc.RULER2_W).values()), it.hits
    alone, _, _ = dev.run(dict(c, frames=1), a)
    assert [(h["first_cell"], h["n_cells"]) for h in alone.hits] != [(h["first_cell"], h["n_cells"]) for h in it.hits]


def test_spread_comb_every_wave_writes_into_the_list(dev):
    """256 hits, 32 ending in each wave's cells, the list not truncated: the exclusive prefix of the hits per thread and the sum
    of the waves' totals place every one."""
    it, rec, _ = dev.run(sc.SPREAD_CFG, sc.spread_comb_frame(dev.topo))
    assert rec["n_hits"] == rec["n_stored"] == len(it.hits) == 256 and rec["n_hot"] == 768
    assert np.bincount([h["first_cell"] // 1024 for h in it.hits], minlength=8).tolist() == [32] * 8
    assert all(h["n_cells"] == 3 and h["peak_cell"] % 16 == 0 for h in it.hits)  # each run straddles two threads


def test_exactly_512_and_513_hits(dev):
    """n_hits == 512: the list is full and nothing is dropped.  n_hits == 513, behind an evaluation with few hits on the same
    source: 512 entries, the model's first 512, nothing of the list before."""
    iq = sc.edge_noise_frame(dev.topo)
    it, rec, psd = dev.run(sc.EDGE_512, iq)
    assert (rec["n_hits"], rec["n_stored"], len(it.hits)) == (512, 512, 512)
    few, rec_few, _ = dev.run(sc.EDGE_FEW, iq)
    assert 0 < rec_few["n_hits"] == len(few.hits) < 100 and len(dev.rx.scan_hits(LEAF)[0]) == rec_few["n_hits"]
    it, rec, psd = dev.run(sc.EDGE_513, iq)
    _, every, _ = sc.evaluate(psd, sc.EDGE_513)
    assert (rec["n_hits"], rec["n_stored"]) == (513, 512) and len(every) == 513
    got, frame = dev.rx.scan_hits(LEAF)
    assert frame == dev.f - 1 and len(got) == 512
    for g, m in zip(got, every[:512]):
        assert {k: g[k] for k in ("first_cell", "n_cells", "peak_cell")} == {k: m[k] for k in ("first_cell", "n_cells", "peak_cell")}
        assert np.array_equal(_bits(np.float64(g["peak_pwr"])), _bits(np.float64(m["peak_pwr"])))
    span = lambda h: (h["first_cell"], h["n_cells"])  # noqa: E731
    assert [span(h) for h in got[:len(few.hits)]] != [span(h) for h in few.hits]  # (the list before is no prefix of this one)
