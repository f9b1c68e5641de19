"""The band scan without a GPU: the ABI additions, the model tests/scan_ref.py on hand-made spectra, sdrreceiver_amd.scan and the
C++ helpers against formulas written out here, and the conditions the GPU tests rely on for their inputs."""
import ctypes as C
import functools
import os
import re

import numpy as np

import scan_ref as sc
import watch_ref as wr
from sdrreceiver_amd import _lib, scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = sc.N
NEW_SYMBOLS = [p + n for p in ("sdrx_", "sdrx_group_") for n in ("set_scan", "get_scan", "get_scan_hits", "get_scan_cells")]


def test_abi_additions():
    hdr = open(os.path.join(ROOT, "include", "sdrx.h")).read()
    declared = set(re.findall(r"\b(sdrx_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
    assert L.sdrx_abi_version() == 5
    assert "SDRX_SCAN_MAX_HITS 512" in hdr and _lib.SCAN_MAX_HITS == scan.MAX_HITS == sc.MAX_HITS == 512
    assert 'sdrx_kernel_name' in declared and "SDRX_NKERNELS 8" in hdr and _lib.NKERNELS == 8  # (the new kernel is not bracketed)

    def offsets(S, names):
        return [getattr(S, f).offset for f in names]

    assert C.sizeof(_lib.ScanCfgC) == 32
    assert offsets(_lib.ScanCfgC, ("cell_bins", "frames", "floor_permille", "ratio_q8", "min_cells", "reserved")) == [0, 4, 8, 12, 16, 20]
    assert C.sizeof(_lib.ScanHitC) == 32
    assert offsets(_lib.ScanHitC, ("first_cell", "n_cells", "peak_cell", "reserved", "peak_pwr", "reserved_d")) == [0, 4, 8, 12, 16, 24]
    assert C.sizeof(_lib.ScanLevelC) == 64
    assert offsets(_lib.ScanLevelC, ("frame", "floor", "thr", "n_hits", "n_stored", "n_hot", "integrated", "frames", "cell_bins", "measured",
                                     "complete", "reserved")) == [0, 8, 16, 24, 28, 32, 36, 40, 44, 48, 52, 56]
    for struct in ("sdrx_scan_cfg", "sdrx_scan_hit", "sdrx_scan_level"):
        assert f"}} {struct};" in hdr, struct


# ---- the model is the definition ---------------------------------------------------------------------------------------------
def _acc_from_cells(cell, w):
    """an ACC whose cells (display order) are `cell`: the value in the cell's first bin, zeros behind it"""
    display = np.zeros(N)
    display[::w] = cell
    return np.concatenate([display[N // 2:], display[:N // 2]])


def test_display_order_and_cells():
    acc = np.arange(N, dtype=np.float64)
    c = sc.cells(acc, 1)
    assert c[0] == N // 2 and c[N // 2 - 1] == N - 1 and c[N // 2] == 0 and c[N - 1] == N // 2 - 1  # cell 0 begins at -fs/2
    c4 = sc.cells(acc, 4)
    assert c4.shape == (N // 4,) and c4[0] == 4 * (N // 2) + 6 and c4[N // 8] == 6
    assert sc.cells(acc, 256).shape == (32,)
    assert np.array_equal(sc.cells(_acc_from_cells(np.arange(32.0), 256), 256), np.arange(32.0))


def test_left_to_right_is_not_np_sum():
    """((a0 + a1) + a2) + a3 against the pairwise (a0 + a1) + (a2 + a3): 1 + 2^-53 + 2^-53 + ... stays 1 from the left, while
    the pairs' sums 2^-52 are not lost."""
    w = 256
    display = np.zeros(N)
    display[:w] = 2.0 ** -53
    display[0] = 1.0
    acc = np.concatenate([display[N // 2:], display[:N // 2]])
    left = sc.cells(acc, w)[0]
    assert left == 1.0
    assert np.sum(display[:w]) != left, "np.sum adds pairwise: the prescribed order matters"
    serial = 0.0
    for x in display[:w].tolist():
        serial += x
    assert serial == left


def test_ties_at_the_rank_and_the_extremes():
    cell = np.array([5.0] * 10 + [1.0] * 12 + [9.0] * 10)  # C = 32: sorted 12 x 1, 10 x 5, 10 x 9
    acc = _acc_from_cells(cell, 256)
    assert sc.rank(0, 32) == 0 and sc.rank(1000, 32) == 31 and sc.rank(500, 32) == 15 and sc.rank(387, 32) == 11 and sc.rank(388, 32) == 12
    for q, want in ((0, 1.0), (387, 1.0), (388, 5.0), (500, 5.0), (709, 5.0), (710, 9.0), (1000, 9.0)):
        f, hits, _ = sc.evaluate(acc, sc.cfg(256, floor_permille=q, ratio_q8=256))
        assert f["floor"] == want and f["thr"] == want, (q, f)
    f, hits, _ = sc.evaluate(acc, sc.cfg(256, floor_permille=500, ratio_q8=256))  # hot: > 5, the ten 9s -- equal cells are not hot
    assert f["n_hot"] == 10 and hits == [dict(first_cell=22, n_cells=10, peak_cell=22, peak_pwr=9.0)]  # peak: the lowest index of the largest
    f, hits, _ = sc.evaluate(acc, sc.cfg(256, floor_permille=1000, ratio_q8=256))  # nothing lies above the largest
    assert f["n_hot"] == 0 and hits == []
    f, hits, _ = sc.evaluate(acc, sc.cfg(256, floor_permille=0, ratio_q8=257))  # thr = fl(1 x 257/256): the 5s and the 9s, two runs
    assert f["thr"] == 257 / 256 and [(h["first_cell"], h["n_cells"], h["peak_cell"]) for h in hits] == [(0, 10, 0), (22, 10, 22)]


def test_no_wrap_and_min_cells():
    cell = np.ones(32)
    cell[[0, 1, 5, 9, 10, 11, 30, 31]] = [7, 8, 9, 4, 6, 6, 3, 2.5]
    acc = _acc_from_cells(cell, 256)
    f, hits, _ = sc.evaluate(acc, sc.cfg(256, floor_permille=500, ratio_q8=2 * 256))
    assert f["floor"] == 1.0 and f["thr"] == 2.0 and f["n_hot"] == 8
    got = [(h["first_cell"], h["n_cells"], h["peak_cell"], h["peak_pwr"]) for h in hits]
    assert got == [(0, 2, 1, 8.0), (5, 1, 5, 9.0), (9, 3, 10, 6.0), (30, 2, 30, 3.0)]  # a run at cell 0 and one at C - 1: two hits
    f2, hits2, _ = sc.evaluate(acc, sc.cfg(256, floor_permille=500, ratio_q8=2 * 256, min_cells=2))
    assert [h["first_cell"] for h in hits2] == [0, 9, 30] and f2["n_hits"] == 3 and f2["n_hot"] == 8
    f3, hits3, _ = sc.evaluate(acc, sc.cfg(256, floor_permille=500, ratio_q8=2 * 256, min_cells=3))
    assert [h["first_cell"] for h in hits3] == [9]
    everything = np.full(32, 2.0)  # one run of all cells
    f4, hits4, _ = sc.evaluate(_acc_from_cells(everything, 256), sc.cfg(256, floor_permille=0, ratio_q8=128))
    assert hits4 == [dict(first_cell=0, n_cells=32, peak_cell=0, peak_pwr=2.0)]


def test_more_hits_than_stored():
    cell = np.ones(N)
    cell[::2] = 3.0  # 4096 runs of one cell
    f, hits, _ = sc.evaluate(cell_acc := _acc_from_cells(cell, 1), sc.cfg(1, floor_permille=0, ratio_q8=2 * 256))
    assert f["n_hits"] == 4096 and f["n_stored"] == 512 and f["n_hot"] == 4096 and len(hits) == 4096
    it = sc.Integrator(sc.cfg(1, floor_permille=0, ratio_q8=2 * 256))
    rec = it.step(cell_acc, 0)
    assert rec["complete"] == 1 and rec["n_stored"] == 512 and len(it.hits) == 512 and it.hits[-1]["first_cell"] == 1022


def test_zero_and_nan():
    f, hits, cell = sc.evaluate(np.zeros(N), sc.cfg(4, floor_permille=500, ratio_q8=16 * 256))
    assert f == dict(floor=0.0, thr=0.0, n_hits=0, n_stored=0, n_hot=0) and hits == [] and not cell.any()
    cell = np.ones(32)
    cell[3], cell[4], cell[5] = 5.0, np.nan, 5.0
    acc = _acc_from_cells(cell, 256)
    f, hits, got = sc.evaluate(acc, sc.cfg(256, floor_permille=500, ratio_q8=2 * 256))
    assert np.isnan(got[4]) and f["floor"] == 1.0 and f["n_hot"] == 2  # a NaN is not hot: it parts the run
    assert [(h["first_cell"], h["n_cells"]) for h in hits] == [(3, 1), (5, 1)]
    f, hits, _ = sc.evaluate(acc, sc.cfg(256, floor_permille=1000, ratio_q8=256))  # the positive NaN's pattern is the largest: floor NaN
    assert np.isnan(f["floor"]) and np.isnan(f["thr"]) and f["n_hot"] == 0 and hits == []


def test_integrator():
    rng = np.random.default_rng(1)
    p = [rng.random(N) for _ in range(5)]
    it = sc.Integrator(sc.cfg(4, frames=3, floor_permille=500, ratio_q8=300))
    r0 = it.step(p[0], 0)
    assert (r0["integrated"], r0["complete"], r0["measured"], r0["frames"], r0["cell_bins"], r0["n_hot"]) == (1, 0, 1, 3, 4, 0)
    r1 = it.step(None, 1)  # no observation
    assert r1 == dict(frame=1, floor=0.0, thr=0.0, n_hits=0, n_stored=0, n_hot=0, integrated=0, frames=0, cell_bins=0, measured=0, complete=0)
    assert it.step(p[1], 2)["integrated"] == 2 and it.hits is None
    r3 = it.step(p[2], 3)
    want, hits, cell = sc.evaluate((p[0] + p[1]) + p[2], it.c)
    assert r3["complete"] == 1 and r3["integrated"] == 3 and {k: r3[k] for k in want} == want
    assert it.hits == hits[:512] and np.array_equal(it.cells, cell) and it.eval_frame == 3
    r4 = it.step(p[3], 4)  # the next round starts from the frame itself, not from zero plus it
    assert r4["integrated"] == 1 and np.array_equal(it.acc, p[3]) and it.eval_frame == 3


# ---- the host helpers ----------------------------------------------------------------------------------------------------------
def _hits_for_helpers():
    rng = np.random.default_rng(4)
    out = []
    for _ in range(40):
        w = int(2 ** rng.integers(0, 9))
        Cn = N // w
        first = int(rng.integers(0, Cn))
        n = int(rng.integers(1, Cn - first + 1))
        out.append((dict(first_cell=first, n_cells=n, peak_cell=first + int(rng.integers(0, n)), peak_pwr=1.0), w,
                    float(rng.choice([30720.0, 245760.0, 2048000.0, 1e6 / 3]))))
    return out


def test_hit_hz_mixer_for_unassigned():
    for hit, w, fs in _hits_for_helpers():
        lo, hi, peak = scan.hit_hz(hit, w, fs)
        assert lo == (hit["first_cell"] * w - 4096) * (fs / 8192)
        assert hi == ((hit["first_cell"] + hit["n_cells"]) * w - 1 - 4096) * (fs / 8192)
        assert peak == (hit["peak_cell"] * w + (w - 1) / 2 - 4096) * (fs / 8192)
        assert lo <= peak <= hi
    assert scan.hit_hz(dict(first_cell=0, n_cells=1, peak_cell=0), 1, 8192.0) == (-4096.0, -4096.0, -4096.0)
    topo = wr.watch_tree()
    for i in range(1, 10):
        d = topo.vfos[i]
        lo, hi = wr.band_hz(d)
        assert scan.leaf_band_hz(d) == (lo, hi)
        for hz in (-9000.3, 0.0, 1234.5, 7000.49):
            f = scan.mixer_for(d, hz)
            assert isinstance(f, int)
            B = hi - lo
            assert f == (int(np.rint(B / 2 - hz)) if d.demod_usb else int(np.rint(-hz))), (i, hz, f)
            import dataclasses
            lo2, hi2 = wr.band_hz(dataclasses.replace(d, mixer_freq=float(f)))
            assert abs((lo2 + hi2) / 2 - hz) <= 0.5  # `hz` lies in the middle of the retuned band, within the rounding to integer Hz
    assert scan.mixer_for(topo.vfos[1], 0.5) == 480 and scan.mixer_for(topo.vfos[9], 0.5) == 0 and scan.mixer_for(topo.vfos[9], 1.5) == -2  # rint: to even
    fs, w = 30720.0, 4
    hits = [dict(first_cell=c, n_cells=2, peak_cell=c, peak_pwr=1.0) for c in (0, 100, 1024, 2000)]
    spans = [scan.hit_hz(h, w, fs)[:2] for h in hits]
    bands = [(spans[1][1], spans[1][1] + 50.0),    # touches hit 1 at its upper end: closed intervals overlap
             (spans[2][0] - 80.0, spans[2][0] - 1e-9)]  # ends just below hit 2
    assert scan.unassigned(hits, w, fs, bands) == [hits[0], hits[2], hits[3]]
    assert scan.unassigned(hits, w, fs, []) == hits
    assert scan.unassigned(hits, w, fs, [(-1e9, 1e9)]) == []


CPP_PROGRAM = r"""
#include "sdrx_host.hpp"
#include <cstdio>
// instantiates the calls (never called: no device here) and prints the host-side arithmetic for hits read from stdin
void never(sdrx_host::sdrj &r, const sdrx_scan_cfg *c) { r.set_scan(1, c); (void)r.scan(1); (void)r.scan_hits(1); (void)r.scan_cells(1, 4); }
int main() {
    sdrx_scan_hit h = {};
    int w, usb, late, bw, dc, fs_leaf;
    double fs, hz, b_lo, b_hi;
    while (std::scanf("%d %d %d %d %lf %d %d %d %d %d %lf %lf %lf", &h.first_cell, &h.n_cells, &h.peak_cell, &w, &fs, &usb, &late, &bw, &dc, &fs_leaf, &hz,
                      &b_lo, &b_hi) == 13) {
        const sdrx_host::sdrj::scan_hz z = sdrx_host::sdrj::scan_hit_hz(h, w, fs);
        sdrx_vfo_desc d = {};
        d.fs = fs_leaf; d.decimate_count = dc; d.demod_usb = usb; d.late_decimate = late; d.filter_bw_hz = bw;
        const size_t left = sdrx_host::sdrj::scan_unassigned({h}, w, fs, {{b_lo, b_hi}}).size();
        std::printf("%.17g %.17g %.17g %lld %zu\n", z.lo, z.hi, z.peak, sdrx_host::sdrj::scan_mixer_for(d, hz), left);
    }
    return sizeof(sdrx_scan_level) == 64 && sizeof(sdrx_scan_hit) == 32 && sizeof(sdrx_scan_cfg) == 32 ? 0 : 1;
}
"""


def test_cpp_host_helpers(tmp_path):
    """host/sdrx_host.hpp: the scan calls compile against the header, and scan_hit_hz / scan_mixer_for / scan_unassigned give what
    sdrreceiver_amd.scan gives."""
    import subprocess
    from sdrreceiver_amd.topology import VfoDesc
    src = tmp_path / "scan_host.cpp"
    src.write_text(CPP_PROGRAM)
    exe = tmp_path / "scan_host"
    lib_dir = os.path.join(ROOT, "sdrreceiver_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "host"), "-o", str(exe), str(src), "-L", lib_dir, "-lsdrx",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True, timeout=300)
    rng = np.random.default_rng(9)
    rows, text = [], ""
    for hit, w, fs in _hits_for_helpers():
        usb, late, bw, dc = int(rng.integers(0, 2)), int(rng.choice([0, 5, 6])), int(rng.choice([0, 300, 100000])), int(rng.integers(0, 6))
        fs_leaf = int(rng.choice([30720, 245760]))
        lo, hi, _ = scan.hit_hz(hit, w, fs)
        hz = float(rng.uniform(-fs / 2, fs / 2))
        band = [(lo - 100.0, lo), (hi, hi + 1.0), (hi + 1e-6, hi + 5.0), (lo - 9.0, lo - 1e-6), (lo, hi)][int(rng.integers(0, 5))]
        rows.append((hit, w, fs, VfoDesc(parent=0, fs=fs_leaf, decimate_count=dc, mixer_freq=0.0, demod_usb=bool(usb), late_decimate=late,
                                         filter_bw=bw, samples_per_buffer=64), hz, band))
        text += (f"{hit['first_cell']} {hit['n_cells']} {hit['peak_cell']} {w} {fs!r} {usb} {late} {bw} {dc} {fs_leaf} {hz!r} {band[0]!r} "
                 f"{band[1]!r}\n")
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    assert len(out) >= len(rows)
    for (hit, w, fs, desc, hz, band), line in zip(rows, out):
        lo, hi, peak, mixer, left = line.split()
        assert (float(lo), float(hi), float(peak)) == scan.hit_hz(hit, w, fs), (hit, w, fs, line)
        assert int(mixer) == scan.mixer_for(desc, hz), (desc, hz, line)
        assert int(left) == len(scan.unassigned([hit], w, fs, [band])), (hit, band, line)


# ---- the inputs of tests/test_gpu_scan.py that a CPU can rebuild: the oracle's parent stream, which the exact arithmetic
# ---- reproduces bit for bit, frame after frame through one tree
@functools.lru_cache(maxsize=None)
def _wt_psds():
    from oracle import binding as ob
    topo = wr.watch_tree()
    nodes, roots = ob.build_tree("port", topo)
    out = []
    for iq in sc.wt_frames(topo):
        ob.process_roots(roots, iq)
        out.append(wr.psd(nodes[0].stream().view(np.complex64).copy()))
    return topo, out


def _margin(fields, cell):
    """how far, relative to the threshold, the cell nearest to it lies"""
    return float(np.min(np.abs(cell - fields["thr"])) / fields["thr"])


def test_the_gpu_inputs_give_the_eight_carriers():
    """watch_tree() with one tone per USB sub over unit noise, w = 4, q = 500, ratio 16: exactly eight hits, each containing the
    cell of one tone, for every single frame (M = 1) and for the three integrated (M = 3)."""
    topo, psds = _wt_psds()
    tones = sc.wt_tone_cells(topo, 4)
    assert len(set(tones)) == 8
    cases = [(f"M=1 seed {s}", p) for s, p in zip(sc.WT_SEEDS, psds)] + [("M=3", (psds[0] + psds[1]) + psds[2])]
    for name, acc in cases:
        fields, hits, cell = sc.evaluate(acc, sc.WT_CARRIERS)
        spans = [(h["first_cell"], h["first_cell"] + h["n_cells"] - 1) for h in hits]
        print(name, "hits", [(a, b - a + 1) for a, b in spans], "margin", _margin(fields, cell))
        assert fields["n_hits"] == 8, (name, spans)
        for t, (a, b) in zip(sorted(tones), spans):
            assert a <= t <= b, (name, t, a, b)


def test_the_gpu_inputs_exercise_the_list():
    topo, psds = _wt_psds()
    for p in psds[:1] + [(psds[0] + psds[1]) + psds[2]]:
        noise, _, _ = sc.evaluate(p, sc.WT_NOISE)
        print("w = 1, ratio 4:", noise["n_hits"], "hits")
        assert 100 < noise["n_hits"] < 512, noise
        trunc, _, _ = sc.evaluate(p, sc.WT_TRUNCATED)
        print("w = 1, ratio 1:", trunc["n_hits"], "hits")
        assert trunc["n_hits"] > 512 and trunc["n_stored"] == 512, trunc
        three, _, _ = sc.evaluate(p, dict(sc.WT_NOISE, min_cells=3))
        assert 0 < three["n_hits"] < noise["n_hits"]  # (min_cells 1 against 3 is a difference on this input)


def test_the_edge_tone_gives_two_hits():
    """One tone at -fs/2 of drift_tree's raw frame: its skirt lies in display bins N - 1, 0 and 1, so the first and the last cell
    are hot -- two hits, never one."""
    import drift_ref as dr
    for n_parent in (8704, 24832):
        topo = dr.drift_tree(n_parent)
        p = wr.psd(sc.edge_tone_frame(topo).view(np.complex64))
        for w in (1, 4):
            fields, hits, cell = sc.evaluate(p, sc.cfg(w, floor_permille=500, ratio_q8=64 * 256))
            C_ = N // w
            assert fields["n_hits"] == 2 and hits[0]["first_cell"] == 0 and hits[1]["first_cell"] + hits[1]["n_cells"] == C_, (n_parent, w, hits)


# ---- the crafted inputs of tests/test_gpu_scan_crafted.py: every condition that file relies on, on the model's own PSD ----------
@functools.lru_cache(maxsize=None)
def _crafted_psd(name, arg=None):
    topo = sc.crafted_tree()
    build = dict(comb=sc.comb_frame, all_hot=sc.all_hot_frame, spread=sc.spread_comb_frame, edge=sc.edge_noise_frame)
    iq = sc.ruler_for(topo, arg) if name == "ruler" else sc.ruler2_frames(topo)[arg] if name == "ruler2" else build[name](topo)
    assert iq.dtype == np.float32 and iq.shape == (2 * topo.frame,) and wr.segments(topo.frame)[0] == 8
    return wr.psd(iq.view(np.complex64))


def _patterns(a):
    return np.unique(np.ascontiguousarray(a, np.float64).view(np.uint64))


def test_crafted_segments_repeat_exactly():
    """The same segment at each of the eight starts: the PSD is exactly 8 x one segment's fp32 power."""
    topo = sc.crafted_tree()
    iq = sc.edge_noise_frame(topo).view(np.complex64)
    one = wr.segment_power(iq[:N]).astype(np.float64)
    assert np.array_equal(_crafted_psd("edge"), 8.0 * one)


def test_comb_ties():
    p = _crafted_psd("comb")
    assert _patterns(p).size == 2 and _patterns(p[0::2]).size == 1 and _patterns(p[1::2]).size == 1
    low, high = float(p[1]), float(p[0])
    assert 0.0 < low < 1e-2 and high > 3e4
    assert sc.rank(500, N) == 4095 and sc.rank(501, N) == 4103  # the last low cell; a high cell
    for q in sc.COMB_LOW_Q:
        f, hits, _ = sc.evaluate(p, sc.cfg(1, floor_permille=q, ratio_q8=sc.COMB_RATIO_Q8))
        assert (f["floor"], f["n_hits"], f["n_stored"], f["n_hot"]) == (low, 4096, 512, 4096)
        assert all(h["n_cells"] == 1 and h["first_cell"] == 2 * i for i, h in enumerate(hits))
    f, hits, _ = sc.evaluate(p, sc.cfg(1, floor_permille=sc.COMB_HIGH_Q, ratio_q8=sc.COMB_RATIO_Q8))
    assert (f["floor"], f["n_hits"], f["n_hot"]) == (high, 0, 0)
    for w in sc.WIDTHS[1:]:
        C_ = N // w
        f, hits, cell = sc.evaluate(p, sc.cfg(w, floor_permille=500, ratio_q8=256))
        assert _patterns(cell).size == 1 and (f["n_hits"], f["n_hot"]) == (0, 0), w  # every cell ties: equal is not hot
        f, hits, cell = sc.evaluate(p, sc.cfg(w, floor_permille=500, ratio_q8=255))
        assert hits == [dict(first_cell=0, n_cells=C_, peak_cell=0, peak_pwr=float(cell[0]))] and f["n_hot"] == C_, w  # the first of C equal largest


def test_all_hot_is_one_run_whose_peak_is_the_argmax():
    p = _crafted_psd("all_hot")
    assert p.min() > 0.0
    for w in sc.WIDTHS:
        C_ = N // w
        for min_cells in (1, C_) + ((32,) if w == 256 else ()):
            f, hits, cell = sc.evaluate(p, sc.all_hot_cfg(w, min_cells))
            assert f["thr"] == cell.min() / 256.0 and f["n_hot"] == C_
            assert hits == [dict(first_cell=0, n_cells=C_, peak_cell=int(np.argmax(cell)), peak_pwr=float(cell.max()))], (w, min_cells)
            if w in sc.ALL_HOT_PEAKS:
                assert hits[0]["peak_cell"] == sc.ALL_HOT_PEAKS[w]
        if C_ >= sc.THREADS:  # the run ends in the last wave; its peak lies in an inner one and reaches the end through the waves' totals
            assert 0 < hits[0]["peak_cell"] // (64 * sc.per_thread(w)) < 7, w


def test_ruler_runs_land_on_the_thread_and_wave_grid():
    for w in sc.WIDTHS:
        p = _crafted_psd("ruler", w)
        f, hits, cell = sc.evaluate(p, sc.ruler_cfg(w))
        hot = cell > f["thr"]
        print(w, f, "cold max", cell[~hot].max(), "hot min", cell[hot].min(), [(h["first_cell"], h["n_cells"], h["peak_cell"]) for h in hits])
        assert cell[~hot].max() < 0.7 * f["thr"] and cell[hot].min() > 2.0 * f["thr"], w  # no cell near the threshold
        cond = sc.ruler_conditions(hits, w) if w in sc.RULER_WIDTHS else sc.wide_conditions(hits, w)
        assert all(cond.values()), (w, cond)
        if w in sc.RULER_WIDTHS:
            assert ("one_thread" in cond and "thread_straddle" in cond) == (w < 16)
            want = sorted(sc.ruler_runs(w).values())  # the runs are where they were designed
            assert [(h["first_cell"], h["first_cell"] + h["n_cells"] - 1) for h in hits] == want, w
            long_run = max(hits, key=lambda h: h["n_cells"])
            assert long_run["peak_cell"] == sc.ruler_boosted_cell(w)
        f1, hits1, _ = sc.evaluate(p, sc.ruler_cfg(w, min_cells=sc.second_longest_plus_one(hits)))
        assert f1["n_hits"] == 1 and hits1 == [max(hits, key=lambda h: h["n_cells"])] and f1["n_hot"] == f["n_hot"], w


def test_ruler_over_two_frames_is_the_ruler_of_the_sum():
    a, b = _crafted_psd("ruler2", 0), _crafted_psd("ruler2", 1)
    c = sc.ruler_cfg(sc.RULER2_W, frames=2)
    f, hits, cell = sc.evaluate(a + b, c)
    assert all(sc.ruler_conditions(hits, sc.RULER2_W).values())
    spans = [(h["first_cell"], h["n_cells"]) for h in hits]
    for alone in (a, b):  # neither frame alone has these runs
        assert [(h["first_cell"], h["n_cells"]) for h in sc.evaluate(alone, c)[1]] != spans
    it = sc.Integrator(c)
    assert it.step(a, 0)["complete"] == 0 and it.step(b, 1)["complete"] == 1 and it.hits == hits


def test_spread_comb_fills_the_list_from_every_wave():
    f, hits, cell = sc.evaluate(_crafted_psd("spread"), sc.SPREAD_CFG)
    hot = cell > f["thr"]
    assert cell[~hot].max() < 0.1 * f["thr"] and cell[hot].min() > 2.0 * f["thr"]
    assert f["n_hits"] == f["n_stored"] == N // sc.SPREAD_L == 256 and f["n_hot"] == 3 * 256
    assert np.bincount([h["first_cell"] // 1024 for h in hits], minlength=8).tolist() == [32] * 8  # every wave writes its 32
    assert all(h["n_cells"] == 3 and h["peak_cell"] == h["first_cell"] + 1 and h["peak_cell"] % 16 == 0 for h in hits)  # each straddles two threads


def test_exactly_512_and_513_hits():
    p = _crafted_psd("edge")
    f512, hits512, _ = sc.evaluate(p, sc.EDGE_512)
    f513, hits513, _ = sc.evaluate(p, sc.EDGE_513)
    assert (f512["n_hits"], f512["n_stored"]) == (512, 512) and (f513["n_hits"], f513["n_stored"]) == (513, 512)
    few, hits_few, _ = sc.evaluate(p, sc.EDGE_FEW)
    assert 0 < few["n_hits"] < 100
    assert hits513[511]["first_cell"] < hits513[512]["first_cell"] and hits_few[0] != hits513[0]
