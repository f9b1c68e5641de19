"""The drift estimate without a GPU: the ABI additions, sdrreceiver_amd.drift against the model tests/drift_ref.py, that the
method finds a drift at all, the separation condition the GPU tests rely on, the sign end to end with the oracle, and
mask_template against the model's bands."""
import ctypes as C
import dataclasses
import functools
import glob
import os
import re

import numpy as np
import pytest

import drift_ref as dr
import lattice
import watch_ref as wr
from helpers import SAMPLE_INI
from sdrreceiver_amd import _lib, drift, topology as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sdrx_set_drift", "sdrx_get_drift", "sdrx_get_drift_profile", "sdrx_group_set_drift", "sdrx_group_get_drift",
               "sdrx_group_get_drift_profile"]


def test_abi_additions():
    hdr = open(os.path.join(ROOT, "include", "sdrx.h")).read()
    declared = set(re.findall(r"\b(sdrx_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
    assert L.sdrx_abi_version() == 5
    assert "SDRX_DRIFT_MAX_SHIFT 1024" in hdr and _lib.DRIFT_MAX_SHIFT == drift.MAX_SHIFT == dr.MAX_SHIFT == 1024
    D = _lib.DriftLevelC
    assert C.sizeof(D) == 64
    assert [getattr(D, f).offset for f in ("frame", "peak", "left", "right", "zero", "shift", "max_shift", "measured", "captured",
                                           "reserved")] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56]
    assert 'sdrx_kernel_name' in declared and "SDRX_NKERNELS 8" in hdr  # (the new kernel is not bracketed)


def test_estimate_against_the_model():
    rng = np.random.default_rng(11)
    for _ in range(200):
        K = int(rng.integers(1, 40))
        prof = rng.random(2 * K + 1)
        if rng.random() < 0.3:  # the maximum at an edge of the window
            prof[0 if rng.random() < 0.5 else -1] = 2.0
        rec = dr.record(prof)
        level = dict(rec, frame=0, measured=1, captured=0)
        assert drift.estimate_bins(level) == dr.estimate(rec), (K, rec)
        assert drift.estimate_hz(level, 30720.0) == dr.estimate(rec) * 30720.0 / 8192
    flat = dr.record(np.ones(9))  # denominator 0: the plain shift, which is the first in the order: 0
    assert flat["shift"] == 0 and drift.estimate_bins(dict(flat)) == 0.0
    assert dr.order(2) == [0, -1, 1, -2, 2]
    tie = np.array([5.0, 1.0, 0.0, 1.0, 5.0])  # -2 and +2 tie: -2 comes first
    assert dr.argmax(tie) == -2 and dr.record(tie)["left"] == 0.0 and dr.record(tie)["right"] == 1.0
    assert drift.new_mix_offset(-1200, 44.6) == -1155 and drift.new_mix_offset(300, -7.4) == 293
    d = drift.drift_dict(_lib.DriftLevelC(3, 9.0, 4.0, 5.0, 1.0, -2, 8, 1, 0))
    assert d == {"frame": 3, "peak": 9.0, "left": 4.0, "right": 5.0, "zero": 1.0, "shift": -2, "max_shift": 8, "measured": 1, "captured": 0}


def test_profile_model_is_the_definition():
    rng = np.random.default_rng(5)
    T, p = rng.random(dr.N), rng.random(dr.N)
    prof = dr.profile(T, p, 3)
    for s in range(-3, 4):
        want = sum(float(T[i]) * float(p[(i + s) % dr.N]) for i in range(dr.N))  # plain left-to-right: within N 2^-53
        assert abs(prof[s + 3] - want) <= dr.N * dr.EPS * want


SHAPES = [(30720, 7680), (192000, 48000), (1024, 256)]  # below N, above N with S = 5 segments, far below N
DRIFTS = [12, -7.3, 0.4, 40.6]


@functools.lru_cache(maxsize=None)
def _template(fs, n):
    return wr.psd(dr.stream(fs, n, 0.0, seed=1))


@pytest.mark.parametrize("fs,n", SHAPES)
@pytest.mark.parametrize("bins", DRIFTS)
def test_the_method_finds_a_drift(fs, n, bins):
    """Eight tones over unit noise, the template from a frame without drift (another noise seed): the parabolic estimate lies
    within one bin -- the method's resolution -- of the injected drift.  Measured: within 0.07 bin at the two larger shapes,
    0.2 bin at n = 256 (zero-padded: 32 samples of signal per 1 024 bins of window)."""
    assert wr.segments(n)[0] == {7680: 1, 48000: 5, 256: 1}[n]
    p = wr.psd(dr.stream(fs, n, bins * fs / dr.N, seed=2))
    rec = dr.record(dr.profile(_template(fs, n), p, 64))
    est = dr.estimate(rec)
    print(f"fs {fs} n {n}: injected {bins} bins, shift {rec['shift']}, estimate {est:.4f}")
    assert abs(est - bins) <= 1.0, (fs, n, bins, rec)


# ---- the inputs of tests/test_gpu_drift.py that a CPU can rebuild (the raw frame as source: its PSD is the model's on the frame
# ---- itself; a parent's stream: the oracle's, which the exact arithmetic reproduces bit for bit)
def _oracle_parent_stream(topo, iq):
    from oracle import binding as ob
    nodes, roots = ob.build_tree("port", topo)
    ob.process_roots(roots, iq)
    return nodes, nodes[0].stream().view(np.complex64)


def test_separation_of_the_gpu_inputs():
    """Where a GPU test compares `shift` with the model's, the model's runner-up lies at or below (1 - 1e-6) x its peak, so
    a rounding difference of (N + 4) 2^-53 ~ 1e-12 cannot change the winner.  (The GPU tests assert the same on the device's own
    PSD before they compare.)"""
    worst = 0.0
    topo = wr.watch_tree()
    _, s0 = _oracle_parent_stream(topo, dr.wt_frame(topo, 0.0, seed=5))
    T = wr.psd(s0)
    for drift_hz, seed in ((0.0, 5), (dr.WT_DRIFT_HZ, 6), (-26.25, 7)):
        _, s1 = _oracle_parent_stream(topo, dr.wt_frame(topo, drift_hz, seed=seed))
        prof = dr.profile(T, wr.psd(s1), dr.WT_K)
        assert dr.argmax(prof) == round(drift_hz / 3.75), (drift_hz, dr.argmax(prof))
        worst = max(worst, dr.separation(prof))
    for n_parent in (8704, 24832):
        t = dr.drift_tree(n_parent)
        frames = [dr.raw_frame(t, bins * t.fs / dr.N, seed=seed) for bins, seed in ((0, 1), (dr.RAW_DRIFT_BINS, 2))]
        raw = [wr.psd(iq.view(np.complex64)) for iq in frames]
        parent = [wr.psd(_oracle_parent_stream(t, iq)[1]) for iq in frames]
        for psds, bins in ((raw, dr.RAW_DRIFT_BINS), (parent, 8 * dr.RAW_DRIFT_BINS)):
            for p, want in ((psds[0], 0), (psds[1], bins)):
                prof = dr.profile(psds[0], p, dr.RAW_K)
                assert dr.argmax(prof) == want, (n_parent, want, dr.argmax(prof))
                worst = max(worst, dr.separation(prof))
    print("largest runner-up / peak:", worst)
    assert worst <= dr.SEPARATION


def test_sign_end_to_end_with_the_oracle():
    """watch_ref.watch_tree(), one tone mid-band of every USB sub, the raw frame moved up by +45 Hz = 12 bins of the main's
    3.75 Hz; the template from the undrifted parent stream.  The estimate is +45 Hz within one bin, and moving every sub's mixer by
    -estimate brings each sub's audio power back.

    How far back: the oracle's sum_sq of the eight subs on the undrifted frame is 2.4e9 .. 2.1e10 (tone amplitudes 20 .. 55).  Heard
    45 Hz too high -- uncorrected -- the same tones come out at 0.946 .. 0.964 of that: the passband of a sub's chain (half-band
    stages, audio low-pass) slopes by at most 5.4 % of power over those 12 bins.  The estimate is good to one bin, so what the
    correction leaves is at most 1/12 of that slope, 0.45 %, doubled for curvature: 0.9 %.  Two things ride on top: another noise
    seed alone moves sum_sq by less than 0.1 % (five seeds, undrifted), and the corrected tone still passes the MAIN's filters 45 Hz
    higher than the undrifted one did, where the main is as flat as its own passband -- allowed 0.5 %.  So a corrected sub lies
    within 1.5 % of the undrifted value, and an uncorrected one does not.  Measured: corrected 0.9958 (sub 1, the outermost in the
    main's band) .. 1.0005."""
    topo = wr.watch_tree()
    usb = list(range(1, 9))

    def sum_sq(nodes):
        return np.array([float((nodes[i].usb().astype(np.int64) ** 2).sum()) for i in usb])

    nodes_a, s_a = _oracle_parent_stream(topo, dr.wt_frame(topo, 0.0, seed=5))
    assert max(int(np.abs(nodes_a[i].usb().astype(np.int32)).max()) for i in usb) < 32000  # (no int16 wrapped)
    T = wr.psd(s_a)
    iq_b = dr.wt_frame(topo, dr.WT_DRIFT_HZ, seed=6)
    nodes_b, s_b = _oracle_parent_stream(topo, iq_b)
    rec = dr.record(dr.profile(T, wr.psd(s_b), dr.WT_K))
    level = dict(rec, frame=0, measured=1, captured=0)
    hz = drift.estimate_hz(level, topo.vfos[1].fs)
    bin_hz = topo.vfos[1].fs / dr.N
    print(f"shift {rec['shift']}, estimate {hz:.4f} Hz")
    assert rec["shift"] == 12 and abs(hz - dr.WT_DRIFT_HZ) <= bin_hz, (rec, hz)
    fixed = dataclasses.replace(topo, vfos=[dataclasses.replace(v, mixer_freq=v.mixer_freq - hz) if v.parent == 0 else v
                                            for v in topo.vfos])
    nodes_c, _ = _oracle_parent_stream(fixed, iq_b)
    a, b, c = sum_sq(nodes_a), sum_sq(nodes_b), sum_sq(nodes_c)
    print("undrifted", a, "\nuncorrected / undrifted", b / a, "\ncorrected / undrifted", c / a)
    assert (np.abs(c / a - 1.0) <= 0.015).all(), c / a
    assert (np.abs(b / a - 1.0) > 0.015).all(), b / a


def _count_from_model(topo, leaves):
    want = np.zeros(dr.N, np.float64)
    for i in leaves:
        first, n = wr.band(topo.vfos[i])
        for j in range(n):
            want[(first + j) % dr.N] += 1.0
    return want


def _by_source(topo):
    groups = {}
    for i in range(len(topo.vfos)):
        if not topo.children(i):
            groups.setdefault(topo.vfos[i].parent, []).append(i)
    return groups


def test_mask_template():
    n = 0
    trees = list(lattice.trees().items())
    for path in sorted(glob.glob(os.path.join(SAMPLE_INI, "*.ini"))):
        trees.append((path, tp.topology_from_ini(open(path).read(), name=os.path.basename(path))))
    for name, topo in trees:
        for parent, leaves in _by_source(topo).items():
            t = drift.mask_template(topo, leaves)
            assert t.dtype == np.float64 and t.shape == (dr.N,)
            assert np.array_equal(t, _count_from_model(topo, leaves)), (name, parent)
            n += 1
    assert n > 20
    topo = wr.watch_tree()
    with pytest.raises(ValueError):
        drift.mask_template(dataclasses.replace(topo, vfos=topo.vfos + [dataclasses.replace(topo.vfos[0], topic="X")]), [1, len(topo.vfos)])


CPP_PROGRAM = r"""
#include "sdrx_host.hpp"
#include <cstdio>
// instantiates the trio (never called: no device here) and prints the host-side estimate for records read from stdin
void never(sdrx_host::sdrj &r, const double *t) { r.set_drift(1, t, 8); (void)r.drift(1); (void)r.drift_profile(1, 8); }
int main() {
    sdrx_drift_level r = {};
    double fs;
    while (std::scanf("%lf %lf %lf %d %d %lf", &r.peak, &r.left, &r.right, &r.shift, &r.max_shift, &fs) == 6)
        std::printf("%.17g %.17g\n", sdrx_host::sdrj::drift_bins(r), sdrx_host::sdrj::drift_hz(r, fs));
    return sizeof(sdrx_drift_level) == 64 ? 0 : 1;
}
"""


def test_cpp_host_helpers(tmp_path):
    """host/sdrx_host.hpp: set_drift / drift / drift_profile compile against the header, and drift_bins / drift_hz give the
    model's estimate."""
    import subprocess
    src = tmp_path / "drift_host.cpp"
    src.write_text(CPP_PROGRAM)
    exe = tmp_path / "drift_host"
    lib_dir = os.path.join(ROOT, "sdrreceiver_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "host"), "-o", str(exe), str(src), "-L", lib_dir, "-lsdrx",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True, timeout=300)
    rng = np.random.default_rng(3)
    recs = []
    for _ in range(20):
        K = int(rng.integers(1, 30))
        prof = rng.random(2 * K + 1)
        if rng.random() < 0.3:
            prof[-1] = 2.0
        recs.append(dr.record(prof))
    text = "".join(f"{r['peak']!r} {r['left']!r} {r['right']!r} {r['shift']} {r['max_shift']} 30720\n" for r in recs)
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    for r, line in zip(recs, out):
        bins, hz = (float(x) for x in line.split())
        assert bins == dr.estimate(r) and hz == dr.estimate(r) * 30720.0 / 8192, (r, line)
