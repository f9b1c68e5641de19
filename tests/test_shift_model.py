"""The frequency shift's model (sdrreceiver_amd.shift, the definition the device is held to): the ABI additions, the tables and the
conversion pair against the library's, the identity, the accuracy of three tables against a double-precision rotation, the wrong
devices of tests/shift_ref.py, and the method end to end -- with the drift estimate and through the oracle's tree.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import drift_ref as dr
import shift_ref as sr
import watch_ref as wr
from oracle import binding as ob
from sdrreceiver_amd import _lib, shift as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sdrx_set_shift", "sdrx_get_shift", "sdrx_shift_tables", "sdrx_shift_inc", "sdrx_shift_hz"]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def test_abi_additions():
    hdr = open(os.path.join(ROOT, "include", "sdrx.h")).read()
    declared = set(re.findall(r"\b(sdrx_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.sdrx_abi_version() == 5
    assert "#define SDRX_SHIFT_LOAD_PHASE 1u" in hdr and sh.LOAD_PHASE == 1
    K, R = _lib.ShiftCfgC, _lib.ShiftRecordC
    assert C.sizeof(K) == 32 and [getattr(K, f).offset for f in ("inc", "phase0", "flags", "reserved")] == [0, 4, 8, 12]
    assert C.sizeof(R) == sh.RECORD_BYTES == 64
    assert [getattr(R, f).offset for f in ("frame", "n_complex", "applied", "phase", "inc", "next_phase", "next_inc", "reserved")] == [0, 8, 12, 16, 20, 24, 28, 32]
    assert "SDRX_NKERNELS 8" in hdr  # (the new kernels run inside the ingest bracket)


def test_tables_are_the_librarys_bit_for_bit():
    got = np.zeros(3 * sh.TAB * 2, np.float32)
    _lib.lib().sdrx_shift_tables(got.ctypes.data)
    want = np.concatenate(sh.tables()).view(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    A, B, Ct = sh.tables()
    assert A[0] == B[0] == Ct[0] == 1 and A[64] .imag == 1 and A[128].real == -1 and A[192].imag == -1


def test_the_conversion_pair_and_its_errors():
    L = _lib.lib()
    u = C.c_uint32()
    rng = np.random.default_rng(4)
    pairs = [(2048000.0, 0.4), (2048000.0, -0.4), (2048000.0, 250000.0), (1e6, 5e5), (1e6, -5e5), (48000.0, 0.0), (30720.0, -45.0), (3.0, 1.0), (2.0 ** 32, 0.5),
             (2.0 ** 32, 1.5), (2.0 ** 32, 2.5), (2.0 ** 32, -0.5), (2.0 ** 32, -1.5)]
    pairs += [(float(fs), float(rng.uniform(-fs / 2, fs / 2))) for fs in rng.uniform(1e3, 1e8, 200)]
    for fs, hz in pairs:
        assert L.sdrx_shift_inc(fs, hz, C.byref(u)) == 0 and u.value == sh.inc_of(fs, hz), (fs, hz)
        assert L.sdrx_shift_hz(fs, u.value) == sh.hz_of(fs, u.value)
        assert abs(sh.hz_of(fs, u.value) - hz) <= fs / 2.0 ** 33 * (1 + 1e-9) or abs(hz) == fs / 2  # half a unit; +-fs/2 are one point
    # ties go to the even integer; the words wrap
    assert [sh.inc_of(2.0 ** 32, v) for v in (0.5, 1.5, 2.5, -0.5, -1.5)] == [0, 2, 2, 0, 0xFFFFFFFE]
    assert sh.inc_of(1e6, 5e5) == sh.inc_of(1e6, -5e5) == 2 ** 31 and sh.hz_of(1e6, 2 ** 31) == -5e5 and sh.hz_of(1e6, 2 ** 32 - 1) == -1e6 / 2 ** 32
    nan, inf = float("nan"), float("inf")
    for fs, hz in ((0.0, 0.0), (-1.0, 0.0), (nan, 0.0), (inf, 0.0), (1e6, nan), (1e6, inf), (1e6, -inf), (1e6, 500000.1), (1e6, -500000.1)):
        assert L.sdrx_shift_inc(fs, hz, C.byref(u)) == _lib.SDRX_EINVAL, (fs, hz)
        with pytest.raises(ValueError):
            sh.inc_of(fs, hz)
    assert L.sdrx_shift_inc(1e6, 1.0, None) == _lib.SDRX_EINVAL
    # follow: the sign and the clamp
    assert sh.follow(100.0, 45.0, fs=30720.0) == 55.0 and sh.follow(-10.0, -7.5, 0.5, fs=30720.0) == -6.25
    assert sh.follow(15000.0, -1000.0, fs=30720.0) == 15360.0 and sh.follow(-15000.0, 1000.0, fs=30720.0) == -15360.0
    assert sh.check_cfg(sh.Cfg(1, 2, 1)) is None and sh.check_cfg(sh.Cfg(1, 2, 2)) and sh.check_cfg(sh.Cfg(2 ** 32, 0)) and sh.check_cfg(sh.Cfg(0, -1))


def test_the_identity_at_zero_phase_and_zero_increment():
    """Finite samples other than -0 keep their bits; a -0 component may become +0 (x - fl(y 0) with y 0 = -0 is x + 0)"""
    rng = np.random.default_rng(6)
    x = np.concatenate([sr.crafted_samples(rng, 4000), np.zeros(8, np.complex64), np.array([1e-30 + 3e38j, -3e38 - 1e-38j], np.complex64)])
    assert np.array_equal(_bits(sh.mix(x, 0, 0)), _bits(x))
    z = np.array([complex(-0.0, 1.0), complex(1.0, -0.0), complex(-0.0, -0.0), complex(-0.0, 0.0)], np.complex64)
    y = sh.mix(z, 0, 0)
    assert np.array_equal(y, z)  # equal as numbers
    assert not np.signbit(y[1].imag) and not np.signbit(y[2].real) and np.signbit(y[2].imag)  # fl(1 0) + fl(-0 1) = +0; fl(-0 1) - fl(-0 0) = -0 - -0 = +0
    for c in sr.crafted():
        if c.cfgs[0] == sh.Cfg(0, 0) and c.finite:
            zs, ys, _ = sr.model_run(c)
            assert all(np.array_equal(a, b) for a, b in zip(zs, ys)), c.name


ACC_N, ACC_FS = 384000, 2048000.0
ACC_HZ = (0.4, 1234.5, -45678.9, 250000.0)
ACC_MAX, ACC_RMS = 5.1e-7, 2.4e-7  # what this test finds (printed); asserted with a margin of a factor 2


def test_accuracy_against_a_double_rotation():
    """The model against x exp(j 2 pi p / 2^32) in double, n = 384 000, four shifts between 0.4 Hz and 250 kHz at 2.048 MS/s: the
    error relative to |x|.  Found: largest 5.1e-7, rms 2.4e-7 (three roundings in each of three products, 2^-24 each, and 2 pi
    2^-24 = 3.7e-7 rad for the dropped byte).  The two-table variant (11 + 11 bits) is three times worse: 1.6e-6."""
    rng = np.random.default_rng(12)
    x = (rng.standard_normal(ACC_N) + 1j * rng.standard_normal(ACC_N)).astype(np.complex64)
    worst, rms, worst2 = 0.0, 0.0, 0.0
    for k, hz in enumerate(ACC_HZ):
        inc, phase = sh.inc_of(ACC_FS, hz), 0x1234567 * (k + 1)
        ref = sh.reference(x, phase, inc)
        e = np.abs(sh.mix(x, phase, inc) - ref) / np.abs(x)
        e2 = np.abs(sr.apply_wrong(x, sh.State(phase, inc, 0), "two_tables", ACC_N)[0] - ref) / np.abs(x)
        print(f"{hz} Hz: inc {inc}, max {e.max():.3e}, rms {np.sqrt((e ** 2).mean()):.3e}; two tables: max {e2.max():.3e}")
        worst, rms, worst2 = max(worst, float(e.max())), max(rms, float(np.sqrt((e ** 2).mean()))), max(worst2, float(e2.max()))
    assert worst <= 2 * ACC_MAX and rms <= 2 * ACC_RMS, (worst, rms)
    assert worst >= ACC_MAX / 2 and worst2 > 2 * worst  # (the figure is a live one, and the reason for three tables holds)


def test_the_second_writing_of_the_definition_is_the_model():
    for c in sr.crafted():
        assert sr.same_run(sr.run_wrong(c, None), sr.model_run(c)[1:]), c.name


@pytest.mark.parametrize("how", sr.WRONG)
def test_every_wrong_device_shows_on_a_crafted_case(how):
    c = sr.by_name(sr.CAUGHT_BY[how])
    assert not sr.same_run(sr.run_wrong(c, how), sr.model_run(c)[1:]), (how, c.name)


def test_crafted_cases_hold_what_they_are_named_for():
    assert set(sr.CAUGHT_BY) == set(sr.WRONG) and len(sr.WRONG) == 13
    for n in sr.LENGTHS:
        nt = sr.tree_len(n)
        assert nt == (4096 if n == 4112 else n)
        for j0 in sr.wrap_targets(nt):  # the wrap lies where the name says
            c = sr.by_name(f"wrap{j0}_n{n}")
            p = sh.phases(c.cfgs[0].phase0, c.cfgs[0].inc, nt).astype(np.int64)
            assert p[j0 - 1] > 2 ** 32 - c.cfgs[0].inc and p[j0] < c.cfgs[0].inc and bool((np.diff(p) < 0)[j0 - 1])
        assert set(sr.wrap_targets(nt)) == ({7, 1024, 4096} if nt > 4096 else {7, 1024} if nt > 1024 else {7})
        recs = sr.model_run(sr.by_name(f"advance_wraps_n{n}"))[2]
        assert (nt * recs[0]["inc"]) >> 32 >= 100 and recs[0]["next_phase"] == (recs[0]["phase"] + nt * recs[0]["inc"]) % 2 ** 32
        recs = sr.model_run(sr.by_name(f"change_n{n}"))[2]
        assert [r["inc"] for r in recs] == [3451912, 3451912, 0xFF000123, 0xFF000123]
        assert recs[2]["phase"] == recs[1]["next_phase"] and recs[3]["phase"] == 0xC0FFEE00 != recs[2]["next_phase"]
        assert recs[1]["next_inc"] == 3451912  # (what the frame left behind: the change comes after it)
        if not sr.rs_case(n):
            c = sr.by_name(f"nonfinite_n{n}")
            ys = sr.model_run(c)[1]
            for x, y in zip(c.frames, ys):
                bad = ~np.isfinite(y.view(np.float32))
                assert bad.any() and (y.view(np.uint32)[np.isnan(y.view(np.float32))] == sh.NAN_BITS).all()
                assert np.isfinite(y[np.isfinite(x.real) & np.isfinite(x.imag)].view(np.float32)).all()  # a sample's trouble stays its own
            f = sr.by_name(f"zeros_n{n}").frames[0].view(np.float32)
            assert (f == 0).sum() >= 16 and np.signbit(f[f == 0]).any() and not np.signbit(f[f == 0]).all()
    for c in sr.crafted():  # records chain
        recs = sr.model_run(c)[2]
        for f in range(1, sr.N_FRAMES):
            if c.cfgs[f] is c.cfgs[f - 1]:
                assert (recs[f]["phase"], recs[f]["inc"]) == (recs[f - 1]["next_phase"], recs[f - 1]["next_inc"]), (c.name, f)


@pytest.mark.parametrize("bins", [12, -7.3])
def test_follow_leaves_the_drift_estimate_a_residual(bins):
    """Eight tones over unit noise as tests/test_drift_model.py builds them, displaced by `bins` of the estimate's spectrum; the
    frame shifted by what follow() makes of the estimate.  The estimate of the shifted frame reads a residual of at most one bin."""
    fs, n = 30720, 7680
    T = wr.psd(dr.stream(fs, n, 0.0, seed=1))
    x = dr.stream(fs, n, bins * fs / dr.N, seed=2)
    est = dr.estimate(dr.record(dr.profile(T, wr.psd(x), 64))) * fs / dr.N
    hz = sh.follow(0.0, est, fs=fs)
    assert hz * bins < 0  # a band that sits high is moved down
    y = sh.mix(x, 0x13572468, sh.inc_of(fs, hz))
    left = dr.estimate(dr.record(dr.profile(T, wr.psd(y), 64)))
    print(f"displaced {bins} bins, estimate {est:.3f} Hz, shift {hz:.3f} Hz, residual {left:.4f} bins")
    assert abs(left) <= 1.0, (bins, est, left)


def test_sign_against_the_oracle():
    """watch_ref.watch_tree(), one tone mid-band of every USB sub and no noise: the frame with every tone 45 Hz high, shifted by
    -45 Hz by the model, gives the oracle's tree the audio of the undisplaced frame; shifted the other way it does not.
    Tolerance: the shifted frame differs from the undisplaced one by the model's 5.2e-7 of a sample's magnitude and by the
    increment's rounding, at most half a unit, which is n / 2^33 turn = 5.6e-6 rad by the end of the frame: 6.2e-6 of at most 360 (the
    sum of the amplitudes).  A sub's int16 audio has a tone of a few thousand to 30 000 LSB for an amplitude of 20 to 55, so what
    reaches it is below 0.2 LSB and can move a rounding by one: at most 1 LSB.  Measured: 1 LSB at the most, on 0.2 % of the samples; the audio peaks at 3 600 to 18 000 LSB."""
    topo = wr.watch_tree()
    usb = list(range(1, 9))
    tones = dr.wt_tones(topo)

    def audio(z):
        nodes, roots = ob.build_tree("port", topo)
        ob.process_roots(roots, dr.interleaved(z))
        return [nodes[i].usb().astype(np.int32) for i in usb]

    a = audio(dr.stream(topo.fs, topo.frame, 0.0, 1, tones=tones, noise=0.0))
    high = dr.stream(topo.fs, topo.frame, dr.WT_DRIFT_HZ, 1, tones=tones, noise=0.0)
    back = audio(sh.mix(high, 0, sh.inc_of(topo.fs, -dr.WT_DRIFT_HZ)))
    away = audio(sh.mix(high, 0, sh.inc_of(topo.fs, dr.WT_DRIFT_HZ)))
    worst = max(int(np.abs(u - v).max()) for u, v in zip(a, back))
    share = max(float((u != v).mean()) for u, v in zip(a, back))
    print("largest difference", worst, "LSB; largest share of samples that differ", share, "; amplitudes", [int(np.abs(u).max()) for u in a])
    assert min(int(np.abs(u).max()) for u in a) > 1000 and max(int(np.abs(u).max()) for u in a) < 32000
    assert worst <= 1
    assert min(int(np.abs(u - v).max()) for u, v in zip(a, away)) > 100
