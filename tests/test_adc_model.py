"""The ADC meter without a GPU: the ABI additions, tests/adc_ref.py's model worked by hand, the derived figures
(sdrreceiver_amd.ingest.adc_levels and host/sdrx_host.hpp's) against formulas written out in float64, the gain suggestion, and
-- asserted here, not assumed -- what the crafted frames of tests/test_gpu_adc_meter.py cross and which wrong devices they
catch."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import adc_ref as ar
from sdrreceiver_amd import _lib, ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CU8, CS8, CS16 = ar.CU8, ar.CS8, ar.CS16


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_the_abi_carries_the_new_symbols_and_keeps_its_version():
    names = ("sdrx_get_adc_meter", "sdrx_group_get_adc_meter")
    hdr = open(os.path.join(ROOT, "include", "sdrx.h")).read()
    for name in names:
        assert name in _lib.SYMBOLS and f"int {name}(" in hdr, name
    L = _lib.lib()  # binds every symbol: AttributeError if the library lacks one
    for name in names:
        assert getattr(L, name).argtypes is not None
    assert L.sdrx_abi_version() == 5 and "#define SDRX_ABI_VERSION 5" in hdr
    A, M = _lib.AdcArmC, _lib.AdcMeterC
    assert C.sizeof(A) == 40 and C.sizeof(M) == 184
    assert (A.sum.offset, A.sum_sq.offset, A.min.offset, A.max.offset, A.at_lo.offset, A.at_hi.offset, A.longest_rail_run.offset) == (0, 8, 16, 20, 24, 28, 32)
    assert (M.frame.offset, M.n_complex.offset, M.fmt.offset, M.measured.offset, M.i.offset, M.q.offset, M.sum_iq.offset, M.bits.offset,
            M.reserved2.offset) == (0, 8, 12, 16, 24, 64, 104, 112, 180)


def test_the_header_structs_have_the_ctypes_layout(tmp_path):
    """the same figures from the C header itself, through a C99 compiler"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sdrx.h"\n'
                   'int main(void) { printf("%u %u %u %u %u %u %u\\n", (unsigned)sizeof(sdrx_adc_arm), (unsigned)sizeof(sdrx_adc_meter),\n'
                   '  (unsigned)offsetof(sdrx_adc_arm, longest_rail_run), (unsigned)offsetof(sdrx_adc_meter, q), (unsigned)offsetof(sdrx_adc_meter, sum_iq),\n'
                   '  (unsigned)offsetof(sdrx_adc_meter, bits), (unsigned)offsetof(sdrx_adc_meter, reserved2)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["40", "184", "32", "64", "104", "112", "180"]


# ---- the model, by hand ---------------------------------------------------------------------------------------------------------
# sixteen samples (I, Q) as codes per format; the same shape in each: a rail run of 3 on I (both rails), a lone rail on Q
HAND = {
    CU8: [(-127, 5), (128, -3), (-127, 0), (1, 128), (0, 0), (7, -8), (64, -64), (127, -126)] + [(2, -2)] * 8,
    CS8: [(-128, 5), (127, -3), (-128, 0), (1, 127), (0, 0), (7, -8), (64, -64), (126, -127)] + [(2, -2)] * 8,
    CS16: [(-32768, 5), (32767, -3), (-32768, 0), (1, 32767), (0, 0), (7, -8), (16384, -16384), (32766, -32767)] + [(2, -2)] * 8,
}
HAND_WANT = {
    CU8: dict(i=dict(sum=-127 + 128 - 127 + 1 + 7 + 64 + 127 + 16, sum_sq=2 * 127 ** 2 + 128 ** 2 + 1 + 49 + 64 ** 2 + 127 ** 2 + 32, min=-127, max=128,
                     at_lo=2, at_hi=1, longest_rail_run=3),
              q=dict(sum=5 - 3 + 128 - 8 - 64 - 126 - 16, sum_sq=25 + 9 + 128 ** 2 + 64 + 64 ** 2 + 126 ** 2 + 32, min=-126, max=128, at_lo=0, at_hi=1,
                     longest_rail_run=1),
              sum_iq=-127 * 5 - 128 * 3 + 128 - 56 - 64 * 64 - 127 * 126 - 32,
              # bit lengths: 0 x3; 1 -> 1; 2 (x16), 3 -> 2; 5, 7 -> 3; 8 -> 4; 64 (x2), 126, 127 (x3) -> 7; 128 (x2) -> 8
              bits=[3, 1, 17, 2, 1, 0, 0, 6, 2] + [0] * 8),
    CS8: dict(i=dict(sum=-128 + 127 - 128 + 1 + 7 + 64 + 126 + 16, sum_sq=2 * 128 ** 2 + 127 ** 2 + 1 + 49 + 64 ** 2 + 126 ** 2 + 32, min=-128, max=127,
                     at_lo=2, at_hi=1, longest_rail_run=3),
              q=dict(sum=5 - 3 + 127 - 8 - 64 - 127 - 16, sum_sq=25 + 9 + 127 ** 2 + 64 + 64 ** 2 + 127 ** 2 + 32, min=-127, max=127, at_lo=0, at_hi=1,
                     longest_rail_run=1),
              sum_iq=-128 * 5 - 127 * 3 + 127 - 56 - 64 * 64 - 126 * 127 - 32,
              bits=[3, 1, 17, 2, 1, 0, 0, 6, 2] + [0] * 8),  # 127 x3, 126, 64 x2 -> 7; 128 x2 -> 8
    CS16: dict(i=dict(sum=-32768 + 32767 - 32768 + 1 + 7 + 16384 + 32766 + 16, sum_sq=2 * 32768 ** 2 + 32767 ** 2 + 1 + 49 + 16384 ** 2 + 32766 ** 2 + 32,
                      min=-32768, max=32767, at_lo=2, at_hi=1, longest_rail_run=3),
               q=dict(sum=5 - 3 + 32767 - 8 - 16384 - 32767 - 16, sum_sq=25 + 9 + 32767 ** 2 + 64 + 16384 ** 2 + 32767 ** 2 + 32, min=-32767, max=32767,
                      at_lo=0, at_hi=1, longest_rail_run=1),
               sum_iq=-32768 * 5 - 32767 * 3 + 32767 - 56 - 16384 * 16384 - 32766 * 32767 - 32,
               bits=[3, 1, 17, 2, 1] + [0] * 10 + [6, 2]),  # 16384 x2, 32766, 32767 x3 -> 15; 32768 x2 -> 16
}


@pytest.mark.parametrize("fmt", ar.FORMATS, ids=ar.NAME.get)
def test_model_on_sixteen_samples_by_hand(fmt):
    codes = np.array(HAND[fmt], np.int64).reshape(-1)
    v = ar.samples_of(codes, fmt)
    assert v.dtype == ingest.FORMATS[fmt] and np.array_equal(ingest.codes(v, fmt), codes)
    got = ar.model(v, fmt, frame=7)
    want = dict(HAND_WANT[fmt], frame=7, n_complex=16, fmt=fmt, measured=1)
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert sum(got["bits"]) == 32
    assert ar.device_like(v, fmt, frame=7) == got


def test_code_tables():
    assert ingest.codes(np.array([0, 127, 128, 255], np.uint8)).tolist() == [-127, 0, 1, 128]
    assert ingest.codes(np.array([-128, 0, 127], np.int8)).tolist() == [-128, 0, 127]
    assert ingest.codes(np.array([-32768, 256, 32767], np.int16)).tolist() == [-32768, 256, 32767]  # the int16 itself, not scaled
    assert ar.bit_lengths([0, 1, -1, 2, 3, 4, 127, 128, -128, 32767, -32768]).tolist() == [0, 1, 1, 2, 2, 3, 7, 8, 8, 15, 16]
    assert (ingest.LOWEST, ingest.HIGHEST) == ({CU8: -127, CS8: -128, CS16: -32768}, {CU8: 128, CS8: 127, CS16: 32767})


# ---- the derived figures ------------------------------------------------------------------------------------------------------
def _float64_levels(v, fmt) -> dict:
    """adc_levels written out on the samples themselves, in float64"""
    x = ingest.codes(v, fmt).astype(np.float64) * (2.0 ** -8 if fmt == CS16 else 1.0)
    i, q = x[0::2], x[1::2]
    var_i, var_q = np.mean(i * i) - np.mean(i) ** 2, np.mean(q * q) - np.mean(q) ** 2
    cov = np.mean(i * q) - np.mean(i) * np.mean(q)
    peak = np.max(np.abs(x))
    rail = (ingest.codes(v, fmt) == ingest.LOWEST[fmt]) | (ingest.codes(v, fmt) == ingest.HIGHEST[fmt])
    return {"dc_i": np.mean(i), "dc_q": np.mean(q), "rms": np.sqrt(np.mean(x * x)), "peak": peak, "headroom_db": 20 * np.log10(128.0 / peak),
            "clip_share": np.mean(rail), "longest_rail_run": max(ar.longest_run(rail[0::2]), ar.longest_run(rail[1::2])),
            "bits_used": int(ar.bit_lengths(ingest.codes(v, fmt)).max()), "gain_imbalance": np.sqrt(var_i / var_q),
            "phase_error": np.arcsin(cov / np.sqrt(var_i * var_q))}


def _imbalanced(fmt, n=4096, seed=3):
    """noise with a gain imbalance of 1.25, a phase error of 0.1 rad and DC offsets, a few samples at the rails"""
    rng = np.random.default_rng(seed + fmt)
    full = 128 if fmt != CS16 else 32768
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    i = 0.1 * full * 1.25 * a + 0.02 * full
    q = 0.1 * full * (math.sin(0.1) * a + math.cos(0.1) * b) - 0.01 * full
    c = np.empty(2 * n, np.int64)
    c[0::2], c[1::2] = np.rint(i), np.rint(q)
    c = np.clip(c, ingest.LOWEST[fmt], ingest.HIGHEST[fmt])
    c[10:16:2] = ingest.HIGHEST[fmt]
    return ar.samples_of(c, fmt)


# What separates the two computations is rounding alone: the integer route rounds each numerator once (2^-53), the float64 route
# rounds every product and mean (n 2^-53 at worst) and subtracts mean^2 from the mean square, which for these frames loses less
# than a factor 10.  1e-9 relative is three orders above that and six below any figure's meaning.
REL = 1e-9


@pytest.fixture(scope="module")
def levels_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("adc") / "adc_levels_check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", str(exe), os.path.join(ROOT, "host", "adc_levels_check.cpp")])
    return str(exe)


def _cpp_levels(exe, rec) -> dict:
    arm = lambda a: [a["sum"], a["sum_sq"], a["min"], a["max"], a["at_lo"], a["at_hi"], a["longest_rail_run"]]  # noqa: E731
    text = " ".join(str(x) for x in [rec["n_complex"], rec["fmt"]] + arm(rec["i"]) + arm(rec["q"]) + [rec["sum_iq"]] + rec["bits"])
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    keys = ("dc_i", "dc_q", "rms", "peak", "headroom_db", "clip_share", "longest_rail_run", "bits_used", "gain_imbalance", "phase_error")
    return {k: (int(x) if k in ("longest_rail_run", "bits_used") else float(x)) for k, x in zip(keys, out)}


@pytest.mark.parametrize("fmt", ar.FORMATS, ids=ar.NAME.get)
def test_adc_levels_python_and_cpp_against_float64_formulas(fmt, levels_exe):
    v = _imbalanced(fmt)
    rec = ar.model(v, fmt)
    want = _float64_levels(v, fmt)
    assert abs(want["gain_imbalance"] - 1.25) < 0.05 and abs(want["phase_error"] - 0.1) < 0.05  # (the frame is what it says)
    py, cpp = ingest.adc_levels(rec), _cpp_levels(levels_exe, rec)
    for got, who in ((py, "python"), (cpp, "c++")):
        assert got.keys() == want.keys()
        for k in want:
            if k in ("longest_rail_run", "bits_used"):
                assert got[k] == want[k], (who, k)
            else:
                assert got[k] == pytest.approx(want[k], rel=REL, abs=1e-12), (who, k)
    for k in py:  # the same operations in the same order: the two agree to the last bit, but for the two figures that come out
        # of log10 and asin, which no two mathematical libraries round alike (a few ulp)
        assert py[k] == (pytest.approx(cpp[k], rel=1e-14) if k in ("headroom_db", "phase_error") else cpp[k]), k
    assert py["longest_rail_run"] == 3 and py["bits_used"] == (16 if fmt == CS16 else 8) - (fmt != CU8)


def test_adc_levels_at_the_edges(levels_exe):
    zeros = ar.model(ar.crafted(CS16, ar.SMALL_N)["zeros"], CS16)
    for lv in (ingest.adc_levels(zeros), _cpp_levels(levels_exe, zeros)):
        assert lv["peak"] == 0 and lv["headroom_db"] == math.inf and lv["bits_used"] == 0 and lv["clip_share"] == 0
        assert math.isnan(lv["gain_imbalance"]) and math.isnan(lv["phase_error"])
    rails = ar.model(ar.crafted(CU8, ar.SMALL_N)["all_highest"], CU8)
    lv = ingest.adc_levels(rails)
    assert lv["peak"] == 128.0 and lv["headroom_db"] == 0.0 and lv["clip_share"] == 1.0 and lv["longest_rail_run"] == ar.SMALL_N
    assert lv["dc_i"] == 128.0 and lv["rms"] == 128.0 and math.isnan(lv["gain_imbalance"])
    low = ar.model(ar.crafted(CS16, ar.SMALL_N)["all_lowest"], CS16)
    assert ingest.adc_levels(low)["peak"] == 128.0 and ingest.adc_levels(low)["dc_q"] == -128.0  # CS16 codes times 2^-8
    with pytest.raises(ValueError):
        ingest.adc_levels(ar.unmeasured(3))


def _rec_with_peak(code, fmt=CS16, run=0):
    c = np.zeros(64, np.int64)
    c[4] = code
    if run:
        c[20:20 + 2 * run:2] = ingest.HIGHEST[fmt]
    return ar.model(ar.samples_of(c, fmt), fmt)


def test_suggest_tuner_gain():
    gains = [0, 90, 140, 197, 254, 297, 338, 372, 402, 434, 496]  # tenths of a dB
    quiet = _rec_with_peak(328)  # 20 log10(32768 / 328) = 39.99 dB of headroom
    assert ingest.adc_levels(quiet)["headroom_db"] == pytest.approx(39.99, abs=0.01)
    # 12 dB asked: 27.99 dB to give away -> the largest entry at most 27.99 dB above the current one
    assert ingest.suggest_tuner_gain(quiet, gains, 140, 12.0) == 402
    assert ingest.suggest_tuner_gain(quiet, gains, 0, 12.0) == 254
    assert ingest.suggest_tuner_gain(quiet, gains, 297, 12.0) == 496  # the list ends first
    assert ingest.suggest_tuner_gain(quiet, gains, 140, 39.99 - 5.7) == 197 and ingest.suggest_tuner_gain(quiet, gains, 140, 39.99 - 5.6) == 140
    loud = _rec_with_peak(16384)  # 6.02 dB
    assert ingest.suggest_tuner_gain(loud, gains, 402, 12.0) == 338  # 5.98 dB short: down by at least that
    assert ingest.suggest_tuner_gain(loud, gains, 0, 12.0) == 0  # nothing lower to go to
    assert ingest.suggest_tuner_gain(loud, gains, 402, 6.0) == 402
    # a rail run of two: down at once, whatever the headroom says; a single sample at the rail is no run
    clipped = _rec_with_peak(100, run=2)
    assert ingest.adc_levels(clipped)["longest_rail_run"] == 2
    assert ingest.suggest_tuner_gain(clipped, gains, 402, 0.0) == 372
    assert ingest.suggest_tuner_gain(clipped, gains, 402, 20.0) == 197  # (the headroom asks for more than one step)
    assert ingest.suggest_tuner_gain(clipped, gains, 0, 0.0) == 0
    assert ingest.suggest_tuner_gain(_rec_with_peak(100, run=1), gains, 402, 0.0) == 402
    # nothing to go by: an unmeasured frame, an all-zero frame
    assert ingest.suggest_tuner_gain(ar.unmeasured(0), gains, 254, 12.0) == 254
    assert ingest.suggest_tuner_gain(_rec_with_peak(0), gains, 254, 12.0) == 254
    assert ingest.suggest_tuner_gain(quiet, [0, 10, 20, 30], 10, 12.0, unit_db=1.0) == 30
    with pytest.raises(ValueError):
        ingest.suggest_tuner_gain(quiet, [], 0, 12.0)


# ---- what the GPU inputs cross: asserted, not assumed -----------------------------------------------------------------------
def _crosses(start, length, unit):
    return start // unit != (start + length - 1) // unit


@pytest.mark.parametrize("fmt", ar.FORMATS, ids=ar.NAME.get)
def test_boundary_frame_crosses_every_kind_of_boundary(fmt):
    n = ar.CRAFT_N
    assert n % 16 == 0 and n % ar.WAVE != 0 and n > 3 * ar.WG  # ends mid-wave in its fourth workgroup
    assert (ar.LOAD[fmt], ar.THREAD, ar.WAVE, ar.WG) == (16 // (4 if fmt == CS16 else 2), 16, 1024, 4096)
    v = ar.crafted(fmt, n)["boundaries"]
    c = ingest.codes(v, fmt)
    rail = (c == ingest.LOWEST[fmt]) | (c == ingest.HIGHEST[fmt])
    ri, rq = ar.runs_of(rail[0::2]), ar.runs_of(rail[1::2])
    plan = ar.boundary_runs(fmt, n)
    assert sorted(ri) == sorted(plan["i"].values()) and sorted(rq) == sorted(plan["q"].values())  # the runs are exactly the planned ones
    L = ar.LOAD[fmt]
    s, k = plan["i"]["inside_load"]
    assert k >= 2 and not _crosses(s, k, L)
    s, k = plan["i"]["across_loads"]
    assert _crosses(s, k, L) and not _crosses(s, k, ar.THREAD)
    s, k = plan["i"]["across_threads"]
    assert _crosses(s, k, ar.THREAD) and not _crosses(s, k, ar.WAVE)
    s, k = plan["i"]["across_waves"]
    assert _crosses(s, k, ar.WAVE) and not _crosses(s, k, ar.WG)
    s, k = plan["i"]["across_workgroups"]
    assert _crosses(s, k, ar.WG)
    s, k = plan["i"]["whole_workgroup"]  # covers workgroup 2 whole, begins and ends mid-thread
    assert s < 2 * ar.WG and s + k > 3 * ar.WG and s % ar.THREAD != 0 and (s + k) % ar.THREAD != 0
    assert plan["i"]["at_0"][0] == 0 and sum(plan["i"]["at_end"]) == n
    # both rails occur inside the runs
    assert (c[0::2] == ingest.LOWEST[fmt]).any() and (c[0::2] == ingest.HIGHEST[fmt]).any()
    # two runs of equal longest length on Q, and the longest of I is one alone
    lens_q = sorted(k for _, k in rq)
    assert lens_q[-1] == lens_q[-2] and lens_q[-1] > lens_q[-3]
    assert _crosses(*plan["q"]["first_longest"], ar.THREAD)
    rec = ar.model(v, fmt)
    assert rec["i"]["longest_rail_run"] == plan["i"]["whole_workgroup"][1] and rec["q"]["longest_rail_run"] == lens_q[-1]
    # a run on I lies beside none on Q (and the other way round): no sample is at a rail on both arms
    assert not (rail[0::2] & rail[1::2]).any()
    # the small frame: one wave and 17 threads
    assert ar.SMALL_N % ar.WAVE == 17 * ar.THREAD and ar.SMALL_N < ar.WG


@pytest.mark.parametrize("fmt", ar.FORMATS, ids=ar.NAME.get)
def test_all_rail_frames(fmt):
    n = ar.CRAFT_N
    F = ar.crafted(fmt, n)
    for name in ("all_lowest", "all_highest", "alternating"):
        rec = ar.model(F[name], fmt)
        assert rec["i"]["longest_rail_run"] == rec["q"]["longest_rail_run"] == n, name
        assert rec["i"]["at_lo"] + rec["i"]["at_hi"] == n
    alt = ingest.adc_levels(ar.model(F["alternating"], fmt))
    assert abs(alt["dc_i"]) <= 0.5 and alt["rms"] > 127.0  # mean about 0: the mean-removed power is full scale
    if fmt == CS16:  # four squares of a thread already pass 32 bits
        assert 4 * ingest.LOWEST[fmt] ** 2 >= 1 << 32 and 5 * ingest.HIGHEST[fmt] ** 2 >= 1 << 32
    for at in (0, 15, 16, n - 1):
        rec = ar.model(F[f"lowest_at_{at}"], fmt)
        assert rec["bits"][16 if fmt == CS16 else 7 + (fmt == CS8)] == 2 and rec["bits"][0] == 2 * n - 2 and rec["i"]["min"] == ingest.LOWEST[fmt]
    if fmt == CU8:
        assert [int(F[f"bytes_{b}"][0]) for b in (0, 127, 128, 255)] == [0, 127, 128, 255]
        assert ar.model(F["bytes_128"], fmt)["bits"][1] == 2 * n and ar.model(F["bytes_127"], fmt)["bits"][0] == 2 * n


def test_device_like_is_the_model_on_every_crafted_frame():
    for n in (1024, ar.SMALL_N, ar.CRAFT_N):
        for fmt in ar.FORMATS:
            for name, v in ar.crafted(fmt, n).items():
                assert ar.device_like(v, fmt) == ar.model(v, fmt), (n, ar.NAME[fmt], name)


@pytest.mark.parametrize("flaw", ar.FLAWS)
def test_every_wrong_device_changes_a_record(flaw):
    """Each way of getting the kernel wrong shows on at least one crafted frame the GPU test feeds."""
    caught = []
    for fmt in ar.FORMATS:
        for name, v in ar.crafted(fmt, ar.CRAFT_N).items():
            if ar.device_like(v, fmt, flaw=flaw) != ar.model(v, fmt):
                caught.append((ar.NAME[fmt], name))
    assert caught, flaw
    names = {name for _, name in caught}
    fmts = {f for f, _ in caught}
    if flaw == "sum32":
        assert "all_lowest" in names and "all_highest" in names and "cs16" in fmts
    if flaw in ("no_wg_merge", "swap_pre_suf"):
        assert "boundaries" in names and fmts == {"cu8", "cs8", "cs16"}
    if flaw in ("pad_zero", "pad_rail"):
        assert fmts == {"cu8", "cs8", "cs16"}
    if flaw == "b_minus_128":
        assert fmts == {"cu8"} and "bytes_127" in names
    if flaw == "bin15":
        assert fmts == {"cs16"} and "lowest_at_0" in names
    if flaw == "iq_unsigned":
        assert "boundaries" in names
