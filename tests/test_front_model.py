"""The half-band front stage without a GPU: the ABI, the library's built-in design against sdrreceiver_amd.front's bit for bit, the
design's stop band and ripple, a real tone through the model, the real formats of sdrreceiver_amd.ingest, and nine wrong devices
that must each change the model's output on the inputs tests/test_gpu_front.py feeds the device."""
import ctypes as C
import os

import numpy as np
import pytest

import adc_ref as ar
import front_ref as fx
from sdrreceiver_amd import _lib, front as fr, ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = pytest.mark.parametrize("case", fx.CASES, ids=fx.IDS)
QUALITY = [(K, A) for K in (7, 15, 31) for A in (60.0, 80.0, 100.0)] + [(3, 60.0), (3, 80.0)]
RIPPLE_DB = {60.0: 0.025, 80.0: 0.003, 100.0: 0.0003}


def _design(K, atten=80.0, cap=fr.MAX_N, taps=True):
    lib = _lib.lib()
    info = _lib.FrontInfoC()
    buf = np.zeros(fr.MAX_N, np.float32)
    rc = lib.sdrx_front_design(K, atten, buf.ctypes.data if taps else None, cap, C.byref(info))
    return rc, buf[:fr.n_taps(K)].copy() if 2 <= K <= 31 else buf, fr.info_dict(info)


# ---- the ABI (the library loads, and designs, without a device) ----------------------------------------------------------------
def test_abi_and_ctypes_layout():
    lib = _lib.lib()
    assert lib.sdrx_abi_version() == 5
    I = _lib.FrontInfoC
    assert C.sizeof(I) == 48
    assert [(n, getattr(I, n).offset) for n, _ in I._fields_] == [
        ("real_input", 0), ("stages", 4), ("K", 8), ("N", 12), ("in_frame", 16), ("out_frame", 20), ("reserved", 24), ("tw", 32),
        ("alias_free", 40)]
    header = open(os.path.join(ROOT, "include", "sdrx.h")).read()
    assert "#define SDRX_ABI_VERSION 5" in header and "#define SDRX_FMT_RS16 3" in header and "#define SDRX_FMT_RU12 4" in header
    for name in ("sdrx_front_design", "sdrx_set_front", "sdrx_get_front"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None and name in header
    assert (ingest.RS16, ingest.RU12) == (3, 4)
    # without a context, without a device: the null-handle answers
    assert lib.sdrx_set_front(None, 1, 1, None, 7, 80.0) == _lib.SDRX_EINVAL
    assert lib.sdrx_get_front(None, None, None, 0) == _lib.SDRX_EINVAL


# ---- the design ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 7, 8, 15, 30, 31])
@pytest.mark.parametrize("atten", [50.5, 60.0, 80.0, 100.0, 120.0])
def test_design_is_the_numpy_design_bit_for_bit(K, atten):
    """Both sides run the same IEEE double operations in the same order (the I0 power series, sin of the same libm) and round
    once: the same bits.  Where one finds the transition wider than the band, so does the other."""
    rc, got, info = _design(K, atten)
    try:
        want, winfo = fr.design(K, atten)
    except ValueError:
        assert rc == _lib.SDRX_EFILTER and 0.25 - (atten - 7.95) / (2.285 * (4 * K + 2) * 2 * np.pi) / 2 <= 0
        assert b"wider than the band" in _lib.lib().sdrx_last_error(None)
        return
    assert rc == 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert info == winfo and info["N"] == 4 * K + 3 and info["alias_free"] == 1.0 - 2.0 * info["tw"]
    C_ = fr.centre(K)
    odd = [k for k in range(1, got.size, 2) if k != C_]
    assert not got[odd].view(np.uint32).any() and got[C_] == 0.5
    assert np.array_equal(got, got[::-1])
    fr.check_taps(got)


def test_design_rules():
    lib = _lib.lib()
    assert _design(2, 80.0)[0] == _lib.SDRX_EFILTER  # K = 2 at 80 dB: the transition is wider than the band
    assert _design(2, 60.0)[0] == 0
    for K in (1, 0, -3, 32):
        assert _design(K)[0] == _lib.SDRX_EINVAL
        with pytest.raises(ValueError):
            fr.design(K)
    for atten in (50.0, 120.5, float("nan")):
        assert _design(7, atten)[0] == _lib.SDRX_EINVAL
        with pytest.raises(ValueError):
            fr.design(7, atten)
    assert _design(7, 80.0, cap=30)[0] == _lib.SDRX_EINVAL and _design(7, 80.0, cap=31)[0] == 0
    assert _design(7, 80.0, cap=0, taps=False)[0] == 0
    assert lib.sdrx_front_design(7, 80.0, None, 0, None) == 0


def _response_db(taps, nfft=1 << 18):
    H = np.abs(np.fft.rfft(taps.astype(np.float64), nfft))
    return np.arange(H.size) / nfft, 20 * np.log10(np.maximum(H, 1e-300))


@pytest.mark.parametrize("K,atten", QUALITY)
def test_stop_band_and_ripple_of_the_librarys_taps(K, atten):
    """The taps as the library rounds them to fp32.  Stop band from 0.25 + tw / 2 of the input rate on: at most -(A - 2.5) dB
    (measured -59.03 .. -99.90 dB on these pairs, the worst shortfall 2.17 dB at K = 3, A = 80).  Ripple, peak to peak, up to
    0.25 - tw / 2: at most 0.025 / 0.003 / 0.0003 dB at 60 / 80 / 100 dB (measured 0.0188 / 0.0020 / 0.00017)."""
    rc, taps, info = _design(K, atten)
    assert rc == 0
    f, db = _response_db(taps)
    stop = float(db[f >= 0.25 + info["tw"] / 2].max())
    pb = db[f <= 0.25 - info["tw"] / 2]
    ripple = float(pb.max() - pb.min())
    print(f"K={K} A={atten}: stop band {stop:.2f} dB, ripple {ripple:.5f} dB")
    assert stop <= -(atten - 2.5), stop
    assert ripple <= RIPPLE_DB[atten], ripple


def test_real_tone_comes_out_translated_at_half_its_amplitude():
    """A real sine of amplitude a = 100 at fs_r / 4 + 1 MHz, fs_r = 20 MS/s, through the K = 15, 80 dB stage: a complex tone at
    +1 MHz of the 10 MS/s output, magnitude a / 2 within 2e-4 (measured: a mean of 49.9999); with the doubled taps, a."""
    K, a, fs_r, f_off, n = 15, 100.0, 20e6, 1e6, 40000
    rc, h, _ = _design(K, 80.0)
    assert rc == 0
    hist, hist2, mags, mags2, peak = None, None, [], [], None
    for f in range(3):
        j = np.arange(f * n, (f + 1) * n, dtype=np.float64)
        r = (a * np.cos(2 * np.pi * (fs_r / 4 + f_off) * j / fs_r)).astype(np.float32)
        y, hist = fr.apply(r, h, True, hist)
        y2, hist2 = fr.apply(r, (2 * h).astype(np.float32), True, hist2)
        if f >= 1:
            mags.append(np.abs(y.astype(np.complex128)))
            mags2.append(np.abs(y2.astype(np.complex128)))
            peak = int(np.argmax(np.abs(np.fft.fft(y.astype(np.complex128)))))
    assert peak == round(f_off / (fs_r / 2) * (n // 2))  # bin of +1 MHz at 10 MS/s
    mean, worst = float(np.concatenate(mags).mean()), float(np.abs(np.concatenate(mags) - a / 2).max())
    print(f"tone: mean magnitude {mean:.4f}, worst {worst:.2e}")
    assert abs(mean - a / 2) <= 2e-4 * a / 2 and worst <= 2e-4 * a / 2
    assert abs(float(np.concatenate(mags2).mean()) - a) <= 2e-4 * a
    assert np.array_equal((2 * h).astype(np.float32).astype(np.float64), 2 * h.astype(np.float64))  # doubling is exact


# ---- the real formats on the host -------------------------------------------------------------------------------------------------
def test_real_formats_of_ingest():
    v16 = np.array([-32768, -1, 0, 1, 32767, 256], np.int16)
    assert np.array_equal(ingest.to_float(v16, ingest.RS16), v16.astype(np.float64) / 256)
    v12 = np.array([0, 2047, 2048, 4095, 0xF000 | 2048, 0x8000 | 1], np.uint16)
    assert np.array_equal(ingest.to_float(v12, ingest.RU12), np.array([-2048, -1, 0, 2047, 0, -2047], np.float64) / 16)
    assert np.array_equal(ingest.codes(v12, ingest.RU12), [-2048, -1, 0, 2047, 0, -2047])
    assert np.array_equal(ingest.codes(v16, ingest.RS16), v16.astype(np.int64))
    # a dtype never stands for a real format
    assert ingest.infer_format(v16) == ingest.CS16 and ingest.to_float(v16).dtype == np.float32
    with pytest.raises(TypeError):
        ingest.infer_format(v12)
    with pytest.raises(ValueError):
        ingest.as_samples(v16, ingest.RU12)  # (uint16 is what RU12 takes)
    with pytest.raises(ValueError):
        ingest.as_samples(v12, ingest.RS16)
    with pytest.raises(ValueError):
        ingest.as_samples(v16, 5)
    assert ingest.NAMES["rs16"] == ingest.RS16 and ingest.NAMES["ru12"] == ingest.RU12
    assert ingest.is_real(ingest.RS16) and ingest.is_real(ingest.RU12) and not ingest.is_real(ingest.CS16)


@pytest.mark.parametrize("fmt", fx.REAL_FORMATS)
def test_adc_levels_merges_the_arms_of_a_real_record(fmt):
    n = 4096
    v = fx.full_range(fmt, n, 3)
    v = v.copy()
    lo_word = np.int16(-32768) if fmt == ingest.RS16 else np.uint16(0)
    v[100:107] = lo_word  # a run of 7 real samples at the low rail: 4 in one arm, 3 in the other
    rec = fx.adc_pair_model(v, fmt)
    assert rec["n_complex"] == n // 2 and rec["fmt"] == fmt
    if fmt == ingest.RS16:  # the same memory as CS16 pairs: adc_ref's model, but for the format's name
        assert rec == dict(ar.model(v, ingest.CS16), fmt=fmt)
    lv = ingest.adc_levels(rec)
    c = ingest.codes(v, fmt).astype(np.float64)
    s = 2.0 ** -8 if fmt == ingest.RS16 else 2.0 ** -4
    assert lv["dc"] == pytest.approx(c.mean() * s, rel=1e-12) and lv["rms"] == pytest.approx(np.sqrt((c * c).mean()) * s, rel=1e-12)
    assert lv["peak"] == np.abs(c).max() * s and lv["peak"] == 128.0
    rails = (c == ingest.rails(fmt)[0]) | (c == ingest.rails(fmt)[1])
    assert lv["clip_share"] == rails.sum() / n
    assert lv["longest_rail_run_is_lower_bound"] and 4 <= lv["longest_rail_run"] <= ar.longest_run(rails) <= 2 * lv["longest_rail_run"] + 1
    assert np.isnan(lv["gain_imbalance"]) and np.isnan(lv["phase_error"])


# ---- the model ----------------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_issues_shapes():
    assert [c[:4] + (c[5],) for c in fx.CASES] == [(1, 1, 2, 2592, 1296), (1, 1, 31, 4096, 2048), (0, 1, 7, 2560, 1280), (0, 2, 3, 8192, 2048),
                                                  (1, 3, 7, 16384, 2048), (1, 1, 7, 6400, 2048)]
    assert fx.CASES[5][4] == 3200 and fx.CASES[0][5] % 1024 == 272
    assert fr.frames(2048, 3) == [(16384, 8192), (8192, 4096), (4096, 2048)]
    with pytest.raises(ValueError):
        fr.check_taps(np.ones(31, np.float32))
    h = fx.random_taps(fx.CASES[2])
    h[1] = -0.0  # a negative zero is not +0.0f
    with pytest.raises(ValueError):
        fr.check_taps(h)


@CASE
def test_three_frames_are_one_long_frame(case):
    real, stages, K, in_frame, n0, n, _ = case
    h = fx.random_taps(case)
    x = np.concatenate([fx.to_input(v, fmt) for v, fmt in fx.arithmetic_frames(case)])
    whole, _ = fr.run(x, h, stages, bool(real))
    got = np.concatenate(fx.model_run(case))
    assert got.size == 3 * n0 and np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    again, hists = [], None
    for v, fmt in fx.arithmetic_frames(case):  # the definition written out a second time
        y, hists = fx.run_wrong(fx.to_input(v, fmt), h, stages, real, hists, None)
        again.append(y)
    assert np.array_equal(np.concatenate(again).view(np.uint32), whole.view(np.uint32))


def test_the_real_stage_is_the_complex_stage_on_the_rotated_samples_but_for_zero_signs():
    """z = r (-j)^n through the complex arithmetic gives the same values: the products the real stage leaves out are zeros."""
    case = fx.CASES[1]
    h = fx.random_taps(case)
    v, fmt = fx.arithmetic_frames(case)[0]
    r = fx.to_input(v, fmt)
    a, _ = fr.apply(r, h, True)
    b, _ = fr.apply(fr.rotate(r), h, False)
    assert np.array_equal(a.real, b.real) and np.array_equal(a.imag, b.imag) and a.real.any() and a.imag.any()


@pytest.mark.parametrize("how", fx.WRONG)
@CASE
def test_wrong_devices_change_the_output(case, how):
    """On the frames and taps of the device's arithmetic test, and on its impulse prototypes over the ramps."""
    real, stages, K, in_frame, n0, n, _ = case
    why = fx.same_by_construction(case, how)
    h = fx.random_taps(case)
    hists, differs = None, []
    for f, (v, fmt) in enumerate(fx.arithmetic_frames(case)):
        y, hists = fx.run_wrong(fx.to_input(v, fmt), h, stages, real, hists, how)
        differs.append(not np.array_equal(y.view(np.uint32), fx.model_run(case)[f].view(np.uint32)))
    if why:  # listed with its reason in front_ref.same_by_construction: the device IS the definition here
        assert why in ("the case has no real stage", "the case has one stage") and not any(differs)
        return
    if how in ("zero_history", "stage2_stage1_history"):
        assert differs == [False, True, True]  # (the first frame's histories ARE zero)
    else:
        assert all(differs), differs
    if how in ("fma", "descending_k"):  # (an impulse prototype has one product per output: nothing to order or to fuse)
        return
    caught = False
    for k in fx.impulse_positions(case):
        hk, ha, hb = fx.impulse_taps(case, k), None, None
        for v, fmt in fx.ramp_frames(case):
            x = fx.to_input(v, fmt)
            a, ha = fr.run(x, hk, stages, bool(real), ha)
            b, hb = fx.run_wrong(x, hk, stages, real, hb, how)
            caught |= not np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert caught


def test_every_wrong_device_is_the_definition_only_where_listed():
    listed = {(i, how) for i, c in enumerate(fx.CASES) for how in fx.WRONG if fx.same_by_construction(c, how)}
    assert listed == {(i, how) for i in (2, 3) for how in ("plus_j", "centre_on_i", "real_as_pairs")} | \
        {(i, "stage2_stage1_history") for i in (0, 1, 2, 5)}
