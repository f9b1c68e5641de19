"""The resampler without a GPU: the ABI, the library's built-in design against sdrreceiver_amd.resample's, the response of the
library's own taps, the refusals, a tone through the model, and eight wrong devices that must each change the model's output
on the inputs tests/test_gpu_resample.py feeds the device."""
import ctypes as C
import os

import numpy as np
import pytest

import resample_ref as rr
from sdrreceiver_amd import _lib, resample as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESPONSE_CASES = [c[:3] for c in rr.CASES] + [(64, 125, 48)]


def _design(L, M, T, atten=80.0, k=1000):
    """The library's taps and info for the ratio L/M at the rates (M k, L k)"""
    lib = _lib.lib()
    info = _lib.ResamplerInfoC()
    taps = np.zeros(rs.MAX_TAPS, np.float32)
    rc = lib.sdrx_resampler_design(M * k, L * k, T, atten, taps.ctypes.data, taps.size, C.byref(info))
    return rc, taps[:L * T].copy(), rs.info_dict(info)


def _code(fs_in, fs_out, T, atten=80.0, cap=rs.MAX_TAPS, taps=True):
    buf = np.zeros(rs.MAX_TAPS, np.float32)
    return _lib.lib().sdrx_resampler_design(fs_in, fs_out, T, atten, buf.ctypes.data if taps else None, cap, None)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
def test_abi_and_ctypes_layout():
    lib = _lib.lib()
    assert lib.sdrx_abi_version() == 5
    I = _lib.ResamplerInfoC
    assert C.sizeof(I) == 48
    assert [(n, getattr(I, n).offset) for n, _ in I._fields_] == [
        ("fs_in", 0), ("fs_out", 4), ("L", 8), ("M", 12), ("taps_per_phase", 16), ("in_frame", 20), ("out_frame", 24), ("reserved", 28),
        ("delay_out_samples", 32), ("passband_hz", 40)]
    for name in ("sdrx_resampler_design", "sdrx_set_resampler", "sdrx_get_resampler", "sdrx_get_resampler_input"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "sdrx.h")).read()
    assert "#define SDRX_ABI_VERSION 5" in header
    for name in ("sdrx_resampler_design", "sdrx_set_resampler", "sdrx_get_resampler", "sdrx_get_resampler_input", "sdrx_resampler_info"):
        assert name in header
    # without a context, without a device: the null-handle answers
    assert lib.sdrx_set_resampler(None, 1000, None, 8) == _lib.SDRX_EINVAL
    assert lib.sdrx_get_resampler(None, None, None, 0) == _lib.SDRX_EINVAL
    assert lib.sdrx_get_resampler_input(None, None, 0) == _lib.SDRX_EINVAL


# ---- the design ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,M,T", RESPONSE_CASES + [(3, 4, 64), (128, 125, 64)])
@pytest.mark.parametrize("atten", [60.0, 80.0, 100.0])
def test_design_is_the_numpy_design_to_one_ulp(L, M, T, atten):
    """Both sides are correct doubles rounded once, so they differ by at most one fp32 ulp of the tap; the 2^-40 max|h| floor
    covers taps next to a zero of the sinc, where the double itself is a difference of nearly equal numbers."""
    rc, got, info = _design(L, M, T, atten)
    if rc == _lib.SDRX_EFILTER:  # (3, 4, 16) and (5, 3, 16) at 100 dB: both sides find the transition wider than the band
        assert atten == 100.0 and L * T <= 80
        with pytest.raises(ValueError):
            rs.design(M * 1000, L * 1000, T, atten)
        return
    assert rc == 0
    want, winfo = rs.design(M * 1000, L * 1000, T, atten)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = np.spacing(np.abs(want)).astype(np.float64) + 2.0 ** -40 * float(np.abs(want).max())
    assert (d <= bound).all(), float((d / bound).max())
    assert info["in_frame"] == 0 and info["out_frame"] == 0
    for key in ("fs_in", "fs_out", "L", "M", "taps_per_phase"):
        assert info[key] == winfo[key], key
    assert info["delay_out_samples"] == (L * T - 1) / (2.0 * M)
    assert info["passband_hz"] == pytest.approx(winfo["passband_hz"], rel=1e-12)


def _response_db(taps, L, nfft=1 << 20):
    H = np.abs(np.fft.rfft(taps.astype(np.float64), nfft)) / L  # relative to the DC gain L
    return np.arange(H.size) / nfft, 20 * np.log10(np.maximum(H, 1e-300))


@pytest.mark.parametrize("L,M,T", RESPONSE_CASES)
def test_response_of_the_librarys_taps_at_80_db(L, M, T):
    """Stop band from fn = 0.5 / max(L, M) on: at most -(A - 2) dB; ripple up to the reported pass band: at most 0.003 dB.
    (The numpy design measures -78.95 .. -80.22 dB and at most 0.0015 dB on these ratios: the 2 dB are twice the worst shortfall.)"""
    rc, taps, info = _design(L, M, T, 80.0)
    assert rc == 0
    f, db = _response_db(taps, L)
    fn = 0.5 / max(L, M)
    stop = float(db[f >= fn].max())
    pb = info["passband_hz"] / (L * info["fs_in"])  # cycles per prototype sample
    ripple = float(np.abs(db[f <= pb]).max())
    print(f"L={L} M={M} T={T}: stop band {stop:.2f} dB, ripple {ripple:.5f} dB")
    assert stop <= -(80.0 - 2.0), stop
    assert ripple <= 0.003, ripple


@pytest.mark.parametrize("L,M,T,atten", [(3, 4, 64, 60.0), (128, 125, 64, 100.0)])
def test_stop_band_at_60_and_100_db(L, M, T, atten):
    rc, taps, _ = _design(L, M, T, atten)
    assert rc == 0
    f, db = _response_db(taps, L)
    stop = float(db[f >= 0.5 / max(L, M)].max())
    print(f"L={L} M={M} T={T} A={atten}: stop band {stop:.2f} dB")
    assert stop <= -(atten - 2.0), stop


# ---- the refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_and_every_rule():
    lib = _lib.lib()
    assert _code(3000, 5000, 8) == _lib.SDRX_EFILTER  # 5/3 with T = 8: the transition is wider than the band
    assert b"wider than the band" in lib.sdrx_last_error(None)
    assert _code(625000, 96000, 32) == _lib.SDRX_EUNSUPPORTED  # (96, 625): M / L = 6.5
    assert rs.refusal(625000, 96000, 32) and rs.refusal(3000, 5000, 8) is None
    with pytest.raises(ValueError):
        rs.design(3000, 5000, 8)
    # L <= 1024
    assert _code(1024, 1025, 32) == _lib.SDRX_EUNSUPPORTED and _code(1023, 1024, 32, taps=False) == 0
    # 1/2 <= M / L <= 4, both ends included
    assert _code(500, 1000, 16) == 0 and _code(499, 1000, 16) == _lib.SDRX_EUNSUPPORTED
    assert _code(4000, 1000, 64) == 0 and _code(4001, 1000, 64) == _lib.SDRX_EUNSUPPORTED
    # T a multiple of 4 in 8 .. 64
    for T, ok in ((4, False), (8, True), (10, False), (12, True), (64, True), (68, False), (0, False), (-8, False)):
        assert (_code(4000, 3000, T) != _lib.SDRX_EUNSUPPORTED) == ok, T  # (short ones may still be SDRX_EFILTER)
        assert (rs.refusal(4000, 3000, T) is None) == ok, T
    assert _code(4000, 3000, 64) == 0
    # L T <= 32768
    assert _code(1023, 1024, 32) == 0 and _code(1023, 1024, 36) == _lib.SDRX_EUNSUPPORTED
    # arguments: rates, attenuation, room
    assert _code(0, 3000, 16) == _lib.SDRX_EINVAL and _code(4000, -1, 16) == _lib.SDRX_EINVAL
    assert _code(4000, 3000, 64, atten=50.0) == _lib.SDRX_EINVAL and _code(4000, 3000, 64, atten=120.5) == _lib.SDRX_EINVAL
    assert _code(4000, 3000, 64, atten=120.0) == 0
    assert _code(4000, 3000, 64, cap=191) == _lib.SDRX_EINVAL and _code(4000, 3000, 64, cap=192) == 0
    # the frame rules of sdrx_finalize, in the model (tests/test_gpu_resample.py asks the library)
    assert rs.refusal(2500000, 1536000, 32, 384000) == "the input frame is not a multiple of 16"
    assert rs.refusal(2500000, 1536000, 32, 380928) is None and rs.in_frame(2500000, 1536000, 380928) == 620000
    assert rs.refusal(4000, 3000, 16, 1297) == "n * M is not a multiple of L"
    assert rs.refusal(4000, 3000, 64, 36) == "the input frame is shorter than taps_per_phase"


def test_frames_gives_the_nearest_valid_pair():
    assert rs.frames(6000000, 6144000, 0.25) == (1500000, 1536000)
    assert rs.frames(10000000, 6144000, 0.25) == (2500000, 1536000)
    assert rs.frames(3000000, 1536000, 0.25) == (750000, 384000)
    assert rs.frames(2400000, 1536000, 0.25) == (600000, 384000)
    assert rs.frames(2048000, 1536000, 0.25) == (512000, 384000)
    assert rs.frames(2500000, 1536000, 0.25, 1024) == (620000, 380928)
    for case in rr.CASES:
        L, M, T, n_in, n = case
        fs_in, fs_out = rr.rates(case)
        assert rs.frames(fs_in, fs_out, n / fs_out, 16) == (n_in, n), case
        assert rs.refusal(fs_in, fs_out, T, n) is None


# ---- the model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rr.CASES, ids=rr.IDS)
def test_three_frames_are_one_long_frame(case):
    L, M, T, n_in, n = case
    h = rr.random_taps(case)
    x = np.concatenate([rr.to_complex(v) for v in rr.arithmetic_frames(case)])
    whole, _ = rs.apply(x, h, L, M)
    got = np.concatenate(rr.model_run(case))
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    again, hist = [], None
    for v in rr.arithmetic_frames(case):  # the definition written out a second time
        y, hist = rr.apply_wrong(rr.to_complex(v), h, L, M, hist, None)
        again.append(y)
    assert np.array_equal(np.concatenate(again).view(np.uint32), whole.view(np.uint32))


@pytest.mark.parametrize("case", rr.CASES, ids=rr.IDS)
def test_tone_comes_out_delayed_and_nothing_else(case):
    """A tone at 0.3 of the pass band: from the second frame on within 2e-4 of the ideal tone delayed by (L T - 1) / (2 M)
    output samples -- twice the 1e-4 an 80 dB design's ripple allows (measured with the numpy design: 2.0e-5 .. 8.6e-5)."""
    L, M, T, n_in, n = case
    fs_in, fs_out = rr.rates(case)
    lib = _lib.lib()
    info = _lib.ResamplerInfoC()
    taps = np.zeros(rs.MAX_TAPS, np.float32)
    assert lib.sdrx_resampler_design(fs_in, fs_out, T, 80.0, taps.ctypes.data, taps.size, C.byref(info)) == 0
    h = taps[:L * T]
    f0 = 0.3 * info.passband_hz
    hist, worst = None, 0.0
    for f in range(rr.N_FRAMES):
        j = np.arange(f * n_in, (f + 1) * n_in, dtype=np.float64)
        x = np.exp(2j * np.pi * f0 * j / fs_in).astype(np.complex64)
        y, hist = rs.apply(x, h, L, M, hist)
        m = np.arange(f * n, (f + 1) * n, dtype=np.float64)
        ideal = np.exp(2j * np.pi * f0 * (m - info.delay_out_samples) / fs_out)
        if f >= 1:
            worst = max(worst, float(np.abs(y.astype(np.complex128) - ideal).max()))
    print(f"L={L} M={M} T={T}: tone error {worst:.2e}")
    assert worst <= 2e-4, worst


@pytest.mark.parametrize("how", rr.WRONG)
@pytest.mark.parametrize("case", rr.CASES, ids=rr.IDS)
def test_wrong_devices_change_the_output(case, how):
    """On the frames and taps of the device's arithmetic test, and on its impulse prototypes over the ramp."""
    L, M, T, n_in, n = case
    h = rr.random_taps(case)
    hist, differs = None, []
    for f, v in enumerate(rr.arithmetic_frames(case)):
        y, hist = rr.apply_wrong(rr.to_complex(v), h, L, M, hist, how)
        differs.append(not np.array_equal(y.view(np.uint32), rr.model_run(case)[f].view(np.uint32)))
    if rr.same_by_construction(case, how):
        assert not any(differs)
        return
    if how == "zero_history":
        assert differs == [False, True, True]  # (the first frame's history IS zero)
    else:
        assert all(differs), differs
    if how in ("fma", "descending_t"):  # (an impulse prototype has one product per output: nothing to order or to fuse)
        return
    caught = False
    for k in rr.impulse_positions(case):
        hk, ha, hb = rr.impulse_taps(case, k), None, None
        for v in rr.ramp_frames(case):
            x = rr.to_complex(v)
            a, ha = rs.apply(x, hk, L, M, ha)
            b, hb = rr.apply_wrong(x, hk, L, M, hb, how)
            caught |= not np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert caught
