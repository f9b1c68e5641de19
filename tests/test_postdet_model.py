"""The post-detection filter's model (sdrreceiver_amd.postdet, the definition the device is held to): the ABI additions, the
library's design against the formula bit for bit and its refusals, the classes of leaf-frames the test trees cover, the crafted
cases of tests/postdet_ref.py -- every wrong device told apart --, the identity, the properties the definition promises, one
functional figure (the stop band on a tone pair) and the INI keys.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import postdet_ref as pr
from sdrreceiver_amd import _lib, detect as dt, postdet as pd, topology as tp
from test_detect_model import ROOT, _ini_with

NEW_SYMBOLS = ["sdrx_set_postfilter", "sdrx_get_postfilter", "sdrx_postfilter_design"]
# The out-of-band tone of the AM pair against the in-band one, both of one amplitude in front of the filter.  The design promises
# atten_db = 60; TONE_MARGIN_DB is what this test lets it miss that by.  Measured here, on the model: the out-of-band tone (4000 Hz,
# well inside the stop band that begins at 1935 Hz) is down by TONE_MEASURED_DB = 75.30 dB, so no margin is taken: 0 dB.
TONE_MARGIN_DB = 0.0
TONE_MEASURED_DB = 75.30


def _design(fs, cutoff, N, atten=80.0, cap=pd.MAX_TAPS, taps=True):
    info = _lib.PostfilterInfoC()
    buf = np.zeros(pd.MAX_TAPS, np.float32)
    rc = _lib.lib().sdrx_postfilter_design(fs, cutoff, N, atten, buf.ctypes.data if taps else None, cap, C.byref(info))
    return rc, buf[:max(min(N, pd.MAX_TAPS), 0)].copy(), pd.info_dict(info)


def test_abi_additions():
    hdr = open(os.path.join(ROOT, "include", "sdrx.h")).read()
    declared = set(re.findall(r"\b(sdrx_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.sdrx_abi_version() == 5
    assert "#define SDRX_POSTFILTER_MAX_TAPS 256\n" in hdr and "#define SDRX_POSTFILTER_MAX_DECIM 16\n" in hdr
    assert (pd.MAX_TAPS, pd.MAX_DECIM) == (256, 16)
    K, I = _lib.PostfilterCfgC, _lib.PostfilterInfoC
    assert C.sizeof(K) == 16 and [getattr(K, f).offset for f in ("decim", "ntaps", "reserved")] == [0, 4, 8]
    assert C.sizeof(I) == 40 and [getattr(I, f).offset for f in ("decim", "ntaps", "out_len", "reserved", "delay_samples", "pass_hz", "stop_hz")] == \
        [0, 4, 8, 12, 16, 24, 32]
    assert "SDRX_NKERNELS 8" in hdr and _lib.NKERNELS == 8  # (the new launches are booked with k_compress)
    assert C.sizeof(_lib.DetectCfgC) == 16 and C.sizeof(_lib.VfoDescC) == 56  # sdrx_detect_cfg and sdrx_vfo_desc do not change
    # without a context, without a device
    assert L.sdrx_set_postfilter(None, 0, None, None) == _lib.SDRX_EINVAL and L.sdrx_get_postfilter(None, 0, None, None, 0) == _lib.SDRX_EINVAL


# ---- the design -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 3, 17, 64, 129, 255, 256])
@pytest.mark.parametrize("atten", [50.5, 60.0, 80.0, 120.0])
@pytest.mark.parametrize("fs,cutoff", [(48000.0, 3000.0), (48000.0, 9600.0), (30720.0, 1500.0), (12000.0, 2999.5)])
def test_design_is_the_formula_bit_for_bit(N, atten, fs, cutoff):
    """Both sides run the same IEEE double operations in the same order (the I0 power series, sin of the same libm, the sum with k
    ascending) and round once: the same bits.  Where one finds that the transition does not fit, so does the other."""
    rc, got, info = _design(fs, cutoff, N, atten)
    tw = (atten - 7.95) / (2.285 * (N - 1) * 2 * np.pi)
    fc = cutoff / fs
    try:
        want, winfo = pd.design(fs, cutoff, N, atten)
    except ValueError:
        assert rc == _lib.SDRX_EFILTER and (fc - tw / 2 <= 0 or fc + tw / 2 > 0.5)
        assert b"does not fit" in _lib.lib().sdrx_last_error(None)
        return
    assert rc == 0 and fc - tw / 2 > 0 and fc + tw / 2 <= 0.5
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert info == winfo and info["pass_hz"] == (fc - tw / 2) * fs and info["stop_hz"] == (fc + tw / 2) * fs
    assert info["delay_samples"] == (N - 1) / 2 and info["ntaps"] == N and info["decim"] == 0 and info["out_len"] == 0
    assert abs(float(want.astype(np.float64).sum()) - 1.0) < 1e-6, "unit DC gain"
    assert np.array_equal(want, want[::-1]), "linear phase"


def test_design_does_what_it_says():
    """The stop band of a design is down by its atten_db (less 1 dB: the Kaiser formula is an estimate), the pass band flat"""
    for N, atten, cutoff in ((129, 60.0, 1500.0), (255, 80.0, 3000.0), (64, 60.0, 3000.0)):
        rc, h, info = _design(float(pr.FS), cutoff, N, atten)
        assert rc == 0
        H = np.abs(np.fft.rfft(h.astype(np.float64), 1 << 16))
        f = np.arange(H.size) * pr.FS / (1 << 16)
        stop = 20 * np.log10(H[f >= info["stop_hz"]].max())
        ripple = 20 * np.log10(H[f <= info["pass_hz"]].max() / H[f <= info["pass_hz"]].min())
        print(f"N={N} A={atten}: stop band {stop:.2f} dB, ripple {ripple:.5f} dB")
        assert stop < -(atten - 1.0) and ripple < 0.1


def test_design_rules():
    L = _lib.lib()
    assert _design(48000.0, 3000.0, 64)[0] == 0
    assert _design(48000.0, 3000.0, 1)[0] == _lib.SDRX_EFILTER  # one tap: the transition is the whole band
    assert _design(48000.0, 300.0, 64)[0] == _lib.SDRX_EFILTER  # fc - tw/2 <= 0
    assert _design(48000.0, 23900.0, 64)[0] == _lib.SDRX_EFILTER  # fc + tw/2 > 0.5
    for N in (0, -1, 257):
        assert _design(48000.0, 3000.0, N)[0] == _lib.SDRX_EINVAL
        with pytest.raises(ValueError):
            pd.design(48000.0, 3000.0, N)
    for atten in (50.0, 120.5, float("nan")):
        assert _design(48000.0, 3000.0, 64, atten)[0] == _lib.SDRX_EINVAL
        with pytest.raises(ValueError):
            pd.design(48000.0, 3000.0, 64, atten)
    for fs, cut in ((0.0, 3000.0), (-1.0, 3000.0), (48000.0, 0.0), (48000.0, -5.0)):
        assert _design(fs, cut, 64)[0] == _lib.SDRX_EINVAL
        with pytest.raises(ValueError):
            pd.design(fs, cut, 64)
    for args in ((48000.0, 3000.0, 1), (48000.0, 300.0, 64), (48000.0, 23900.0, 64)):
        with pytest.raises(ValueError):
            pd.design(*args)
    assert _design(48000.0, 3000.0, 64, cap=63)[0] == _lib.SDRX_EINVAL and _design(48000.0, 3000.0, 64, cap=64)[0] == 0
    assert _design(48000.0, 3000.0, 64, cap=0, taps=False)[0] == 0
    assert L.sdrx_postfilter_design(48000.0, 3000.0, 64, 80.0, None, 0, None) == 0


# ---- the trees and the cases -----------------------------------------------------------------------------------------------------------
def test_the_trees_cover_the_classes():
    topos = [pr.TREES[k]() for k in sorted(pr.TREES)]
    got = pr.classes(topos)
    want = {"short", "one_block", "block_and_partial", "three_blocks", "edge_R3", "edge_R5", "edge_R6", "R16", "am", "fm", "parentless", "below_main",
            "below_main_of_main"} | {f"T{t}" for t in (1, 2, 17, 64, 255, 256)} | {f"R{r}" for r in (1, 2, 3, 5, 6, 16)}
    assert want <= got, want - got
    for topo in topos:
        for i in pr.filtered_leaves(topo):
            d = topo.vfos[i]
            assert topo.is_leaf(i) and d.detector and pd.refusal(len(d.post_taps), d.post_decim, d.n_stage_out) is None, i
        leaves = [v for i, v in enumerate(topo.vfos) if topo.is_leaf(i)]
        assert any(v.detector and not len(v.post_taps) for v in leaves), "an unfiltered detector leaf beside them"
        assert any(not v.detector and not v.demod_usb for v in leaves), "an IQ leaf beside them"
    assert any(v.demod_usb for v in topos[0].vfos), "a USB leaf beside them"
    short = [(d.n_stage_out, len(d.post_taps)) for t in topos for d in t.vfos if len(d.post_taps) and d.n_stage_out < len(d.post_taps) - 1]
    assert (60, 64) in short
    names = set(pr.case_ids())
    assert {"impulse", "am_tone_pair", "fm_step", "zeros", "wrap", "gain_step", "short"} <= names
    for c in pr.gpu_cases():
        assert all(z.size == pr.N_CRAFT for z in c.frames) and len(c.frames) == pr.N_FRAMES and pr.N_CRAFT % c.decim == 0, c.name


@pytest.mark.parametrize("wrong", pr.WRONG)
def test_every_wrong_device_is_told_apart(wrong):
    assert len(pr.WRONG) >= 12
    for kind in pr.WRONG_KINDS[wrong]:
        changed = {}
        for c in pr.crafted():
            want = pr.model_run(c, kind)
            got = pr.wrong_run(c, kind, wrong)
            if wrong == "meter_over_n":  # the payload is the model's; the meter record is not
                assert all(np.array_equal(a["payload"], b["payload"]) for a, b in zip(got, want))
                changed[c.name] = sum(int(a["n_values"] != b["n_values"]) + int(a["sum_sq"] != b["sum_sq"]) for a, b in zip(got, want))
            else:
                changed[c.name] = sum(int(np.count_nonzero(a["payload"] != b["payload"])) for a, b in zip(got, want))
        assert sum(changed.values()) > 0, (wrong, kind, changed)
    # the variants are the model when nothing is wrong
    c = pr.crafted()[0]
    for kind in (dt.AM, dt.FM):
        assert all(np.array_equal(a["payload"], b["payload"]) for a, b in zip(pr.wrong_run(c, kind, ""), pr.model_run(c, kind)))


@pytest.mark.parametrize("kind", [dt.AM, dt.FM])
def test_identity(kind):
    """T = 1, h = {1.0f}, R = 1: payload and meter are those of the same leaf without the stage, bit for bit"""
    for c in dr_cases():
        g = c.gain_am if kind == dt.AM else c.gain_fm
        plain, st = dt.State(), pd.State()
        for z in c.frames:
            a = dt.run(kind, z, g, plain)
            b = pd.run(kind, z, g, (1.0,), 1, st)
            assert np.array_equal(a["payload"], b["payload"]), c.name
            for k in ("n_values", "sum_sq", "clipped"):
                assert int(a[k]) == int(b[k]), (c.name, k)
            assert np.float32(a["peak"]) == np.float32(b["peak"]), c.name


def dr_cases():
    import detect_ref as dr
    return dr.crafted()  # (the detector's own crafted streams: zeros, 1e-20, wraps, exact pi steps, axes and diagonals)


def test_what_the_definition_promises():
    # the taps read back from a single non-zero value of pre (FM: one quarter turn = 0.5 half-turns at gain 1)
    imp = next(c for c in pr.crafted() if c.name == "impulse")
    h = np.asarray(imp.taps, np.float32)
    runs = pr.model_run(imp, dt.FM)
    y = np.concatenate([r["y"] for r in runs])
    k = pr.N_CRAFT + pr.BLOCK - 6
    assert np.array_equal(y[k:k + h.size], (h * np.float32(0.5)).astype(np.float32)) and not y[:k].any() and not y[k + h.size:].any()
    # frames join without a seam: the model over the joined pre is the model frame by frame (FM; an AM carrier is per frame)
    c = next(c for c in pr.crafted() if c.name == "fm_step")
    runs = pr.model_run(c, dt.FM)
    pre = dt.fm_pre(np.concatenate(c.frames), c.gain_fm)
    whole, _ = pd.fir(pre, c.taps, c.decim)
    assert np.array_equal(whole, np.concatenate([r["y"] for r in runs]))
    assert all(r["n_values"] == pr.N_CRAFT // c.decim == r["payload"].size for r in runs)
    # history spans more than one frame where n < T - 1
    s = next(c for c in pr.crafted() if c.name == "short")
    assert s.frames[0].size == 48 < len(s.taps) - 1
    runs = pr.model_run(s, dt.FM)
    whole, _ = pd.fir(dt.fm_pre(np.concatenate(s.frames), s.gain_fm), s.taps, s.decim)
    assert np.array_equal(whole, np.concatenate([r["y"] for r in runs]))
    # a frame of zeros drains the history and leaves zeros behind it (T - 1 = 254 < n)
    z = next(c for c in pr.crafted() if c.name == "zeros")
    for kind in (dt.AM, dt.FM):
        runs = pr.model_run(z, kind)
        tail = (len(z.taps) - 1 + z.decim - 1) // z.decim
        assert runs[1]["payload"][:tail].any() and not runs[1]["payload"][tail + 1:].any(), kind
    # the wrap case wraps in front of the filter and not behind it
    w = next(c for c in pr.crafted() if c.name == "wrap")
    for kind in (dt.AM, dt.FM):
        g = pr.gain_of(w, kind)
        assert all(dt.run(kind, zf, g, dt.State())["clipped"] > 1000 for zf in w.frames), kind
        assert all(r["clipped"] == 0 for r in pr.model_run(w, kind)[1:]), kind
    # the old gain's values stay in the history: a run with the new gain throughout differs in the first outputs of the frame only
    gs = next(c for c in pr.crafted() if c.name == "gain_step")
    runs = pr.model_run(gs, dt.AM)
    st = pd.State()
    pd.run(dt.AM, gs.frames[0], pr.gain_of(gs, dt.AM, 1), gs.taps, gs.decim, st)
    other = pd.run(dt.AM, gs.frames[1], pr.gain_of(gs, dt.AM, 1), gs.taps, gs.decim, st)
    edge = (len(gs.taps) - 1 + gs.decim - 1) // gs.decim
    assert not np.array_equal(other["payload"][:edge], runs[1]["payload"][:edge]) and np.array_equal(other["payload"][edge:], runs[1]["payload"][edge:])
    # refusals of the model
    for T, R, n in ((0, 1, 48), (257, 1, 4096), (4, 0, 48), (4, 17, 4096), (4, 5, 48)):
        assert pd.refusal(T, R, n) is not None
    assert pd.refusal(256, 16, 4096) is None and pd.refusal(1, 1, 1) is None
    with pytest.raises(ValueError):
        pd.fir(np.zeros(50, np.float32), (1.0, 2.0), 3)


def test_levels():
    topo = pr.tree_c()
    lv = pd.levels(topo.vfos[1])
    assert lv == {"rate": 15360 // 6, "out_len": 2560, "bytes": 5120, "delay_samples": 31.5, "delay_s": 31.5 / 15360}
    assert pd.levels(topo.vfos[8])["rate"] == 7680 and pd.levels(topo.vfos[8])["delay_samples"] == 0.0  # no filter
    assert pd.levels(topo.vfos[8], 17, 3)["out_len"] == 2560
    with pytest.raises(ValueError):
        pd.levels(topo.vfos[8], 17, 7)
    assert topo.vfos[1].n_detect_out == 2560 and topo.vfos[1].detect_rate == 2560 and topo.vfos[8].n_detect_out == 7680


def test_the_out_of_band_tone_is_down_by_the_design():
    """One functional figure, on the model only (the device is the model bit for bit): both tones of the AM pair enter the filter
    with one amplitude; behind it the one outside the pass band (4000 Hz, aliased to 1120 Hz by the decimation) is down by the
    design's atten_db less TONE_MARGIN_DB."""
    c = next(c for c in pr.crafted() if c.name == "am_tone_pair")
    runs = pr.model_run(c, dt.AM)
    y = np.concatenate([r["y"] for r in runs[1:]]).astype(np.float64)  # (frame 0 holds the start from a zero history)
    fs_out = pr.FS / c.decim
    f_alias = abs(pr.TONE_OUT - round(pr.TONE_OUT / fs_out) * fs_out)
    assert f_alias == 1120.0 and pr.TONE_IN < 1065.0 and pr.TONE_OUT > 1935.0
    m0 = pr.N_CRAFT // c.decim
    t = (np.arange(y.size) + m0) / fs_out
    A = np.stack([np.ones_like(t)] + [fn(2 * np.pi * f * t) for f in (pr.TONE_IN, f_alias) for fn in (np.sin, np.cos)], axis=1)
    # the AM carrier is each frame's own mean: one constant per frame
    frames = np.repeat(np.arange(len(runs) - 1), m0)
    A = np.concatenate([A[:, 1:], (frames[:, None] == np.arange(len(runs) - 1)[None, :]).astype(np.float64)], axis=1)
    coef = np.linalg.lstsq(A, y, rcond=None)[0]
    a_in, a_out = np.hypot(coef[0], coef[1]), np.hypot(coef[2], coef[3])
    down = 20 * np.log10(a_in / a_out)
    print(f"in-band tone {a_in:.6f}, out-of-band tone {a_out:.3e}: down by {down:.2f} dB (design: {pr.TONE_ATT} dB)")
    assert a_in == pytest.approx(0.7 * 0.4 * 0.3, rel=1e-3)
    assert down >= pr.TONE_ATT - TONE_MARGIN_DB
    assert abs(down - TONE_MEASURED_DB) < 0.5, "the figure written beside the margin is the measured one"


# ---- the INI keys -----------------------------------------------------------------------------------------------------------------------
def postfilter_ini():
    """(text, topology): sdr_25E.ini with a filtered AM, a filtered FM and an unfiltered FM entry beside the last 48 kS/s sub"""
    from helpers import SAMPLE_INI
    plain = tp.topology_from_ini(open(os.path.join(SAMPLE_INI, "sdr_25E.ini")).read())
    sub = plain.vfos[-1]
    f = int(plain.center_frequency - plain.vfos[sub.parent].mixer_freq - sub.mixer_freq)
    text, _ = _ini_with([
        {"frequency": f + 5000, "gain": 50, "topic": "AIR01", "detector": "am", "post_decim": 6, "post_taps": 64, "post_cutoff_hz": 3000, "post_atten_db": 60},
        {"frequency": f - 5000, "gain": 100, "topic": "AIS01", "detector": "fm", "post_decim": 1, "post_taps": 255, "post_cutoff_hz": 9600.5, "post_atten_db": 80},
        {"frequency": f - 9000, "gain": 100, "topic": "POC01", "detector": "fm"}])
    return text, tp.topology_from_ini(text)


def test_the_ini_keys():
    from helpers import SAMPLE_INI
    plain = tp.topology_from_ini(open(os.path.join(SAMPLE_INI, "sdr_25E.ini")).read())
    assert all(v.post_taps == () and v.post_decim == 1 for v in plain.vfos)
    text, topo = postfilter_ini()
    assert len(topo.vfos) == len(plain.vfos) + 3 and topo.vfos[:len(plain.vfos)] == plain.vfos
    am, fm, poc = topo.vfos[-3:]
    assert am.out_rate_stage == 48000 and (am.post_decim, len(am.post_taps)) == (6, 64) and (fm.post_decim, len(fm.post_taps)) == (1, 255)
    assert np.array_equal(np.asarray(am.post_taps, np.float32), pd.design(48000.0, 3000.0, 64, 60.0)[0]), "designed at the leaf's rate"
    assert np.array_equal(np.asarray(fm.post_taps, np.float32), pd.design(48000.0, 9600.5, 255, 80.0)[0])
    assert poc.detector == dt.FM and poc.post_taps == () and am.detect_rate == 8000 and am.n_detect_out == am.n_stage_out // 6
    sub = plain.vfos[-1]
    f = int(plain.center_frequency - plain.vfos[sub.parent].mixer_freq - sub.mixer_freq)
    full = {"frequency": f, "detector": "am", "post_decim": 6, "post_taps": 64, "post_cutoff_hz": 3000, "post_atten_db": 60}
    for drop in ("post_decim", "post_taps", "post_cutoff_hz", "post_atten_db"):  # all four or none
        with pytest.raises(ValueError, match="all four keys or none"):
            tp.topology_from_ini(_ini_with([{k: v for k, v in full.items() if k != drop}])[0])
    with pytest.raises(ValueError, match="detector=am"):
        tp.topology_from_ini(_ini_with([{k: v for k, v in full.items() if k != "detector"}])[0])
    for key, val, what in (("post_decim", 17, "decim must be"), ("post_decim", 7, "not a multiple"), ("post_taps", 257, "ntaps must be"),
                           ("post_cutoff_hz", 100, "does not fit"), ("post_atten_db", 40, "atten_db")):
        with pytest.raises(ValueError, match=what):
            tp.topology_from_ini(_ini_with([dict(full, **{key: val})])[0])
