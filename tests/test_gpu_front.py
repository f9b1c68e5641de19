"""The half-band front stage on the device (sdrx_set_front, k_front_halfband): the frame behind it bit for bit
sdrreceiver_amd.front's, whatever the taps, the format, the arithmetic and the way the frame is handed over; the tree behind it
bit for bit a receiver without the stage that is fed the model's frame.

The cases, trees and frames are tests/front_ref.py's: six cases, three frames each -- a second tile, a short last tile
(1296 = 1024 + 272), the longest history (K = 31), 1, 2 and 3 stages, real and complex first stages, and one in front of the
resampler.  tests/test_front_model.py shows that nine wrong devices each change the output on these very inputs."""
import ctypes as C

import numpy as np
import pytest

import adc_ref as ar
import front_ref as fx
import resample_ref as rr
from helpers import bits
from oracle import binding as ob
from sdrreceiver_amd import _lib, front as fr, ingest, resample as rs, topology as tp
from sdrreceiver_amd.receiver import SPECTRUM_RAW, Receiver, SdrxError
from test_gpu_parity import _check_exact, _check_tolerance

pytestmark = pytest.mark.gpu

CASE = pytest.mark.parametrize("case", fx.CASES, ids=fx.IDS)


def _rx(case, taps, **kw):
    return Receiver.from_topology(fx.tree(case), **fx.receiver_kw(case, taps), **kw)


def _code(call):
    with pytest.raises(SdrxError) as e:
        call()
    return e.value.code


def _same(a, b):
    return np.array_equal(bits(np.ascontiguousarray(a)), bits(np.ascontiguousarray(b)))


def _launches(rx):
    return {k: v["launches"] for k, v in rx.kernel_times().items()}


def _device(frames):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(v).view(np.int16 if v.dtype == np.uint16 else v.dtype)).cuda() for v in frames]
    torch.cuda.synchronize()
    return out


class _Model:
    """The model behind one receiver of a case: the front stages' histories and, where the case has one, the resampler's"""

    def __init__(self, case, h):
        self.case, self.h, self.hists, self.rs_hist = case, h, None, None
        self.h_rs = rr.random_taps(case[6]) if case[6] else None

    def step(self, x):
        """(the front stage's output frame, the tree's raw frame) for the stage-1 input x"""
        y, self.hists = fr.run(x, self.h, self.case[1], bool(self.case[0]), self.hists)
        raw, self.rs_hist = fx.tree_frames(self.case, y, self.h_rs, self.rs_hist)
        return y, raw


def _check_frame(rx, case, y, raw, what):
    """The receiver's frames against the model's: the stage's output is the raw frame, or what the resampler read"""
    got = rx.raw()
    assert got.size == case[5]
    bad = np.flatnonzero(got.view(np.uint64) != raw.view(np.uint64))
    assert bad.size == 0, (what, "raw", bad.size, int(bad[0]))
    if case[6]:
        got = rx.resampler_input()
        bad = np.flatnonzero(got.view(np.uint64) != y.view(np.uint64))
        assert got.size == case[4] and bad.size == 0, (what, "resampler input", bad.size, int(bad[0]))


# ---- 1. indexing ----------------------------------------------------------------------------------------------------------------
@CASE
def test_impulse_prototypes_over_a_ramp(case):
    """h = one 1.0 at k = 0, C and N - 1: every output component is one input sample, its negation or 0, so a wrong index, tile,
    rotation or history shows as another sample of the ramp.  Real cases: int16 and 12-bit ramps."""
    real, stages, K, in_frame, n0, n, _ = case
    for fmt in (fx.formats(case) if real else (ingest.CS16,)):
        frames = fx.ramp_frames(case, fmt)
        for k in fx.impulse_positions(case):
            h = fx.impulse_taps(case, k)
            rx = _rx(case, h)
            info = rx.front
            assert (info["real_input"], info["stages"], info["K"], info["N"], info["in_frame"], info["out_frame"]) == (real, stages, K, 4 * K + 3, in_frame, n0)
            assert info["tw"] == 0 and info["alias_free"] == 0 and _same(info["taps"], h)
            m = _Model(case, h)
            for f, (v, _) in enumerate(frames):
                rx.process_fmt(v, fmt=fmt)
                _check_frame(rx, case, *m.step(fx.to_input(v, fmt)), (case, fmt, k, f))
            rx.close()


# ---- 2. arithmetic --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [0, 1, 2])
@CASE
def test_random_taps_and_full_range_samples(case, exact):
    """Full-mantissa asymmetric taps and full-range samples, the format alternating among those the context takes: the same bits
    in all three arithmetics (two roundings per tap, ascending k, no FMA)."""
    rx = _rx(case, fx.random_taps(case), exact=exact)
    h_rs, rs_hist = (rr.random_taps(case[6]) if case[6] else None), None
    for f, (v, fmt) in enumerate(fx.arithmetic_frames(case, first=exact)):
        rx.process_fmt(v, fmt=fmt)
        y = fx.model_run(case, first=exact)[f]
        raw, rs_hist = fx.tree_frames(case, y, h_rs, rs_hist)
        _check_frame(rx, case, y, raw, (case, exact, f))
    rx.close()


# ---- 3. DC removal in front of a complex stage; the built-in design -------------------------------------------------------------
@pytest.mark.parametrize("speculative", [True, False])
@pytest.mark.parametrize("case", fx.CASES[2:4], ids=fx.IDS[2:4])
def test_dc_removal_then_the_builtin_design(case, speculative):
    real, stages, K, in_frame, n0, n, _ = case
    rx = _rx(case, K, front_atten_db=80.0, dc_speculative=speculative)
    info = rx.front
    want_taps, want_info = fr.design(K, 80.0)
    assert _same(info["taps"], want_taps) and info["tw"] == want_info["tw"] and info["alias_free"] == want_info["alias_free"]
    m = _Model(case, info["taps"])
    state = np.zeros(2, np.float32)
    for f in range(fx.N_FRAMES):
        fmt = fx.COMPLEX_FORMATS[f % 3]
        v = rr.full_range(fmt, in_frame, 300 + f)
        v[1::2] = v[1::2] // 4 + (60 if fmt != ingest.CS16 else 60 << 8)  # a DC offset worth removing
        rx.process_fmt(v, correct_dc=True)
        iq = ingest.to_float(v)
        ob.dc_correct(iq, state)
        _check_frame(rx, case, *m.step(iq.view(np.complex64)), (case, f))
    rx.close()


def test_builtin_design_on_a_real_context_in_front_of_the_resampler():
    case = fx.CASES[5]
    rx = _rx(case, case[2], front_atten_db=60.0)
    info = rx.front
    assert _same(info["taps"], fr.design(case[2], 60.0)[0]) and info["alias_free"] == 1.0 - 2.0 * info["tw"] > 0.5
    assert rx.resampler["in_frame"] == case[4] == info["out_frame"] and rx.resampler["out_frame"] == case[5]
    m = _Model(case, info["taps"])
    for f, (v, fmt) in enumerate(fx.arithmetic_frames(case)):
        rx.process_fmt(v, fmt=fmt)
        _check_frame(rx, case, *m.step(fx.to_input(v, fmt)), (case, f))
    rx.close()


# ---- 4. the tree behind it: a twin without the stage, fed the model's frame ----------------------------------------------------------
@pytest.mark.parametrize("exact", [1, 0, 2])
@CASE
def test_twin_receiver_fed_the_models_frame(case, exact):
    """Five frames: the raw spectrum updates with the fifth (sdrj's every-4th-call cadence).  The built-in designs, front stage
    and resampler: unit gain, so the tree sees samples of the range its tolerance arithmetic is held to the oracle for."""
    topo = fx.tree(case)
    leaves = [i for i in range(len(topo.vfos)) if not topo.children(i)]
    kw = dict(exact=exact, meter=True, watch=True, keep_streams=True, keep_prequant=exact != 1)
    fkw = fx.receiver_kw(case, case[2])
    if case[6]:
        fkw["resample_taps"] = case[6][2]
    rx, twin = Receiver.from_topology(topo, front_atten_db=60.0, **fkw, **kw), Receiver.from_topology(topo, **kw)
    nodes, roots = ob.build_tree("port", topo)
    for r in (rx, twin):
        r.set_watch([3], [1])  # the parent-less leaf: its source is the raw frame
        r.set_spectrum(SPECTRUM_RAW)
    m = _Model(case, rx.front["taps"])
    if case[6]:
        m.h_rs = rx.resampler["taps"]
    F = fx.formats(case)
    for f in range(5):
        fmt = F[(f + exact) % len(F)]
        v = fx.full_range(fmt, case[3], 500 + 10 * exact + f)
        _, y = m.step(fx.to_input(v, fmt))
        rx.process_fmt(v, fmt=fmt)
        twin.process(y.view(np.float32))
        ob.process_roots(roots, y.view(np.float32))
        assert _same(rx.raw(), y) and _same(twin.raw(), y), (case, f)
        assert rx.published == twin.published and len(rx.published) == len(leaves), (case, f)
        for i in range(len(topo.vfos)):
            assert _same(rx.stream(i), twin.stream(i)), (case, f, i, "stream")
        for i in leaves:
            assert np.array_equal(rx.output(i), twin.output(i)), (case, f, i, "payload")
        for a, b in ((rx.meters(leaves), twin.meters(leaves)), (rx.watch([3]), twin.watch([3])), (rx.spectrum(SPECTRUM_RAW), twin.spectrum(SPECTRUM_RAW))):
            assert a.keys() == b.keys()
            for key in a:
                assert _same(np.atleast_1d(a[key]), np.atleast_1d(b[key])), (case, f, key)
        pa, pb = rx.watch_psd(3), twin.watch_psd(3)
        assert pa[1] == pb[1] and _same(pa[0], pb[0]) and pa[0].any(), (case, f, "watch psd")
        (_check_exact if exact == 1 else _check_tolerance)(rx, nodes, topo, (case, exact, f))
    assert rx.spectrum(SPECTRUM_RAW)["updates"] == twin.spectrum(SPECTRUM_RAW)["updates"] >= 1
    rx.close()
    twin.close()


# ---- 5. launch forms ------------------------------------------------------------------------------------------------------------
@CASE
def test_every_launch_form_gives_the_same_bits(case):
    real, stages, K, in_frame, n0, n, _ = case
    h = fx.random_taps(case, seed=5)
    fmt = ingest.RU12 if real else ingest.CS16
    frames = [fx.full_range(fmt, in_frame, 700 + f) for f in range(fx.N_FRAMES)]
    ref = _rx(case, h)
    want = []
    for v in frames:
        ref.process_fmt(v, fmt=fmt)
        want.append((list(ref.published), ref.raw()))
    ref.close()
    assert all(len(m) == 3 for m, _ in want)

    rx = _rx(case, h)  # submit_fmt, two frames in flight
    rx.submit_fmt(frames[0], fmt=fmt)
    rx.submit_fmt(frames[1], fmt=fmt)
    rx.wait()
    assert rx.published == want[0][0]
    rx.submit_fmt(frames[2], fmt=fmt)
    rx.wait()
    assert rx.published == want[1][0]
    rx.wait()
    assert rx.published == want[2][0] and _same(rx.raw(), want[2][1])
    rx.close()

    dev = _device(frames)  # process_device_fmt queued back to back, then fetch
    rx = _rx(case, h)
    for k in range(fx.N_FRAMES):
        rx.process_device_fmt(dev[k].data_ptr(), in_frame, fmt)
    rx.fetch()
    assert rx.published == want[2][0] and _same(rx.raw(), want[2][1])
    rx.close()

    rx = _rx(case, h)  # submit_device_fmt
    rx.submit_device_fmt(dev[0].data_ptr(), in_frame, fmt)
    rx.submit_device_fmt(dev[1].data_ptr(), in_frame, fmt)
    rx.wait()
    assert rx.published == want[0][0]
    rx.wait()
    assert rx.published == want[1][0] and _same(rx.raw(), want[1][1])
    rx.close()
    if real:
        return

    floats = [ingest.to_float(v) for v in frames]  # the same values as cf32
    rx = _rx(case, h)
    for k, iq in enumerate(floats):
        rx.process(iq)
        assert rx.published == want[k][0] and _same(rx.raw(), want[k][1]), (case, k, "process")
    rx.close()

    fdev = _device(floats)
    rx = _rx(case, h)
    for k in range(fx.N_FRAMES):
        rx.process_device(fdev[k].data_ptr(), in_frame)
        rx.fetch()
        assert rx.published == want[k][0] and _same(rx.raw(), want[k][1]), (case, k, "process_device")
    rx.close()

    rx = _rx(case, h)  # submit (cf32) and submit_device
    rx.submit(floats[0])
    rx.submit_device(fdev[1].data_ptr(), in_frame)
    rx.wait()
    assert rx.published == want[0][0]
    rx.wait()
    assert rx.published == want[1][0] and _same(rx.raw(), want[1][1])
    rx.close()


# ---- 6. the ADC meter sees the frame as it arrived: a real frame as pairs ------------------------------------------------------------
@CASE
def test_adc_meter_counts_the_input_frame(case):
    real, in_frame = case[0], case[3]
    rx = _rx(case, fx.random_taps(case), adc_meter=True)
    for f, (v, fmt) in enumerate(fx.arithmetic_frames(case)):
        if real:  # both rails, and a run of them across the pair view's arms
            v = v.copy()
            lo, hi = (np.int16(-32768), np.int16(32767)) if fmt == ingest.RS16 else (np.uint16(0xA000), np.uint16(0x5FFF))
            v[[0, 3]], v[[1, 2]], v[200:209] = lo, hi, hi
        rx.process_fmt(v, fmt=fmt, correct_dc=bool(f & 1) and not real)
        got, want = rx.adc_meter(), (fx.adc_pair_model if real else ar.model)(v, fmt, frame=f)
        if fmt == ingest.RS16:  # the same memory as CS16 pairs: adc_ref's model, but for the format's name
            assert want == dict(ar.model(v, ingest.CS16, frame=f), fmt=fmt)
        assert want["n_complex"] == (in_frame // 2 if real else in_frame) and want["fmt"] == fmt
        assert got == want, (case, f, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        if real:
            assert got["i"]["at_hi"] >= 5 and got["q"]["at_hi"] >= 5 and got["i"]["longest_rail_run"] >= 4
            lv = ingest.adc_levels(got)
            assert lv["peak"] == 128.0 and lv["longest_rail_run_is_lower_bound"] and lv["longest_rail_run"] >= 5
    rx.close()


# ---- 7. off means off; what it holds; the error codes -------------------------------------------------------------------------------
def _watching(topo, **kw):
    rx = Receiver(watch=True, meter=True, **kw)
    for d in topo.vfos:
        rx.add_vfo(d)
    return rx


def test_off_means_off():
    case = fx.CASES[0]
    n = case[5]
    topo = fx.tree(case)
    leaves = [i for i in range(len(topo.vfos)) if not topo.children(i)]
    h = fx.random_taps(case)
    never = _watching(topo)
    off = _watching(topo)  # set, and switched off again
    off._chk(off.L.sdrx_set_front(off.h, 1, 1, h.ctypes.data, case[2], 0.0))
    off._chk(off.L.sdrx_set_front(off.h, 0, 0, None, 0, 0.0))
    assert off.L.sdrx_get_front(off.h, C.byref(_lib.FrontInfoC()), None, 0) == _lib.SDRX_ESTATE
    for rx in (never, off):
        rx.finalize()
        rx.set_watch([3], [1])
        rx.set_spectrum(SPECTRUM_RAW)
        rx.enable_kernel_timing(True)
    assert off.stats()["device_bytes"] == never.stats()["device_bytes"]
    for f in range(5):
        v = rr.full_range(fx.COMPLEX_FORMATS[f % 3], n, 900 + f)
        for rx in (never, off):
            rx.process_fmt(v, correct_dc=f == 3)
        assert off.published == never.published and len(off.published) == len(leaves)
        assert _same(off.raw(), never.raw())
        for a, b in ((off.meters(leaves), never.meters(leaves)), (off.watch([3]), never.watch([3])), (off.spectrum(SPECTRUM_RAW), never.spectrum(SPECTRUM_RAW))):
            for key in b:
                assert _same(np.atleast_1d(a[key]), np.atleast_1d(b[key])), (f, key)
    assert off.stats()["device_bytes"] == never.stats()["device_bytes"]
    assert _launches(off) == _launches(never)
    # ... and the real formats stay refused without a real front stage
    assert _code(lambda: off.process_fmt(fx.full_range(ingest.RS16, n, 1), fmt=ingest.RS16)) == _lib.SDRX_EINVAL
    for rx in (never, off):
        rx.close()


@CASE
def test_device_bytes_formula(case):
    """What the stage holds: the cf32 input frame of every complex stage in whole tiles plus one, both parities
    of every stage's history (128 cf32 each), and the 2 K + 3 non-zero taps."""
    real, stages, K, in_frame, n0, n, _ = case
    topo = fx.tree(case)
    kw = fx.receiver_kw(case, fx.random_taps(case))
    base_kw = {k: v for k, v in kw.items() if not k.startswith("front_")}
    base, on = Receiver.from_topology(topo, **base_kw), Receiver.from_topology(topo, **kw)
    grown = on.stats()["device_bytes"] - base.stats()["device_bytes"]
    want = sum(8 * (-(-n_in // 1024) * 1024 + 1024) for s, (n_in, _) in enumerate(fr.frames(n0, stages), 1) if s >= (2 if real else 1))
    want += 8 * 2 * 128 * stages + 4 * (2 * K + 3)
    assert grown == want, (grown, want)
    # one more launch per stage inside the ingest bracket: the kinds and the bracket count are the twin's
    for rx, count in ((base, n0), (on, in_frame)):
        rx.enable_kernel_timing(True)
        fmt = ingest.RS16 if real and rx is on else ingest.CS16
        rx.process_fmt(fx.full_range(fmt, count, 5), fmt=fmt)
    a, b = _launches(base), _launches(on)
    assert a == b and a["k_ingest"] == 1, (a, b)
    base.close()
    on.close()


def test_error_codes():
    case = fx.CASES[0]  # real, one stage, K = 2
    real, stages, K, in_frame, n0, n, _ = case
    topo = fx.tree(case)
    h = fx.random_taps(case)
    lib = _lib.lib()
    # before the first parent-less VFO, bad arguments, after finalize
    rx = Receiver()
    assert lib.sdrx_set_front(rx.h, 1, 1, h.ctypes.data, K, 0.0) == _lib.SDRX_ESTATE
    rx.add_vfo(topo.vfos[0])
    for args in ((2, 1, K), (-1, 1, K), (1, 4, K), (1, -1, K), (1, 1, 1), (1, 1, 32)):
        assert lib.sdrx_set_front(rx.h, args[0], args[1], np.zeros(127, np.float32).ctypes.data, args[2], 0.0) == _lib.SDRX_EINVAL, args
    for k, val in ((1, 1e-30), (3, -0.0), (4 * K + 1, 1.0)):  # an odd tap that is not +0.0f
        bad = h.copy()
        bad[k] = val
        assert lib.sdrx_set_front(rx.h, 1, 1, bad.ctypes.data, K, 0.0) == _lib.SDRX_EINVAL, k
    assert lib.sdrx_set_front(rx.h, 1, 1, None, 7, 50.0) == _lib.SDRX_EINVAL
    assert lib.sdrx_set_front(rx.h, 1, 1, None, 2, 80.0) == _lib.SDRX_EFILTER and b"wider than the band" in lib.sdrx_last_error(rx.h)
    assert lib.sdrx_get_front(rx.h, C.byref(_lib.FrontInfoC()), None, 0) == _lib.SDRX_ESTATE
    assert lib.sdrx_set_front(rx.h, 1, 1, None, 2, 60.0) == 0  # the atten_db argument is the design's
    info = _lib.FrontInfoC()
    assert lib.sdrx_get_front(rx.h, C.byref(info), None, 0) == 0 and (info.in_frame, info.out_frame, info.N) == (0, 0, 11)
    rx.close()
    rx = _rx(case, h)
    assert lib.sdrx_set_front(rx.h, 1, 1, h.ctypes.data, K, 0.0) == _lib.SDRX_ESTATE
    assert lib.sdrx_set_front(rx.h, 0, 0, None, 0, 0.0) == _lib.SDRX_ESTATE
    assert lib.sdrx_get_front(rx.h, None, None, 0) == _lib.SDRX_EINVAL
    # a real context: another count, a complex format, bytes, floats, DC removal -- through every door
    good = fx.full_range(ingest.RS16, in_frame, 1)
    for fmt in fx.REAL_FORMATS:
        for count in (n0, in_frame // 2 * 3, in_frame + 4):
            bad = fx.full_range(fmt, count, 2)
            assert _code(lambda: rx.process_fmt(bad, fmt=fmt)) == _lib.SDRX_EINVAL
            assert _code(lambda: rx.submit_fmt(bad, fmt=fmt)) == _lib.SDRX_EINVAL
        ok = fx.full_range(fmt, in_frame, 3)
        assert _code(lambda: rx.process_fmt(ok, fmt=fmt, correct_dc=True)) == _lib.SDRX_EINVAL
        assert _code(lambda: rx.submit_fmt(ok, fmt=fmt, correct_dc=True)) == _lib.SDRX_EINVAL
    for fmt in fx.COMPLEX_FORMATS:
        for count in (in_frame, in_frame // 2):
            bad = rr.full_range(fmt, count, 4)
            assert _code(lambda: rx.process_fmt(bad)) == _lib.SDRX_EINVAL and _code(lambda: rx.submit_fmt(bad)) == _lib.SDRX_EINVAL
    bytes_ = rr.full_range(ingest.CU8, in_frame, 5)
    assert _code(lambda: rx.process_u8(bytes_)) == _lib.SDRX_EINVAL and _code(lambda: rx.submit_u8(bytes_)) == _lib.SDRX_EINVAL
    floats = np.zeros(2 * in_frame, np.float32)
    assert _code(lambda: rx.process(floats)) == _lib.SDRX_EINVAL and _code(lambda: rx.submit(floats)) == _lib.SDRX_EINVAL
    dev = _device([floats, good])
    assert _code(lambda: rx.process_device(dev[0].data_ptr(), in_frame)) == _lib.SDRX_EINVAL
    assert _code(lambda: rx.submit_device(dev[0].data_ptr(), in_frame)) == _lib.SDRX_EINVAL
    assert _code(lambda: rx.process_device_fmt(dev[1].data_ptr(), in_frame, ingest.CS16)) == _lib.SDRX_EINVAL
    assert _code(lambda: rx.process_device_fmt(dev[1].data_ptr(), n0, ingest.RS16)) == _lib.SDRX_EINVAL
    assert _code(lambda: rx.submit_device_fmt(dev[1].data_ptr(), in_frame, ingest.RS16, correct_dc=True)) == _lib.SDRX_EINVAL
    assert _code(lambda: rx.process_device_fmt(dev[1].data_ptr(), in_frame, 5)) == _lib.SDRX_EINVAL
    assert rx.in_flight() == 0
    rx.process_fmt(good, fmt=ingest.RS16)  # ... and nothing of that was queued
    want, _ = fr.apply(fx.to_input(good, ingest.RS16), h, True)
    assert _same(rx.raw(), want)
    # shared frames: neither as the reader nor as the source
    plain = Receiver.from_topology(topo)
    tree_floats = np.zeros(2 * n, np.float32)
    plain.process(tree_floats)
    assert _code(lambda: rx.process_shared(plain)) == _lib.SDRX_ESTATE and _code(lambda: plain.process_shared(rx)) == _lib.SDRX_ESTATE
    assert _code(lambda: rx.submit_shared(plain)) == _lib.SDRX_ESTATE and _code(lambda: plain.submit_shared(rx)) == _lib.SDRX_ESTATE
    assert _code(lambda: plain.process_if_same(rx, tree_floats)) == _lib.SDRX_ESTATE and _code(lambda: rx.submit_if_same(plain, tree_floats)) == _lib.SDRX_ESTATE
    plain.close()
    rx.close()
    # a complex context: the real formats, and the tree's own frame length
    case = fx.CASES[2]
    rx = _rx(case, fx.random_taps(case))
    for fmt in fx.REAL_FORMATS:
        bad = fx.full_range(fmt, case[3], 6)
        assert _code(lambda: rx.process_fmt(bad, fmt=fmt)) == _lib.SDRX_EINVAL and _code(lambda: rx.submit_fmt(bad, fmt=fmt)) == _lib.SDRX_EINVAL
    short = rr.full_range(ingest.CS16, case[4], 7)
    assert _code(lambda: rx.process_fmt(short)) == _lib.SDRX_EINVAL
    assert _code(lambda: rx.process(np.zeros(2 * case[4], np.float32))) == _lib.SDRX_EINVAL
    rx.process(np.zeros(2 * case[3], np.float32))
    assert not rx.raw().any()
    plain = Receiver.from_topology(fx.tree(case))
    plain.process(np.zeros(2 * case[5], np.float32))
    assert _code(lambda: rx.process_shared(plain)) == _lib.SDRX_ESTATE and _code(lambda: plain.submit_shared(rx)) == _lib.SDRX_ESTATE
    plain.close()
    rx.close()


def test_finalize_refuses_roots_of_two_rates():
    case = fx.CASES[2]
    n = case[5]
    topo = fx.tree(case)
    rx = Receiver()
    for d in topo.vfos[:3]:
        rx.add_vfo(d)
    rx.add_vfo(tp.VfoDesc(topic="RAW03", parent=-1, fs=8 * n, decimate_count=0, mixer_freq=1.0, demod_usb=False, cstyle=0, samples_per_buffer=n))
    h = fx.random_taps(case)
    rx._chk(rx.L.sdrx_set_front(rx.h, 0, 1, h.ctypes.data, case[2], 0.0))
    assert rx.L.sdrx_finalize(rx.h) == _lib.SDRX_EUNSUPPORTED and b"share one fs" in rx.L.sdrx_last_error(rx.h)
    rx.close()


def test_set_front_before_or_after_set_resampler():
    case = fx.CASES[5]
    topo = fx.tree(case)
    h, h_rs = fx.random_taps(case), rr.random_taps(case[6])
    fs_in, T = rr.rates(case[6])[0], case[6][2]
    out = []
    for front_first in (True, False):
        rx = Receiver()
        for d in topo.vfos:
            rx.add_vfo(d)
        calls = [lambda: rx.L.sdrx_set_front(rx.h, 1, 1, h.ctypes.data, case[2], 0.0), lambda: rx.L.sdrx_set_resampler(rx.h, fs_in, h_rs.ctypes.data, T)]
        for call in (calls if front_first else calls[::-1]):
            rx._chk(call())
        rx.finalize()
        info = _lib.FrontInfoC()
        rx._chk(rx.L.sdrx_get_front(rx.h, C.byref(info), None, 0))
        assert (info.in_frame, info.out_frame) == (case[3], case[4])
        v, fmt = fx.arithmetic_frames(case)[0]
        rx._chk(rx.L.sdrx_process_fmt(rx.h, v.ctypes.data, v.size, fmt, 0))
        out.append(rx.raw())
        rx.close()
    y, _ = fr.apply(fx.to_input(*fx.arithmetic_frames(case)[0]), h, True)
    want, _ = rs.apply(y, h_rs, case[6][0], case[6][1])
    assert _same(out[0], want) and _same(out[1], want)


# ---- the C++ host layer: sdrj::setFront behind sdrx_demo --front-stages ---------------------------------------------------------
def test_demo_takes_real_frames(tmp_path):
    import os
    import subprocess
    from test_topology import INI_25E_LIKE
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    demo = os.path.join(root, "host", "sdrx_demo")
    subprocess.check_call(["make", "-C", os.path.join(root, "host")], stdout=subprocess.DEVNULL)
    profile = tmp_path / "profile.ini"
    profile.write_text(INI_25E_LIKE)
    plain = subprocess.check_output([demo, str(profile), "--frames", "2", "--format", "cs16"], text=True).splitlines()
    for extra, real in ((["--format", "rs16", "--front-real"], 1), (["--format", "ru12", "--front-real"], 1), (["--format", "cs16"], 0)):
        lines = subprocess.check_output([demo, str(profile), "--frames", "2", "--front-stages", "2", "--front-taps", "7"] + extra, text=True).splitlines()
        head = lines[0].split()
        n = int(head[6])
        assert head[:7] == ["front", str(real), "2", "7", "31", str(4 * n), str(n)], head
        want = fr.design(7, 80.0)[1]
        assert float(head[7]) == pytest.approx(want["tw"], rel=1e-6) and float(head[8]) == pytest.approx(want["alias_free"], rel=1e-6)
        # the same messages in the same order (frame, topic, rate, bytes), other payloads: the frames are other samples
        assert [ln.split()[:4] for ln in lines[1:]] == [ln.split()[:4] for ln in plain] and len(plain) > 0
