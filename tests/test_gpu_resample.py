"""The rational resampler on the device (sdrx_set_resampler, k_resample): the tree's raw frame bit for bit
sdrreceiver_amd.resample.apply's, whatever the taps, the format, the arithmetic and the way the frame is handed over; the tree
behind it bit for bit a receiver without the resampler that is fed the model's frame.

The ratios, trees and frames are tests/resample_ref.py's: five ratios, three frames each, the smallest frames that have more
than one output chunk, a short last chunk (1296 = 1024 + 272), up- and downsampling, and T = 16, 24, 32.
tests/test_resample_model.py shows that eight wrong devices each change the output on these very inputs."""
import ctypes as C

import numpy as np
import pytest

import adc_ref as ar
import resample_ref as rr
from helpers import bits
from oracle import binding as ob
from sdrreceiver_amd import _lib, ingest, resample as rs, topology as tp
from sdrreceiver_amd.receiver import SPECTRUM_RAW, Receiver, SdrxError
from test_gpu_parity import _check_exact, _check_tolerance

pytestmark = pytest.mark.gpu

CASE = pytest.mark.parametrize("case", rr.CASES, ids=rr.IDS)


def _rx(case, taps, **kw):
    return Receiver.from_topology(rr.tree(case), input_rate=rr.rates(case)[0], resample_taps=taps, **kw)


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
    out = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in frames]
    torch.cuda.synchronize()
    return out


# ---- 1. indexing ----------------------------------------------------------------------------------------------------------------
@CASE
def test_impulse_prototypes_over_a_ramp(case):
    """h = one 1.0 at k = 0, L-1, L, L T - 1 and in the middle: every output is one input sample (or 0), so a wrong index, phase
    or history shows as another sample of the ramp."""
    L, M, T, n_in, n = case
    frames = rr.ramp_frames(case)
    for k in rr.impulse_positions(case):
        h = rr.impulse_taps(case, k)
        rx = _rx(case, h)
        info = rx.resampler
        assert (info["L"], info["M"], info["taps_per_phase"], info["in_frame"], info["out_frame"]) == (L, M, T, n_in, n)
        assert info["fs_in"] == 4 * n_in and info["fs_out"] == 4 * n and info["delay_out_samples"] == (L * T - 1) / (2.0 * M)
        assert info["passband_hz"] == 0 and _same(info["taps"], h)
        hist = None
        for f, v in enumerate(frames):
            rx.process_fmt(v)
            want, hist = rs.apply(rr.to_complex(v), h, L, M, hist)
            got = rx.raw()
            assert got.size == n and _same(got, want), (case, k, f, int(np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[0]))
            assert _same(rx.resampler_input(), rr.to_complex(v)), (case, k, f)
        rx.close()


# ---- 2. arithmetic --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [0, 1, 2])
@CASE
def test_random_taps_and_full_range_samples(case, exact):
    """Full-mantissa taps and full-range CU8, CS8 and CS16 samples, the format alternating: the same bits in all three
    arithmetics (two roundings per tap, ascending t, no FMA)."""
    rx = _rx(case, rr.random_taps(case), exact=exact)
    for f, v in enumerate(rr.arithmetic_frames(case, first=exact)):
        rx.process_fmt(v)
        got, want = rx.raw(), rr.model_run(case, first=exact)[f]
        bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
        assert bad.size == 0, (case, exact, f, bad.size, int(bad[0]))
    rx.close()


# ---- 3. DC removal in front, the built-in design ----------------------------------------------------------------------------------
@pytest.mark.parametrize("speculative", [True, False])
@CASE
def test_dc_removal_then_the_builtin_design(case, speculative):
    L, M, T, n_in, n = case
    fs_in, fs_out = rr.rates(case)
    rx = _rx(case, T, resample_atten_db=80.0, dc_speculative=speculative)
    info = rx.resampler
    want_taps, want_info = rs.design(fs_in, fs_out, T, 80.0)
    h = info["taps"]
    d = np.abs(h.astype(np.float64) - want_taps.astype(np.float64))
    assert (d <= np.spacing(np.abs(want_taps)).astype(np.float64) + 2.0 ** -40 * float(np.abs(want_taps).max())).all()
    assert info["passband_hz"] == pytest.approx(want_info["passband_hz"], rel=1e-12)
    state, hist = np.zeros(2, np.float32), None
    for f in range(rr.N_FRAMES):
        fmt = rr.FORMATS[f % 3]
        v = rr.full_range(fmt, n_in, 300 + f)
        v[1::2] = v[1::2] // 4 + (60 if fmt != ingest.CS16 else 60 << 8)  # a DC offset worth removing
        rx.process_fmt(v, correct_dc=True)
        iq = ingest.to_float(v)
        ob.dc_correct(iq, state)
        assert _same(rx.resampler_input(), iq.view(np.complex64)), (case, f, "input")
        want, hist = rs.apply(iq.view(np.complex64), h, L, M, hist)
        assert _same(rx.raw(), want), (case, f, "raw")
    rx.close()


# ---- 4. the tree behind it: a twin without the resampler, fed the model's frame ----------------------------------------------------
@pytest.mark.parametrize("exact", [1, 0, 2])
@CASE
def test_twin_receiver_fed_the_models_frame(case, exact):
    """Five frames: the raw spectrum updates with the fifth (sdrj's every-4th-call cadence)."""
    L, M, T, n_in, n = case
    topo = rr.tree(case)
    leaves = [i for i in range(len(topo.vfos)) if not topo.children(i)]
    kw = dict(exact=exact, meter=True, watch=True, keep_streams=True, keep_prequant=exact != 1)
    rx, twin = _rx(case, T, **kw), Receiver.from_topology(topo, **kw)
    h = rx.resampler["taps"]
    nodes, roots = ob.build_tree("port", topo)
    for r in (rx, twin):
        r.set_watch([3], [1])  # the parent-less leaf: its source is the raw frame
        r.set_spectrum(SPECTRUM_RAW)
    hist = None
    for f in range(5):
        v = rr.full_range(rr.FORMATS[(f + exact) % 3], n_in, 500 + 10 * exact + f)
        y, hist = rs.apply(rr.to_complex(v), h, L, M, hist)
        rx.process_fmt(v)
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
    L, M, T, n_in, n = case
    h = rr.random_taps(case, seed=5)
    frames = [rr.full_range(ingest.CS16, n_in, 700 + f) for f in range(rr.N_FRAMES)]
    ref = _rx(case, h)
    want = []
    for v in frames:
        ref.process_fmt(v)
        want.append((list(ref.published), ref.raw()))
    ref.close()
    assert all(len(m) == 3 for m, _ in want)

    rx = _rx(case, h)  # submit_fmt, two frames in flight
    rx.submit_fmt(frames[0])
    rx.submit_fmt(frames[1])
    rx.wait()
    assert rx.published == want[0][0]
    rx.submit_fmt(frames[2])
    rx.wait()
    assert rx.published == want[1][0]
    rx.wait()
    assert rx.published == want[2][0] and _same(rx.raw(), want[2][1]) and _same(rx.resampler_input(), rr.to_complex(frames[2]))
    rx.close()

    dev = _device(frames)  # process_device_fmt queued back to back, then fetch
    rx = _rx(case, h)
    for k in range(rr.N_FRAMES):
        rx.process_device_fmt(dev[k].data_ptr(), n_in, ingest.CS16)
    rx.fetch()
    assert rx.published == want[2][0] and _same(rx.raw(), want[2][1])
    rx.close()

    floats = [ingest.to_float(v) for v in frames]  # the same values as cf32
    rx = _rx(case, h)
    for k, iq in enumerate(floats):
        rx.process(iq)
        assert rx.published == want[k][0] and _same(rx.raw(), want[k][1]), (case, k, "process")
    rx.close()

    fdev = _device(floats)
    rx = _rx(case, h)
    for k in range(rr.N_FRAMES):
        rx.process_device(fdev[k].data_ptr(), n_in)
        rx.fetch()
        assert rx.published == want[k][0] and _same(rx.raw(), want[k][1]), (case, k, "process_device")
    rx.close()

    rx = _rx(case, h)  # submit (cf32) and submit_device
    rx.submit(floats[0])
    rx.submit_device(fdev[1].data_ptr(), n_in)
    rx.wait()
    assert rx.published == want[0][0]
    rx.wait()
    assert rx.published == want[1][0] and _same(rx.raw(), want[1][1])
    rx.close()


# ---- 6. the ADC meter sees the frame as it arrived ----------------------------------------------------------------------------------
@CASE
def test_adc_meter_counts_the_input_frame(case):
    rx = _rx(case, rr.random_taps(case), adc_meter=True)
    for f, v in enumerate(rr.arithmetic_frames(case)):
        rx.process_fmt(v, correct_dc=bool(f & 1))
        fmt = ingest.infer_format(v)
        got, want = rx.adc_meter(), ar.model(v, fmt, frame=f)
        assert want["n_complex"] == case[3] and got == want, (case, f, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
    rx.close()


# ---- 7. off means off; what it holds; the error codes -------------------------------------------------------------------------------
def _watching(topo, **kw):
    rx = Receiver(watch=True, meter=True, **kw)
    for d in topo.vfos:
        rx.add_vfo(d)
    return rx


def _started(rx):
    rx.finalize()
    rx.set_watch([3], [1])
    rx.set_spectrum(SPECTRUM_RAW)
    rx.enable_kernel_timing(True)
    return rx


def test_off_means_off():
    case = rr.CASES[2]
    L, M, T, n_in, n = case
    topo = rr.tree(case)
    leaves = [i for i in range(len(topo.vfos)) if not topo.children(i)]
    h = rr.random_taps(case)
    never = _watching(topo)
    off = _watching(topo)  # set, and switched off again
    off._chk(off.L.sdrx_set_resampler(off.h, 4 * n_in, h.ctypes.data, T))
    off._chk(off.L.sdrx_set_resampler(off.h, 0, None, 0))
    assert off.L.sdrx_get_resampler(off.h, C.byref(_lib.ResamplerInfoC()), None, 0) == _lib.SDRX_ESTATE
    on = _watching(topo, input_rate=4 * n_in, resample_taps=h)
    for rx in (never, off, on):
        rx.finalize()
    base = never.stats()["device_bytes"]
    assert off.stats()["device_bytes"] == base
    # what it holds: the input-rate frame in whole tiles plus one, the history of both parities (64 cf32 each), the taps
    grown = on.stats()["device_bytes"] - base
    assert grown == 8 * (-(-n_in // 1024) * 1024 + 1024) + 8 * 2 * 64 + 4 * L * T, grown
    for rx in (never, off):
        rx.set_watch([3], [1])
        rx.set_spectrum(SPECTRUM_RAW)
        rx.enable_kernel_timing(True)
    for f in range(5):
        v = rr.full_range(rr.FORMATS[f % 3], n, 900 + f)
        for rx in (never, off):
            rx.process_fmt(v, correct_dc=f == 3)
        assert off.published == never.published and len(off.published) == len(leaves)
        assert _same(off.raw(), never.raw())
        for a, b in ((off.meters(leaves), never.meters(leaves)), (off.watch([3]), never.watch([3])), (off.spectrum(SPECTRUM_RAW), never.spectrum(SPECTRUM_RAW))):
            for key in b:
                assert _same(np.atleast_1d(a[key]), np.atleast_1d(b[key])), (f, key)
    assert off.stats()["device_bytes"] == never.stats()["device_bytes"]
    assert _launches(off) == _launches(never)
    buf = np.zeros(2 * n, np.float32)
    assert off.L.sdrx_get_resampler_input(off.h, buf.ctypes.data, n) == _lib.SDRX_ESTATE
    for rx in (never, off, on):
        rx.close()


def test_error_codes():
    case = rr.CASES[2]
    L, M, T, n_in, n = case
    topo = rr.tree(case)
    h = rr.random_taps(case)
    lib = _lib.lib()
    # before the first parent-less VFO, bad arguments, after finalize
    rx = Receiver()
    assert lib.sdrx_set_resampler(rx.h, 4 * n_in, h.ctypes.data, T) == _lib.SDRX_ESTATE
    rx.add_vfo(topo.vfos[0])
    assert lib.sdrx_set_resampler(rx.h, -1, h.ctypes.data, T) == _lib.SDRX_EINVAL
    assert lib.sdrx_set_resampler(rx.h, 4 * n_in, None, T) == _lib.SDRX_EINVAL
    assert lib.sdrx_set_resampler(rx.h, 4 * n_in, h.ctypes.data, 0) == _lib.SDRX_EINVAL
    assert lib.sdrx_get_resampler(rx.h, C.byref(_lib.ResamplerInfoC()), None, 0) == _lib.SDRX_ESTATE
    rx.close()
    rx = _rx(case, h)
    assert lib.sdrx_set_resampler(rx.h, 4 * n_in, h.ctypes.data, T) == _lib.SDRX_ESTATE
    assert lib.sdrx_set_resampler(rx.h, 0, None, 0) == _lib.SDRX_ESTATE
    assert lib.sdrx_get_resampler(rx.h, None, None, 0) == _lib.SDRX_EINVAL
    assert _code(rx.resampler_input) == _lib.SDRX_ESTATE  # no frame yet
    # a frame of out_frame samples, through every door
    good = rr.full_range(ingest.CS16, n_in, 1)
    for fmt in rr.FORMATS:
        bad = rr.full_range(fmt, n, 2)
        assert _code(lambda: rx.process_fmt(bad)) == _lib.SDRX_EINVAL
        assert _code(lambda: rx.submit_fmt(bad, correct_dc=True)) == _lib.SDRX_EINVAL
    bytes_ = rr.full_range(ingest.CU8, n, 3)
    assert _code(lambda: rx.process_u8(bytes_)) == _lib.SDRX_EINVAL and _code(lambda: rx.submit_u8(bytes_)) == _lib.SDRX_EINVAL
    floats = np.zeros(2 * n, np.float32)
    assert _code(lambda: rx.process(floats)) == _lib.SDRX_EINVAL and _code(lambda: rx.submit(floats)) == _lib.SDRX_EINVAL
    dev = _device([floats, good])
    assert _code(lambda: rx.process_device(dev[0].data_ptr(), n)) == _lib.SDRX_EINVAL
    assert _code(lambda: rx.submit_device(dev[0].data_ptr(), n)) == _lib.SDRX_EINVAL
    assert _code(lambda: rx.process_device_fmt(dev[1].data_ptr(), n, ingest.CS16)) == _lib.SDRX_EINVAL
    assert _code(lambda: rx.submit_device_fmt(dev[1].data_ptr(), n, ingest.CS16)) == _lib.SDRX_EINVAL
    assert rx.in_flight() == 0
    rx.process_fmt(good)  # ... and nothing of that was queued
    want, _ = rs.apply(rr.to_complex(good), h, L, M)
    assert _same(rx.raw(), want)
    # shared frames: neither as the reader nor as the source
    plain = Receiver.from_topology(topo)
    plain.process(floats)
    assert _code(lambda: rx.process_shared(plain)) == _lib.SDRX_ESTATE and _code(lambda: plain.process_shared(rx)) == _lib.SDRX_ESTATE
    assert _code(lambda: rx.submit_shared(plain)) == _lib.SDRX_ESTATE and _code(lambda: plain.submit_shared(rx)) == _lib.SDRX_ESTATE
    assert _code(lambda: plain.process_if_same(rx, floats)) == _lib.SDRX_ESTATE and _code(lambda: rx.submit_if_same(plain, floats)) == _lib.SDRX_ESTATE
    plain.close()
    rx.close()


@pytest.mark.parametrize("why,fs_in,taps_per_phase", [
    ("n M % L", 5346, 16),          # 5184 / 5346 = 32 / 33: 1296 * 33 is no multiple of 32
    ("n_in % 16", 6480, 16),        # 4 / 5: n_in = 1620
    ("L <= 1024", 5183, 16),        # L = 5184
    ("M / L <= 4", 25920, 16),      # 1 / 5
    ("1/2 <= M / L", 2304, 16),     # 9 / 4
    ("T % 4", 6912, 18),
    ("T >= 8", 6912, 4),
    ("T <= 64", 6912, 68)])
def test_finalize_refuses(why, fs_in, taps_per_phase):
    """Every rule of the header is SDRX_EUNSUPPORTED at sdrx_finalize, with the reason; afterwards the context takes a valid
    setting and finalizes.  (n_in >= taps_per_phase cannot be missed by a tree sdrx_finalize takes: its frames have at least
    256 samples, so n_in >= 128.)"""
    case = rr.CASES[2]
    L, M, T, n_in, n = case
    topo = rr.tree(case)
    rx = Receiver()
    for d in topo.vfos:
        rx.add_vfo(d)
    h = np.ones(32768, np.float32)
    rx._chk(rx.L.sdrx_set_resampler(rx.h, fs_in, h.ctypes.data, taps_per_phase))
    assert rx.L.sdrx_finalize(rx.h) == _lib.SDRX_EUNSUPPORTED, why
    assert b"resampler" in rx.L.sdrx_last_error(rx.h)
    rx._chk(rx.L.sdrx_set_resampler(rx.h, 4 * n_in, h.ctypes.data, T))
    rx.finalize()
    info = _lib.ResamplerInfoC()
    rx._chk(rx.L.sdrx_get_resampler(rx.h, C.byref(info), None, 0))
    assert (info.in_frame, info.out_frame, info.L, info.M) == (n_in, n, L, M)
    rx.close()


def test_finalize_refuses_roots_of_two_rates_and_too_many_taps():
    case = rr.CASES[2]
    L, M, T, n_in, n = case
    topo = rr.tree(case)
    rx = Receiver()
    for d in topo.vfos[:3]:
        rx.add_vfo(d)
    rx.add_vfo(tp.VfoDesc(topic="RAW03", parent=-1, fs=8 * n, decimate_count=0, mixer_freq=1.0, demod_usb=False, cstyle=0, samples_per_buffer=n))
    h = rr.random_taps(case)
    rx._chk(rx.L.sdrx_set_resampler(rx.h, 4 * n_in, h.ctypes.data, T))
    assert rx.L.sdrx_finalize(rx.h) == _lib.SDRX_EUNSUPPORTED and b"share one fs" in rx.L.sdrx_last_error(rx.h)
    rx.close()
    # L T <= 32768: L = 1024 with 36 taps per phase
    t = tp.Topology(fs=16384, frame=4096, name="wide")
    t.vfos.append(tp.VfoDesc(topic="W", parent=-1, fs=16384, decimate_count=0, mixer_freq=100.0, demod_usb=False, cstyle=0, samples_per_buffer=4096))
    rx = Receiver()
    rx.add_vfo(t.vfos[0])
    big = np.ones(1024 * 36, np.float32)
    rx._chk(rx.L.sdrx_set_resampler(rx.h, 16368, big.ctypes.data, 36))  # 16384 / 16368 = 1024 / 1023
    assert rx.L.sdrx_finalize(rx.h) == _lib.SDRX_EUNSUPPORTED and b"32768" in rx.L.sdrx_last_error(rx.h)
    rx.close()


# ---- the C++ host layer: sdrj::setInputRate behind sdrx_demo --input-rate ------------------------------------------------------
def test_demo_takes_frames_at_the_input_rate(tmp_path):
    import os
    import subprocess
    from test_topology import INI_25E_LIKE
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    demo = os.path.join(root, "host", "sdrx_demo")
    subprocess.check_call(["make", "-C", os.path.join(root, "host")], stdout=subprocess.DEVNULL)
    profile = tmp_path / "profile.ini"
    profile.write_text(INI_25E_LIKE)
    plain = subprocess.check_output([demo, str(profile), "--frames", "2", "--format", "cs16"], text=True).splitlines()
    lines = subprocess.check_output([demo, str(profile), "--frames", "2", "--format", "cs16", "--input-rate", "2400000"], text=True).splitlines()
    head = lines[0].split()
    fs_out, n = int(head[2]), int(head[7])
    L, M = rs.ratio(2400000, fs_out)
    assert head[:8] == ["resampler", "2400000", str(fs_out), str(L), str(M), "32", str(rs.in_frame(2400000, fs_out, n)), str(n)]
    assert float(head[8]) == pytest.approx((L * 32 - 1) / (2.0 * M)) and float(head[9]) == pytest.approx(rs.design(2400000, fs_out, 32)[1]["passband_hz"], rel=1e-6)
    # the same messages in the same order (frame, topic, rate, bytes), other payloads: the frames are other samples
    assert [ln.split()[:4] for ln in lines[1:]] == [ln.split()[:4] for ln in plain] and len(plain) > 0
