"""The device spectrum display (sdrx_set_spectrum / sdrx_get_spectrum / sdrx_get_spectrum_levels) against the numpy
restatement of fftHandlerSlot (tests/spectrum_ref.py, itself pinned bit for bit to the real kiss_fft): every update's input
is what sdrx_get_stream / sdrx_get_raw return for that frame (both pinned to the oracle elsewhere), or the test's own device
tensor for device frames.  Bins bit-exact; pwr / smooth / maxval / aveval within 1e-9 dB.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import spectrum_ref as sr
from sdrreceiver_amd import _lib, synth, topology as tp

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def R():
    from sdrreceiver_amd.receiver import Receiver
    return Receiver


def check(got, d: sr.Display, ctx):
    assert got["updates"] == d.updates, ctx
    assert np.array_equal(got["bins"].view(np.uint32), d.bins.view(np.uint32)), ctx
    assert np.abs(got["pwr"] - d.pwr).max() <= TOL, ctx
    assert np.abs(got["smooth"] - d.smooth).max() <= TOL, ctx
    if d.updates:
        assert abs(got["maxval"] - d.maxval) <= TOL and abs(got["aveval"] - d.aveval) <= TOL, ctx


def stream_len(topo, v):
    return topo.vfos[v].samples_per_buffer >> topo.vfos[v].decimate_count


def run_vfos(rx, topo, vids, frames, feed, ctx):
    """feed(f) processes frame f; every VFO of `vids` is checked after every frame."""
    disp = {v: sr.Display() for v in vids}
    for v in vids:
        rx.set_spectrum(v)
    for f in range(frames):
        feed(f)
        for v in vids:
            disp[v].update(rx.stream(v))
            got = rx.spectrum(v)
            assert got["n_in"] == min(stream_len(topo, v), sr.N)
            check(got, disp[v], (ctx, f, v))
    return disp


@pytest.mark.parametrize("exact", [1, 0, 2])
def test_config1_leaf_and_main_every_frame(R, exact):
    """The sub VFO (a leaf: natural order) and the main VFO (tile layout) of config 1 over 9 frames, in all three
    arithmetics: the bins are kiss_fft's of whatever stream that arithmetic produced."""
    topo = tp.config1()
    rx = R.from_topology(topo, device=0, exact=exact)
    lcg = synth.Lcg(5)
    frames = [synth.lcg_frame(topo.frame, lcg) for _ in range(9)]
    run_vfos(rx, topo, [0, 1], 9, lambda f: rx.process(frames[f]), ("config1", exact))
    rx.close()


def test_short_stream_of_sdr_25e_is_zero_padded(R):
    topo = tp.profile_25e()
    vid = next(v for v in range(len(topo.vfos)) if stream_len(topo, v) == 3000)
    rx = R.from_topology(topo, device=0)
    lcg = synth.Lcg(7)
    run_vfos(rx, topo, [vid, 0], 9, lambda f: rx.process_u8(synth.lcg_frame_u8(topo.frame, lcg), correct_dc=True), "25e")
    assert rx.spectrum(vid)["n_in"] == 3000
    rx.close()


def test_tapped_fused_leaf_of_config4(R):
    """A /5 leaf whose decimating low-pass runs inside the mix wave: its stream exists only while it is tapped, and so do its
    spectrum's updates."""
    topo = tp.config4(12)
    leaf = 3 + 4
    rx = R.from_topology(topo, device=0)
    lcg = synth.Lcg(9)
    rx.set_spectrum(leaf)
    for _ in range(2):
        rx.process(synth.lcg_frame(topo.frame, lcg))
    assert rx.spectrum(leaf)["updates"] == 0  # not tapped: no stream, no update
    rx.set_tap(leaf)
    run_vfos(rx, topo, [leaf], 9, lambda f: rx.process(synth.lcg_frame(topo.frame, lcg)), "config4 tap")
    rx.close()


def _raw_run(R, topo, frames, feed, raw_of, ctx, **kw):
    rx = R.from_topology(topo, device=0, **kw)
    rx.set_spectrum(_lib.SPECTRUM_RAW)
    d = sr.Display()
    calls = sr.raw_update_calls(frames)
    for f in range(frames):
        feed(rx, f)
        if f + 1 in calls:
            d.update(raw_of(rx, f))
        check(rx.spectrum(_lib.SPECTRUM_RAW), d, (ctx, f))
    assert d.updates == len(calls) and calls[:2] == [5, 9]
    return rx, d


@pytest.mark.parametrize("form", ["process", "u8", "u8_dc", "device"])
def test_raw_frame_spectrum_every_fourth_frame(R, form):
    import torch
    topo = tp.config1()
    lcg = synth.Lcg(3)
    n = 10
    if form == "process":
        fr = [synth.lcg_frame(topo.frame, lcg) for _ in range(n)]
        feed = lambda rx, f: rx.process(fr[f])  # noqa: E731
    elif form.startswith("u8"):
        fr = [synth.lcg_frame_u8(topo.frame, lcg) for _ in range(n)]
        feed = lambda rx, f: rx.process_u8(fr[f], correct_dc=form == "u8_dc")  # noqa: E731
    else:
        fr = [synth.lcg_frame(topo.frame, lcg) for _ in range(n)]
        dev = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() for x in fr]
        torch.cuda.synchronize()
        feed = lambda rx, f: rx.process_device(dev[f].data_ptr(), topo.frame)  # noqa: E731
    raw_of = (lambda rx, f: np.ascontiguousarray(fr[f], np.float32).reshape(-1).view(np.complex64)) if form == "device" \
        else (lambda rx, f: rx.raw())
    rx, d = _raw_run(R, topo, n, feed, raw_of, form)
    # disabling and re-enabling restarts the state and sdrj's counter
    rx.set_spectrum(_lib.SPECTRUM_RAW, False)
    rx.set_spectrum(_lib.SPECTRUM_RAW)
    d2 = sr.Display()
    for f in range(5):
        feed(rx, f)
        if f == 4:
            d2.update(raw_of(rx, f))
        check(rx.spectrum(_lib.SPECTRUM_RAW), d2, (form, "re-enabled", f))
    rx.close()


def test_pipelined_submit_and_device_queue_equal_the_synchronous_path(R):
    """submit/wait with two frames in flight, and process_device through the frame pipeline (k_mix_levels' level lag), give
    the synchronous path's spectra bit for bit."""
    import torch
    topo = tp.config1()
    lcg = synth.Lcg(21)
    fr = [synth.lcg_frame(topo.frame, lcg) for _ in range(9)]
    sync = R.from_topology(topo, device=0)
    disp = run_vfos(sync, topo, [0, 1], 9, lambda f: sync.process(fr[f]), "sync")
    pipe = R.from_topology(topo, device=0)
    for v in (0, 1):
        pipe.set_spectrum(v)
    pipe.submit(fr[0])
    for f in range(1, 9):
        pipe.submit(fr[f])
        pipe.wait()
    with pytest.raises(Exception) as e:
        pipe.spectrum(0)  # a frame is still in flight
    assert getattr(e.value, "code", None) == _lib.SDRX_ESTATE
    pipe.wait()
    dev = R.from_topology(topo, device=0)
    for v in (0, 1):
        dev.set_spectrum(v)
    t = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() for x in fr]
    torch.cuda.synchronize()
    for x in t:
        dev.process_device(x.data_ptr(), topo.frame)
    for rx, ctx in ((pipe, "submit"), (dev, "device")):
        for v in (0, 1):
            check(rx.spectrum(v), disp[v], (ctx, v))
    for rx in (sync, pipe, dev):
        rx.close()


def test_config3_every_sub_has_a_spectrum(R):
    topo = tp.config3(1024)
    subs = list(range(2, len(topo.vfos)))
    rng = np.random.default_rng(1234)
    checked = sorted(set([subs[0], subs[-1]] + [int(v) for v in rng.choice(subs, 32, replace=False)]))
    on = R.from_topology(topo, device=0)
    off = R.from_topology(topo, device=0)
    for v in subs:
        on.set_spectrum(v)
    disp = {v: sr.Display() for v in checked}
    lcg = synth.Lcg(77)
    for f in range(9):
        iq = synth.lcg_frame(topo.frame, lcg)
        on.process(iq)
        off.process(iq)
        for v in range(2, len(topo.vfos)):
            assert np.array_equal(on.output(v), off.output(v)), (f, v)
        if f in (0, 8):
            for v in range(len(topo.vfos)):
                assert np.array_equal(on.stream(v).view(np.uint64), off.stream(v).view(np.uint64)), (f, v)
        for v in checked:
            disp[v].update(on.stream(v))
            check(on.spectrum(v), disp[v], ("config3", f, v))
    lv = on.spectrum_levels(subs)
    for k, v in enumerate(subs):
        if v in disp:
            assert abs(lv["maxval"][k] - disp[v].maxval) <= TOL and abs(lv["aveval"][k] - disp[v].aveval) <= TOL
        s = on.spectrum(v) if v in checked or k % 97 == 0 else None
        if s is not None:
            assert (lv["maxval"][k], lv["aveval"][k], lv["updates"][k]) == (s["maxval"], s["aveval"], s["updates"])
    assert (lv["updates"] == 9).all()
    on.close()
    off.close()


def test_errors(R):
    from sdrreceiver_amd.receiver import SdrxError
    topo = tp.config1()
    rx = R(device=0)
    for d in topo.vfos:
        rx.add_vfo(d)
    with pytest.raises(SdrxError) as e:
        rx.set_spectrum(1)
    assert e.value.code == _lib.SDRX_ESTATE
    rx.finalize()
    for bad in (2, -1, -3, 99):
        with pytest.raises(SdrxError) as e:
            rx.set_spectrum(bad)
        assert e.value.code == _lib.SDRX_EINVAL, bad
    with pytest.raises(SdrxError) as e:
        rx.spectrum(1)  # not enabled
    assert e.value.code == _lib.SDRX_ESTATE
    with pytest.raises(SdrxError) as e:
        rx.spectrum(7)
    assert e.value.code == _lib.SDRX_EINVAL
    rx.set_spectrum(1)
    s = rx.spectrum(1)
    assert s["updates"] == 0 and s["n_in"] == 3000 and not s["pwr"].any()
    iq = synth.lcg_frame(topo.frame, synth.Lcg(2))
    rx.submit(iq)
    for call in (lambda: rx.spectrum(1), lambda: rx.spectrum_levels([1]), lambda: rx.set_spectrum(0)):
        with pytest.raises(SdrxError) as e:
            call()
        assert e.value.code == _lib.SDRX_ESTATE
    rx.wait()
    assert rx.spectrum(1)["updates"] == 1
    rx.close()


def test_group_members_carry_spectra(R):
    from sdrreceiver_amd.receiver import Group
    topo = tp.profile_25e()
    grp = Group.from_topology(topo, devices=[0, 0])
    L = _lib.lib()
    vids = [2, 3, len(topo.vfos) - 1]
    where = {v: grp.locate(v) for v in vids}
    assert len({m for m, _ in where.values()}) == 2
    for v, (m, lid) in where.items():
        ctx, _ = grp.member_context(m)
        assert L.sdrx_set_spectrum(ctx, lid, 1) == 0
    disp = {v: sr.Display() for v in vids}
    lcg = synth.Lcg(31)
    for f in range(3):
        grp.process(synth.lcg_frame(topo.frame, lcg))
        for v, (m, lid) in where.items():
            disp[v].update(grp.stream(v))
            ctx, _ = grp.member_context(m)
            info = _lib.SpectrumInfoC()
            pwr, smooth = np.zeros(sr.N), np.zeros(sr.N - 10)
            bins = np.zeros(2 * sr.N, np.float32)
            assert L.sdrx_get_spectrum(ctx, lid, C.byref(info), pwr.ctypes.data, smooth.ctypes.data, bins.ctypes.data) == 0
            check({"updates": info.updates, "bins": bins.view(np.complex64), "pwr": pwr, "smooth": smooth,
                   "maxval": info.maxval, "aveval": info.aveval}, disp[v], ("group", f, v))
    grp.close()
