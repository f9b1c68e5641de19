"""The spur canceller on the device (sdrx_set_notch, notch.hip) against the model sdrreceiver_amd.notch, bit for bit: every crafted
case of tests/notch_ref.py in the three arithmetics (raw frame, record, settings read back, leaf payloads); cf32 and CS16 frames from
host and device memory; sdrx_process, two frames in flight and frames queued on the device with one fetch; the shift behind it and
the resampler in front; a live change between frames; off means off and what on costs; and the refusals."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import notch_ref as nr
import shift_ref as sr
from helpers import bits
from oracle import binding as ob
from sdrreceiver_amd import _lib, ingest, notch as nt, shift as sh
from sdrreceiver_amd.receiver import Group, Receiver, SdrxError
from test_gpu_parity import _check_exact

pytestmark = pytest.mark.gpu

N = 8464  # two full blocks and a short one: the smallest frame with a frequency step
CASE = f"off20_afc1_n{N}"


def _same(a, b):
    return np.array_equal(bits(np.ascontiguousarray(a)), bits(np.ascontiguousarray(b)))


def _code(call):
    with pytest.raises(SdrxError) as e:
        call()
    return e.value.code


def _leaves(topo):
    return [i for i in range(len(topo.vfos)) if not topo.children(i)]


def _launches(rx):
    return {k: v["launches"] for k, v in rx.kernel_times().items()}


def _device(frames):
    import torch
    out = [torch.from_numpy(np.array(v)).cuda() for v in frames]  # (a copy: the shared frames are read-only)
    torch.cuda.synchronize()
    return out


def _cfg32(c: nt.Cfg) -> tuple:
    """The settings as the library holds them: mu, afc_gain and min_coherence are fp32"""
    return (tuple(c.inc0), float(np.float32(c.mu)), float(np.float32(c.afc_gain)), float(np.float32(c.min_coherence)), int(c.max_pull), int(c.flags))


def _mismatch(got, want, what):
    bad = np.flatnonzero(got.view(np.uint64) != np.ascontiguousarray(want).view(np.uint64))
    assert got.size == want.size and bad.size == 0, (what, bad.size, int(bad[0]))


def _check_stage(rx, y, rec, what, cfg=None):
    """The stage of the last delivered frame against the model: the tree's raw frame, the record, the settings"""
    _mismatch(rx.raw(), y, (what, "raw"))
    got = rx.notch
    assert nt.record_key(got) == nt.record_key(rec), (what, got, rec)
    if cfg is not None:
        assert _cfg32(got["cfg"]) == _cfg32(cfg), (what, got["cfg"], cfg)


def _check_twin(rx, twin, topo, what):
    assert rx.published == twin.published and len(rx.published) == len(_leaves(topo)), (what, "published")
    for i in range(len(topo.vfos)):
        assert _same(rx.stream(i), twin.stream(i)), (what, i, "stream")
    for i in _leaves(topo):
        assert np.array_equal(rx.output(i), twin.output(i)), (what, i, "payload")


# ---- 1. every crafted case, in the three arithmetics ------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [1, 0, 2])
@pytest.mark.parametrize("case", nr.crafted(), ids=nr.case_ids())
def test_crafted_case(case, exact):
    topo = nr.tree(case.n)
    ys, recs = nr.model_run(case)
    kw = dict(exact=exact, keep_streams=True)
    rx = Receiver.from_topology(topo, notch=case.cfgs[0], **kw)
    twin = nodes = None
    if case.finite and exact == 1:
        nodes, roots = ob.build_tree("port", topo)
    elif case.finite:
        twin = Receiver.from_topology(topo, **kw)  # (no stage: fed the model's notched frames)
    for f, x in enumerate(case.frames):
        if f and case.cfgs[f] is not case.cfgs[f - 1]:
            rx._set_notch_cfg(case.cfgs[f])
        rx.process(x.view(np.float32))
        _check_stage(rx, ys[f], recs[f], (case.name, exact, f), case.cfgs[f])
        if nodes:
            ob.process_roots(roots, np.ascontiguousarray(ys[f]).view(np.float32))
            _check_exact(rx, nodes, topo, (case.name, f))
        elif twin:
            twin.process(ys[f].view(np.float32))
            _check_twin(rx, twin, topo, (case.name, exact, f))
    rx.close()
    if twin:
        twin.close()


# ---- 2. every way a frame is handed over ---------------------------------------------------------------------------------------------
CFG16 = nr.cfg([nr.BASE, nr.hz(-300000.0)])


def _cs16_frames():
    """CS16 frames of noise (blank_ref's) with two carriers added: one 3 Hz beside where it is given, one where it is given"""
    out = []
    for f, v in enumerate(nr.integer_frames(ingest.CS16, N, seed=3, frames=3)):
        t = nr.signal(N, f, [(0.25, nr.BASE + nr.hz(3.0), 0.3), (0.1, nr.hz(-300000.0), 0.6)], 7, noise=0.0)
        w = np.clip(v.astype(np.int64) + np.rint(t.view(np.float32) * 32768.0).astype(np.int64), -32768, 32767).astype(np.int16)
        out.append(w)
    return out


@pytest.mark.parametrize("where", ["host", "device"])
def test_cs16_frames_with_the_adc_meter_untouched(where):
    topo = nr.tree(N)
    frames = _cs16_frames()
    rx = Receiver.from_topology(topo, notch=CFG16, keep_streams=True, adc_meter=True)
    plain = Receiver.from_topology(topo, adc_meter=True)  # (no stage: the ADC meter sees the samples as they arrived)
    nodes, roots = ob.build_tree("port", topo)
    dev = _device(frames) if where == "device" else None
    st = nt.State.initial(CFG16)
    for f, v in enumerate(frames):
        if dev:
            rx.process_device_fmt(dev[f].data_ptr(), N, ingest.CS16, False)
            rx.fetch()
        else:
            rx.process_fmt(v, correct_dc=False)
        plain.process_fmt(v, correct_dc=False)
        y, rec, st = nt.apply(ingest.to_float(v).view(np.complex64), CFG16, st)
        _check_stage(rx, y, rec, (where, f))
        assert rx.adc_meter() == plain.adc_meter()
        ob.process_roots(roots, np.ascontiguousarray(y).view(np.float32))
        _check_exact(rx, nodes, topo, (where, f))
    assert rec["tones"][0]["adapted"] and rec["tones"][0]["inc_next"] != CFG16.inc0[0]  # the first carrier was followed
    rx.close()
    plain.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_cf32_frames_and_the_callers_buffer_is_never_written(where):
    case = nr.by_name(CASE)
    topo = nr.tree(N)
    ys, recs = nr.model_run(case)
    rx = Receiver.from_topology(topo, notch=case.cfgs[0], keep_streams=True)
    nodes, roots = ob.build_tree("port", topo)
    host = [np.array(x.view(np.float32)) for x in case.frames]
    dev = _device(host) if where == "device" else None
    for f, x in enumerate(case.frames):
        if dev:
            rx.process_device(dev[f].data_ptr(), N)
            rx.fetch()
        else:
            rx.process(host[f])
        _check_stage(rx, ys[f], recs[f], (where, f))
        ob.process_roots(roots, np.ascontiguousarray(ys[f]).view(np.float32))
        _check_exact(rx, nodes, topo, (where, f))
    for f, x in enumerate(case.frames):  # the caller's frames are what they were
        assert _same(host[f], x.view(np.float32))
        if dev:
            assert _same(dev[f].cpu().numpy(), x.view(np.float32))
    rx.close()


# ---- 3. frames in flight, frames queued on the device: the state carries without a host call ----------------------------------------
def test_two_frames_in_flight_and_four_frames_queued_on_the_device():
    topo = nr.tree(N)
    case = nr.by_name(CASE)
    cfg = case.cfgs[0]
    ys, recs = nr.model_run(case)
    frames = [np.array(x.view(np.float32)) for x in case.frames]
    ref = Receiver.from_topology(topo)  # (no stage, fed the model's frames)
    want = []
    for y in ys:
        ref.process(y.view(np.float32))
        want.append(list(ref.published))
    ref.close()
    keys = [nt.record_key(r) for r in recs]
    assert all(len(m) == 3 for m in want) and len({r["tones"][0]["inc"] for r in recs}) >= 3  # the increment moves between frames

    rx = Receiver.from_topology(topo, notch=cfg)  # sdrx_process: one frame at a time
    for f in range(nr.N_FRAMES):
        rx.process(frames[f])
        assert rx.published == want[f] and nt.record_key(rx.notch) == keys[f]
    rx.close()

    rx = Receiver.from_topology(topo, notch=cfg)  # sdrx_submit / sdrx_wait, two frames in flight
    rx.submit(frames[0])
    rx.submit(frames[1])
    rx.wait()
    assert rx.published == want[0] and nt.record_key(rx.notch) == keys[0]
    rx.submit(frames[2])
    rx.wait()
    assert rx.published == want[1] and nt.record_key(rx.notch) == keys[1]
    rx.submit(frames[3])
    rx.wait()
    assert rx.published == want[2] and nt.record_key(rx.notch) == keys[2]
    rx.wait()
    assert rx.published == want[3] and nt.record_key(rx.notch) == keys[3]
    assert _same(rx.raw(), ys[3])
    rx.close()

    dev = _device(frames)  # sdrx_process_device queued back to back, one fetch: the state moved across them with no host call
    rx = Receiver.from_topology(topo, notch=cfg)
    for k in range(nr.N_FRAMES):
        rx.process_device(dev[k].data_ptr(), N)
    rx.fetch()
    assert rx.published == want[3] and nt.record_key(rx.notch) == keys[3]
    assert _same(rx.raw(), ys[3])
    rx.close()


# ---- 4. the resampler in front, the shift behind -------------------------------------------------------------------------------------
def test_behind_the_resampler_and_in_front_of_the_shift():
    """shift_ref's 4112 -> 4096 resampler case: the notch sees the tree's 4096 samples (one block), the shift what the notch left.
    One device copy of the tables serves both: device_bytes grows by the notch's figure less the tables."""
    n_in = 4112
    topo = sr.tree(n_in)
    n = sr.tree_len(n_in)
    ncfg = nr.cfg([nr.BASE, nr.hz(100000.0)], mu=0.5)
    scfg = sh.Cfg(3451912, sr.wrap_at(3451912, 1024))
    rx = Receiver.from_topology(topo, notch=ncfg, shift=scfg, keep_streams=True, **sr.receiver_kw(n_in))
    only_shift = Receiver.from_topology(topo, shift=scfg, **sr.receiver_kw(n_in))
    assert rx.stats()["device_bytes"] - only_shift.stats()["device_bytes"] == nt.device_bytes(n, shift_on=True)
    only_shift.close()
    nodes, roots = ob.build_tree("port", topo)
    nst, sst, hist = nt.State.initial(ncfg), sh.State.initial(scfg), None
    for f in range(3):
        x = nr.signal(n_in, f, [(30.0, nr.BASE * 256 / 257, 0.1), (5.0, nr.hz(100000.0) * 256 / 257, 0.2)], 11)  # (where the resampler puts them)
        rx.process(x.view(np.float32))
        z, hist = sr.behind(n_in, x, hist)
        y, nrec, nst = nt.apply(z, ncfg, nst)
        w, srec, sst = sh.apply(y, sst)
        _mismatch(rx.raw(), w, (f, "raw"))
        assert nt.record_key(rx.notch) == nt.record_key(nrec) and nrec["n_complex"] == n != n_in
        assert {k: rx.shift[k] for k in sh.RECORD_FIELDS} == srec
        assert rx.resampler_input().size == sr.rs_case(n_in)[3]
        ob.process_roots(roots, np.ascontiguousarray(w).view(np.float32))
        _check_exact(rx, nodes, topo, f)
    rx.close()


# ---- 5. a live change through the Python interface -------------------------------------------------------------------------------------
def test_set_notch_between_frames_in_hz():
    topo = nr.tree(N)
    fs = float(topo.vfos[0].fs)
    f1, f2, f3 = 0.11 * fs, -0.23 * fs, 0.31 * fs
    kw = dict(hz=[f1, f2], mu=0.25, afc_gain=1.0, min_coherence=0.5, max_pull_hz=fs / 1000)
    rx = Receiver.from_topology(topo, notch=kw)
    cfg = nt.Cfg((sh.inc_of(fs, f1), sh.inc_of(fs, f2)), 0.25, 1.0, 0.5, sh.inc_of(fs, fs / 1000))
    assert rx._notch == cfg
    tones = [(20.0, cfg.inc0[0] + 300, 0.1), (8.0, cfg.inc0[1] - 200 - 2 ** 32, 0.2), (12.0, sh.inc_of(fs, f3), 0.3)]
    st = nt.State.initial(cfg)
    for f in range(5):
        if f == 2:  # the first tone stays (and keeps its state), the second is replaced; mu changes, the rest is kept
            rx.set_notch(hz=[f1, f3], mu=0.5)
            new = dataclasses.replace(cfg, inc0=(cfg.inc0[0], sh.inc_of(fs, f3)), mu=0.5)
            st, cfg = nt.load(st, cfg, new), new
            assert st.tones[0].a_re != 0 and st.tones[1] == nt.Tone.start(cfg.inc0[1])
        if f == 4:
            rx.set_notch(load=True)
            new = dataclasses.replace(cfg, flags=nt.LOAD)
            st, cfg = nt.load(st, cfg, new), new
        x = nr.signal(N, f, tones, 13)
        rx.process(x.view(np.float32))
        y, rec, st = nt.apply(x, cfg, st)
        _check_stage(rx, y, rec, f, cfg)
    lv = rx.notch["levels"]
    assert len(lv) == 2 and lv[0]["hz"] == sh.hz_of(fs, rec["tones"][0]["inc_next"])
    rx.close()


# ---- 6. off means off, and what on costs -------------------------------------------------------------------------------------------------
def test_off_means_off_and_what_on_costs():
    topo = nr.tree(N)
    never, off, on = Receiver(), Receiver(), Receiver()
    for r in (never, off, on):
        for d in topo.vfos:
            r.add_vfo(d)
    off._set_notch_cfg(CFG16)
    off.set_notch(off=True)
    on._set_notch_cfg(CFG16)
    for r in (never, off, on):
        r.finalize()
        r.enable_kernel_timing(True)
    assert off.stats()["device_bytes"] == never.stats()["device_bytes"]
    # on: eight slots of 32 bytes, c and used of the frame's 3 blocks (8 slots of 8 bytes each), two records of 544 bytes, the tables
    assert on.stats()["device_bytes"] - never.stats()["device_bytes"] == nt.device_bytes(N) == 256 + 2 * 3 * 64 + 2 * 544 + 6144 == 7872
    v = _cs16_frames()[0]
    for r in (never, off, on):
        r.process_fmt(v)
    assert off.published == never.published and _same(off.raw(), never.raw())
    assert _launches(off) == _launches(never) == _launches(on)  # (the stage's kernels run inside the ingest bracket)
    x = nr.signal(N, 1, [], 1)
    for r in (never, off):
        r.process(x.view(np.float32))
    assert off.published == never.published and _same(off.raw(), never.raw()) and _launches(off) == _launches(never)
    assert off.notch is None and off.L.sdrx_get_notch(off.h, C.byref(_lib.NotchCfgC()), C.byref(_lib.NotchRecordC())) == _lib.SDRX_ESTATE
    for r in (never, off, on):
        r.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def _c(inc0=(1 << 24,), mu=0.25, afc=1.0, coh=0.5, pull=100, flags=0, n_tones=None):
    c = _lib.NotchCfgC(n_tones=len(inc0) if n_tones is None else n_tones, flags=flags, max_pull=pull, mu=mu, afc_gain=afc, min_coherence=coh)
    for k, v in enumerate(inc0):
        c.inc0[k] = v
    return c


def test_refusals():
    topo = nr.tree(N)
    lib = _lib.lib()
    good = _c()
    cfg_out, rec_out = _lib.NotchCfgC(), _lib.NotchRecordC()
    nan = float("nan")
    res0, res1, res = _c(), _c(), _c()
    res0.reserved0, res1.reserved1, res.reserved[7] = 1, 1, 1
    bad = [_c(mu=0.0), _c(mu=1.5), _c(mu=nan), _c(mu=-0.25), _c(afc=-0.1), _c(afc=1.1), _c(afc=nan), _c(coh=0.0), _c(coh=1.01), _c(coh=nan), _c(flags=2),
           _c(flags=3), _c(n_tones=9), _c(inc0=(5, 7), n_tones=1), res0, res1, res,
           _c(inc0=(1000, 1000 + nt.SPACING - 1)), _c(inc0=(5, 5)), _c(inc0=(2 ** 32 - 100, nt.SPACING - 101)),  # (the distance is circular)
           _c(inc0=tuple(k * nt.SPACING for k in range(7)) + (3 * nt.SPACING + 1,))]
    ok = [_c(inc0=(1000, 1000 + nt.SPACING)), _c(inc0=(2 ** 32 - 100, nt.SPACING - 100)), _c(mu=1.0, afc=0.0, coh=1.0, pull=2 ** 32 - 1),
          _c(inc0=tuple(k * nt.SPACING for k in range(8)))]
    assert nt.check_cfg(nt.Cfg((1000, 1000 + nt.SPACING - 1), 0.25, 1.0, 0.5, 100)) and not nt.check_cfg(nt.Cfg((1000, 1000 + nt.SPACING), 0.25, 1.0, 0.5, 100))
    rx = Receiver()
    for d in topo.vfos:
        rx.add_vfo(d)
    for b in bad:
        assert lib.sdrx_set_notch(rx.h, C.byref(b)) == _lib.SDRX_EINVAL
    for g in ok:
        assert lib.sdrx_set_notch(rx.h, C.byref(g)) == 0
    assert lib.sdrx_get_notch(rx.h, C.byref(cfg_out), C.byref(rec_out)) == _lib.SDRX_ESTATE  # before sdrx_finalize
    assert lib.sdrx_set_notch(rx.h, C.byref(good)) == 0
    rx._notch = nt.Cfg((1 << 24,), 0.25, 1.0, 0.5, 100)
    rx.finalize()
    for b in bad:
        assert lib.sdrx_set_notch(rx.h, C.byref(b)) == _lib.SDRX_EINVAL
    assert lib.sdrx_set_notch(rx.h, None) == _lib.SDRX_ESTATE
    with pytest.raises(ValueError):
        rx.set_notch(hz=[rx.tree_rate])  # beyond half the rate
    with pytest.raises(ValueError):
        rx.set_notch(hz=[1.0], inc=[1])
    # the record before a frame; the settings are there as written
    assert lib.sdrx_get_notch(rx.h, None, C.byref(rec_out)) == _lib.SDRX_ESTATE
    assert lib.sdrx_get_notch(rx.h, C.byref(cfg_out), None) == 0 and (cfg_out.n_tones, cfg_out.inc0[0], cfg_out.max_pull) == (1, 1 << 24, 100)
    rx.process(np.zeros(2 * N, np.float32))
    assert lib.sdrx_get_notch(rx.h, None, None) == _lib.SDRX_EINVAL
    assert lib.sdrx_get_notch(rx.h, None, C.byref(rec_out)) == 0 and (rec_out.n_tones, rec_out.n_complex, rec_out.blocks, rec_out.tone[0].inc) == (1, N, 3, 1 << 24)
    # frames in flight: not the setter
    rx.submit(np.zeros(2 * N, np.float32))
    assert lib.sdrx_set_notch(rx.h, C.byref(good)) == _lib.SDRX_ESTATE
    rx.wait()
    assert lib.sdrx_set_notch(rx.h, C.byref(good)) == 0
    # no tones on a running stage: the frame passes as it came
    assert lib.sdrx_set_notch(rx.h, C.byref(_c(inc0=()))) == 0
    x = nr.signal(N, 0, [(3.0, 1 << 24, 0.0)], 5)
    rx.process(x.view(np.float32))
    assert _same(rx.raw(), x) and rx.notch["n_tones"] == 0
    # shared frames: neither as the reader nor as the source
    plain = Receiver.from_topology(topo)
    floats = np.zeros(2 * N, np.float32)
    plain.process(floats)
    assert _code(lambda: rx.process_shared(plain)) == _lib.SDRX_ESTATE and _code(lambda: plain.process_shared(rx)) == _lib.SDRX_ESTATE
    assert _code(lambda: rx.submit_shared(plain)) == _lib.SDRX_ESTATE and _code(lambda: plain.submit_shared(rx)) == _lib.SDRX_ESTATE
    assert _code(lambda: plain.process_if_same(rx, floats)) == _lib.SDRX_ESTATE and _code(lambda: rx.submit_if_same(plain, floats)) == _lib.SDRX_ESTATE
    # a context without the stage: the setter after sdrx_finalize, the getter
    assert lib.sdrx_set_notch(plain.h, C.byref(good)) == _lib.SDRX_ESTATE
    assert lib.sdrx_get_notch(plain.h, C.byref(cfg_out), C.byref(rec_out)) == _lib.SDRX_ESTATE
    assert lib.sdrx_set_notch(None, C.byref(good)) == _lib.SDRX_EINVAL and lib.sdrx_get_notch(None, C.byref(cfg_out), None) == _lib.SDRX_EINVAL
    plain.close()
    rx.close()


def test_a_group_does_not_offer_it():
    g = Group.from_topology(nr.tree(N), [0, 0])
    ctx, _ = g.member_context(0)
    assert g.L.sdrx_set_notch(ctx, C.byref(_c())) == _lib.SDRX_ESTATE
    assert g.L.sdrx_get_notch(ctx, C.byref(_lib.NotchCfgC()), C.byref(_lib.NotchRecordC())) == _lib.SDRX_ESTATE
    g.close()


# ---- the C++ host layer: sdrj::setNotch behind sdrx_demo --notch -----------------------------------------------------------------------
def test_demo_prints_the_tracked_frequencies(tmp_path):
    import os
    import subprocess
    from test_topology import INI_25E_LIKE
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    demo = os.path.join(root, "host", "sdrx_demo")
    subprocess.check_call(["make", "-C", os.path.join(root, "host")], stdout=subprocess.DEVNULL)
    profile = tmp_path / "profile.ini"
    profile.write_text(INI_25E_LIKE)
    fs = 1536000.0  # (the profile's sample_rate: the mains' rate)
    lines = subprocess.check_output([demo, str(profile), "--frames", "3", "--format", "cs16", "--notch", "1000.5,-250000:0.25,0,0.5,50"], text=True).splitlines()
    recs = [ln.split() for ln in lines if ln.startswith("notch ")]
    assert len(recs) == 3 and all(len(r) == 3 + 2 * 9 for r in recs)
    for f, r in enumerate(recs):
        assert r[1] == str(f) and int(r[2]) == nt.blocks(384000) == 94  # (the profile's frames are 384 000 samples)
        for k, hz in enumerate((1000.5, -250000.0)):  # afc_gain 0: the frequencies hold where they were given
            t = r[3 + 9 * k: 12 + 9 * k]
            assert int(t[1], 16) == int(t[2], 16) == sh.inc_of(fs, hz) and float(t[0]) == round(sh.hz_of(fs, sh.inc_of(fs, hz)), 3) and t[6] == "0"
    # the short form: MU alone
    lines = subprocess.check_output([demo, str(profile), "--frames", "1", "--format", "cs16", "--notch", "1000.5:0.5"], text=True).splitlines()
    assert len([ln for ln in lines if ln.startswith("notch ")]) == 1
    # two tones inside the spacing limit are the library's to refuse
    r = subprocess.run([demo, str(profile), "--frames", "1", "--notch", "1000,2000:0.25"], capture_output=True, text=True)
    assert r.returncode == 1 and "notch" in r.stderr
