"""The frequency shift on the device (sdrx_set_shift, shift.hip) against the model sdrreceiver_amd.shift, bit for bit: every
crafted case of tests/shift_ref.py in the three arithmetics; every way a frame is handed over; frames in flight and frames queued on
the device, across which the phase carries without a host call; behind the whole ingest chain and behind a real first front stage;
the increment changed and a phase loaded between frames; the identity, off means off; and the refusals."""
import ctypes as C

import numpy as np
import pytest

import chain_ref as cr
import front_ref as fx
import iq_ref as ir
import shift_ref as sr
from helpers import bits
from oracle import binding as ob
from sdrreceiver_amd import _lib, front as fr, ingest, iqbal as iq, shift as sh
from sdrreceiver_amd.receiver import Group, Receiver, SdrxError
from test_gpu_parity import _check_exact

pytestmark = pytest.mark.gpu

N = sr.LENGTHS[-1]  # 4368: a workgroup and a short tile
CFG = sh.Cfg(3451912, sr.wrap_at(3451912, 4096))  # the 2^32 wrap of frame 0 on the workgroup boundary


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


def _rec(rx):
    got = rx.shift
    return {k: got[k] for k in sh.RECORD_FIELDS}


def _mismatch(got, want, what):
    bad = np.flatnonzero(got.view(np.uint64) != np.ascontiguousarray(want).view(np.uint64))
    assert got.size == want.size and bad.size == 0, (what, bad.size, int(bad[0]))


def _check_stage(rx, y, rec, what, z=None):
    """The stage of the last delivered frame against the model: the tree's raw frame, the record; `z`: what reached the stage from
    a resampler in front (its input is what it was)"""
    _mismatch(rx.raw(), y, (what, "raw"))
    assert _rec(rx) == rec, (what, rx.shift, rec)
    if z is not None:
        assert rx.resampler_input().size == sr.rs_case(4112)[3]


def _check_twin(rx, twin, topo, what):
    assert rx.published == twin.published and len(rx.published) == len(_leaves(topo)), (what, "published")
    for i in range(len(topo.vfos)):
        assert _same(rx.stream(i), twin.stream(i)), (what, i, "stream")
    for i in _leaves(topo):
        assert np.array_equal(rx.output(i), twin.output(i)), (what, i, "payload")


def _set(rx, cfg):
    """sdrx_set_shift between two frames as the case's settings say"""
    rx.set_shift(inc=cfg.inc, phase=cfg.phase0 if cfg.flags & sh.LOAD_PHASE else None)


# ---- 1. every crafted case, in the three arithmetics ------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [1, 0, 2])
@pytest.mark.parametrize("case", sr.crafted(), ids=sr.case_ids())
def test_crafted_case(case, exact):
    topo = sr.tree(case.n)
    zs, ys, recs = sr.model_run(case)
    kw = dict(exact=exact, keep_streams=True)
    rx = Receiver.from_topology(topo, shift=case.cfgs[0], **sr.receiver_kw(case.n), **kw)
    twin = nodes = None
    if case.finite and exact == 1:
        nodes, roots = ob.build_tree("port", topo)
    elif case.finite:
        twin = Receiver.from_topology(topo, **kw)  # (no stage, no resampler: fed the model's shifted frames)
    for f, x in enumerate(case.frames):
        if f and case.cfgs[f] is not case.cfgs[f - 1]:
            _set(rx, case.cfgs[f])
        rx.process(x.view(np.float32))
        _check_stage(rx, ys[f], recs[f], (case.name, exact, f), zs[f] if sr.rs_case(case.n) else None)
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
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("fmt,correct_dc", [(ingest.CU8, True), (ingest.CU8, False), (ingest.CS16, False), (ingest.CS8, True)])
def test_integer_formats_with_and_without_dc_removal(fmt, correct_dc, where):
    topo = sr.tree(N)
    frames = sr.integer_frames(fmt, N)
    rx = Receiver.from_topology(topo, shift=CFG, keep_streams=True, adc_meter=True)
    plain = Receiver.from_topology(topo, adc_meter=True)  # (no stage: the ADC meter sees the samples as they arrived)
    nodes, roots = ob.build_tree("port", topo)
    dev = _device(frames) if where == "device" else None
    state, st = np.zeros(2, np.float32), sh.State.initial(CFG)
    for f, v in enumerate(frames):
        if dev:
            rx.process_device_fmt(dev[f].data_ptr(), N, fmt, correct_dc)
            rx.fetch()
        else:
            rx.process_fmt(v, correct_dc=correct_dc)
        plain.process_fmt(v, correct_dc=correct_dc)
        iqf = ingest.to_float(v)
        if correct_dc:
            ob.dc_correct(iqf, state)
        y, rec, st = sh.apply(iqf.view(np.complex64), st)
        _check_stage(rx, y, rec, (fmt, correct_dc, where, f))
        assert rx.adc_meter() == plain.adc_meter()
        ob.process_roots(roots, np.ascontiguousarray(y).view(np.float32))
        _check_exact(rx, nodes, topo, (fmt, correct_dc, where, f))
    rx.close()
    plain.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_cf32_frames_and_the_callers_buffer_is_never_written(where):
    case = sr.by_name(f"wrap4096_n{N}")
    topo = sr.tree(N)
    _, ys, recs = sr.model_run(case)
    rx = Receiver.from_topology(topo, shift=case.cfgs[0], keep_streams=True)
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


def test_behind_a_real_first_front_stage():
    """RS16 samples through a real first half-band stage: the stage the IQ balance and the blanker cannot sit behind"""
    case = fx.CASES[0]  # real, one stage, K = 2: 2592 real samples -> 1296
    real, stages, K, in_frame, n0, n, _ = case
    h = fx.random_taps(case)
    topo = fx.tree(case)
    cfg = sh.Cfg(0x9E3779B1, sr.wrap_at(3451912, 1024))
    rx = Receiver.from_topology(topo, **fx.receiver_kw(case, h), shift=cfg, keep_streams=True)
    nodes, roots = ob.build_tree("port", topo)
    st, hists = sh.State.initial(cfg), None
    for f in range(sr.N_FRAMES):
        v = fx.full_range(ingest.RS16, in_frame, 700 + f)
        rx.process_fmt(v, fmt=ingest.RS16)
        z, hists = fr.run(fx.to_input(v, ingest.RS16), h, stages, True, hists)
        y, rec, st = sh.apply(z, st)
        _check_stage(rx, y, rec, f)
        ob.process_roots(roots, np.ascontiguousarray(y).view(np.float32))
        _check_exact(rx, nodes, topo, f)
    rx.close()


# ---- 3. frames in flight, frames queued on the device: the phase carries without a host call ----------------------------------------
def test_two_frames_in_flight_and_four_frames_queued_on_the_device():
    topo = sr.tree(N)
    case = sr.by_name(f"advance_wraps_n{N}")
    cfg = case.cfgs[0]
    _, ys, recs = sr.model_run(case)
    frames = [np.array(x.view(np.float32)) for x in case.frames]
    ref = Receiver.from_topology(topo)  # (no stage, fed the model's frames)
    want = []
    for y in ys:
        ref.process(y.view(np.float32))
        want.append(list(ref.published))
    ref.close()
    assert all(len(m) == 3 for m in want) and len({r["phase"] for r in recs}) == sr.N_FRAMES  # the phase moves on every frame

    rx = Receiver.from_topology(topo, shift=cfg)  # sdrx_process: one frame at a time
    for f in range(sr.N_FRAMES):
        rx.process(frames[f])
        assert rx.published == want[f] and _rec(rx) == recs[f]
    rx.close()

    rx = Receiver.from_topology(topo, shift=cfg)  # sdrx_submit / sdrx_wait, two frames in flight
    rx.submit(frames[0])
    rx.submit(frames[1])
    rx.wait()
    assert rx.published == want[0] and _rec(rx) == recs[0]
    rx.submit(frames[2])
    rx.wait()
    assert rx.published == want[1] and _rec(rx) == recs[1]
    rx.submit(frames[3])
    rx.wait()
    assert rx.published == want[2] and _rec(rx) == recs[2]
    rx.wait()
    assert rx.published == want[3] and _rec(rx) == recs[3]
    assert _same(rx.raw(), ys[3])
    rx.close()

    dev = _device(frames)  # sdrx_process_device queued back to back, one sync: the phase moved across them with no host call
    rx = Receiver.from_topology(topo, shift=cfg)
    for k in range(sr.N_FRAMES):
        rx.process_device(dev[k].data_ptr(), N)
    rx.fetch()
    assert rx.published == want[3] and _rec(rx) == recs[3]
    assert _same(rx.raw(), ys[3])
    rx.close()


# ---- 4. behind the whole ingest chain ------------------------------------------------------------------------------------------------
def test_behind_iq_balance_blanker_front_stage_and_resampler():
    """chain_ref's case B -- CS16, the blanker, one complex front stage, the resampler 25 -> 16 -- with the IQ balance in front and
    the shift last: chain_ref's composition of the models, the IQ balance's output handed to it as the converted frame"""
    case = cr.CASES["B"]
    icfg = iq.Cfg(0.25, 0.0, 0.03, 1.1)
    cfg = sh.Cfg(sh.inc_of(4.0 * case.n, -123.4), 0xFEDCBA98)
    kw = dict(case.receiver_kw(), iq_balance=icfg, shift=cfg)
    rx = Receiver.from_topology(case.topo(), **kw)
    nodes, roots = ob.build_tree("port", case.topo())
    chain, ist, st = cr.Chain(case), None, sh.State.initial(cfg)
    hits = 0
    for f, (v, fmt) in enumerate(cr.frames(case)[:4]):
        rx.process_fmt(v)
        x, irec, ist = iq.apply(fx.to_input(v, fmt), icfg, ist)
        s = chain.step(v, fmt, converted=x)
        y, rec, st = sh.apply(s.raw, st)
        assert _same(rx.blanker_input(), s.blank_in) and _same(rx.resampler_input(), s.front_out), f
        assert {k: rx.iq_balance[k] for k in iq.RECORD_FIELDS} == irec and {k: rx.blanker[k] for k in s.rec} == s.rec, f
        _check_stage(rx, y, rec, f)
        assert rec["n_complex"] == case.n != case.in_frame
        ob.process_roots(roots, np.ascontiguousarray(y).view(np.float32))
        _check_exact(rx, nodes, case.topo(), f)
        hits += s.rec["hits"]
    assert hits
    rx.close()


# ---- 5. the increment changed and a phase loaded between frames ------------------------------------------------------------------------
def test_set_shift_between_frames_in_hz_and_with_a_phase():
    """The increment changes and the phase carries on; with a phase it is the caller's, in front of the next frame.  The getter
    tells what the frame ran with."""
    topo = sr.tree(N)
    fs = float(topo.vfos[0].fs)
    frames = sr.integer_frames(ingest.CS16, N, seed=9, frames=6)
    hz = [100.0, 100.0, -2500.25, -2500.25, 0.4, fs / 2]
    rx = Receiver.from_topology(topo, shift=hz[0])
    assert rx.tree_rate == fs
    st, loaded = sh.State(0, sh.inc_of(fs, hz[0]), 0), 0
    for f, v in enumerate(frames):
        if f and hz[f] != hz[f - 1]:
            phase = 0x80000001 if f == 4 else None
            rx.set_shift(hz=hz[f], phase=phase)
            st = sh.load(st, sh.Cfg(sh.inc_of(fs, hz[f]), phase or 0, sh.LOAD_PHASE if phase is not None else 0))
            loaded = phase if phase is not None else loaded
        rx.process_fmt(v)
        before = st
        y, rec, st = sh.apply(ingest.to_float(v).view(np.complex64), st)
        _check_stage(rx, y, rec, f)
        got = rx.shift
        assert got["cfg"].inc == before.inc and got["cfg"].phase0 == loaded and got["hz"] == sh.hz_of(fs, before.inc), (f, got)
        if f in (2, 5):
            assert rec["phase"] == prev["next_phase"] and rec["inc"] != prev["next_inc"]  # the phase carried on across the change
        if f == 4:
            assert rec["phase"] == 0x80000001 != prev["next_phase"]
        prev = rec
    rx.close()


# ---- 6. identity; the three arithmetics; off means off ---------------------------------------------------------------------------------
def test_zero_shift_gives_the_inputs_bits():
    topo = sr.tree(N)
    leaves = _leaves(topo)
    kw = dict(meter=True, keep_streams=True)
    rx = Receiver.from_topology(topo, shift=0.0, **kw)
    plain = Receiver.from_topology(topo, **kw)
    for f, v in enumerate(sr.integer_frames(ingest.CS16, N, seed=12)):
        for r in (rx, plain):
            r.process_fmt(v, correct_dc=f == 1)
        assert rx.published == plain.published and len(rx.published) == len(leaves)
        assert _same(rx.raw(), plain.raw())
        a, b = rx.meters(leaves), plain.meters(leaves)
        for key in b:
            assert _same(np.atleast_1d(a[key]), np.atleast_1d(b[key])), (f, key)
        _check_twin(rx, plain, topo, f)
        assert _rec(rx) == {"frame": f, "n_complex": N, "applied": 1, "phase": 0, "inc": 0, "next_phase": 0, "next_inc": 0}
    rx.close()
    plain.close()


def test_the_stage_is_the_same_in_the_three_arithmetics():
    case = sr.by_name(f"inc9e3779b1_n{N}")
    raws = []
    for exact in (1, 0, 2):
        rx = Receiver.from_topology(sr.tree(N), shift=case.cfgs[0], exact=exact)
        out = []
        for x in case.frames:
            rx.process(x.view(np.float32))
            out.append((rx.raw().copy(), _rec(rx)))
        raws.append(out)
        rx.close()
    for other in raws[1:]:
        for (a, ra), (b, rb) in zip(raws[0], other):
            assert _same(a, b) and ra == rb


def test_off_means_off_and_what_on_costs():
    topo = sr.tree(N)
    never, off, on = Receiver(), Receiver(), Receiver()
    for r in (never, off, on):
        for d in topo.vfos:
            r.add_vfo(d)
    off.set_shift(hz=1000.0)
    off.set_shift(off=True)
    on.set_shift(inc=CFG.inc, phase=CFG.phase0)
    for r in (never, off, on):
        r.finalize()
        r.enable_kernel_timing(True)
    assert off.stats()["device_bytes"] == never.stats()["device_bytes"]
    # on: the state (16 bytes), the one copy of the three tables (6 KiB) and two records of 64 bytes -- no staging frame, whatever the frame
    assert on.stats()["device_bytes"] - never.stats()["device_bytes"] == sh.STATE_BYTES + sh.TABLE_BYTES + 2 * sh.RECORD_BYTES == 6288
    v = sr.integer_frames(ingest.CS16, N)[0]
    for r in (never, off, on):
        r.process_fmt(v)
    assert off.published == never.published and _same(off.raw(), never.raw())
    assert _launches(off) == _launches(never) == _launches(on)  # (k_shift runs inside the ingest bracket)
    x = ir.tone(N, 1)
    for r in (never, off):
        r.process(x.view(np.float32))
    assert off.published == never.published and _same(off.raw(), never.raw()) and _launches(off) == _launches(never)
    assert off.shift is None and off.L.sdrx_get_shift(off.h, C.byref(_lib.ShiftCfgC()), C.byref(_lib.ShiftRecordC())) == _lib.SDRX_ESTATE
    for r in (never, off, on):
        r.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    topo = sr.tree(N)
    lib = _lib.lib()
    good = _lib.ShiftCfgC(12345, 0, 0)
    cfg_out, rec_out = _lib.ShiftCfgC(), _lib.ShiftRecordC()
    rx = Receiver()
    for d in topo.vfos:
        rx.add_vfo(d)
    bad = [(1, 0, 2), (1, 0, 3), (1, 0, 0x80000000), (1, 0, 0x80000001)]
    reserved = _lib.ShiftCfgC(1, 0, 0)
    reserved.reserved[4] = 1
    for b in bad:
        assert sh.check_cfg(sh.Cfg(*b)) and lib.sdrx_set_shift(rx.h, C.byref(_lib.ShiftCfgC(*b))) == _lib.SDRX_EINVAL, b
    assert lib.sdrx_set_shift(rx.h, C.byref(reserved)) == _lib.SDRX_EINVAL
    assert lib.sdrx_get_shift(rx.h, C.byref(cfg_out), C.byref(rec_out)) == _lib.SDRX_ESTATE  # before sdrx_finalize, and not on
    assert lib.sdrx_set_shift(rx.h, C.byref(good)) == 0
    rx._shift = sh.Cfg(12345)
    rx.finalize()
    for b in bad:
        assert lib.sdrx_set_shift(rx.h, C.byref(_lib.ShiftCfgC(*b))) == _lib.SDRX_EINVAL, b
    assert lib.sdrx_set_shift(rx.h, C.byref(reserved)) == _lib.SDRX_EINVAL
    assert lib.sdrx_set_shift(rx.h, None) == _lib.SDRX_ESTATE
    with pytest.raises(ValueError):
        rx.set_shift(hz=rx.tree_rate)  # beyond half the rate
    with pytest.raises(ValueError):
        rx.set_shift()
    # the getter before a frame
    assert lib.sdrx_get_shift(rx.h, C.byref(cfg_out), C.byref(rec_out)) == _lib.SDRX_ESTATE
    assert _code(lambda: rx.process(np.zeros(2 * (N - 16), np.float32))) == _lib.SDRX_EINVAL  # in_frame is the tree's
    rx.process(np.zeros(2 * N, np.float32))
    assert lib.sdrx_get_shift(rx.h, None, None) == _lib.SDRX_EINVAL and lib.sdrx_get_shift(rx.h, C.byref(cfg_out), None) == 0
    assert lib.sdrx_get_shift(rx.h, None, C.byref(rec_out)) == 0 and (rec_out.applied, rec_out.n_complex, rec_out.inc) == (1, N, 12345)
    # frames in flight: not the setter
    rx.submit(np.zeros(2 * N, np.float32))
    assert lib.sdrx_set_shift(rx.h, C.byref(good)) == _lib.SDRX_ESTATE
    rx.wait()
    assert lib.sdrx_set_shift(rx.h, C.byref(good)) == 0
    # shared frames: neither as the reader nor as the source
    plain = Receiver.from_topology(topo)
    floats = np.zeros(2 * N, np.float32)
    plain.process(floats)
    assert _code(lambda: rx.process_shared(plain)) == _lib.SDRX_ESTATE and _code(lambda: plain.process_shared(rx)) == _lib.SDRX_ESTATE
    assert _code(lambda: rx.submit_shared(plain)) == _lib.SDRX_ESTATE and _code(lambda: plain.submit_shared(rx)) == _lib.SDRX_ESTATE
    assert _code(lambda: plain.process_if_same(rx, floats)) == _lib.SDRX_ESTATE and _code(lambda: rx.submit_if_same(plain, floats)) == _lib.SDRX_ESTATE
    # a context without the stage: the setter after sdrx_finalize, the getter
    assert lib.sdrx_set_shift(plain.h, C.byref(good)) == _lib.SDRX_ESTATE
    assert lib.sdrx_get_shift(plain.h, C.byref(cfg_out), C.byref(rec_out)) == _lib.SDRX_ESTATE
    assert lib.sdrx_set_shift(None, C.byref(good)) == _lib.SDRX_EINVAL and lib.sdrx_get_shift(None, C.byref(cfg_out), None) == _lib.SDRX_EINVAL
    plain.close()
    rx.close()


def test_a_group_does_not_offer_it():
    g = Group.from_topology(sr.tree(N), [0, 0])
    ctx, _ = g.member_context(0)
    assert g.L.sdrx_set_shift(ctx, C.byref(_lib.ShiftCfgC(1, 0, 0))) == _lib.SDRX_ESTATE
    assert g.L.sdrx_get_shift(ctx, C.byref(_lib.ShiftCfgC()), C.byref(_lib.ShiftRecordC())) == _lib.SDRX_ESTATE
    g.close()


# ---- the C++ host layer: sdrj::setShift behind sdrx_demo --shift -----------------------------------------------------------------------
def test_demo_prints_the_record(tmp_path):
    import os
    import subprocess
    from test_topology import INI_25E_LIKE
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    demo = os.path.join(root, "host", "sdrx_demo")
    subprocess.check_call(["make", "-C", os.path.join(root, "host")], stdout=subprocess.DEVNULL)
    profile = tmp_path / "profile.ini"
    profile.write_text(INI_25E_LIKE)
    plain = subprocess.check_output([demo, str(profile), "--frames", "3", "--format", "cs16"], text=True).splitlines()
    # a shift of zero: the same messages, and a record per frame
    lines = subprocess.check_output([demo, str(profile), "--frames", "3", "--format", "cs16", "--shift", "0"], text=True).splitlines()
    recs = [ln.split() for ln in lines if ln.startswith("shift ")]
    assert [ln for ln in lines if not ln.startswith("shift ")] == plain and recs == [["shift", str(f)] + ["00000000"] * 4 for f in range(3)]
    # a shift in Hz: the increment is the conversion's, the phase chains
    lines = subprocess.check_output([demo, str(profile), "--frames", "3", "--format", "cs16", "--shift", "-1234.5"], text=True).splitlines()
    recs = [ln.split() for ln in lines if ln.startswith("shift ")]
    assert len(recs) == 3 and recs[0][2] == "00000000" and len({r[3] for r in recs} | {r[5] for r in recs}) == 1
    assert int(recs[0][3], 16) == sh.inc_of(1536000.0, -1234.5)  # (the profile's sample_rate: the mains' rate)
    for f in (1, 2):
        assert recs[f][2] == recs[f - 1][4]
    # a shift beyond half the rate is the library's to refuse
    r = subprocess.run([demo, str(profile), "--frames", "1", "--shift", "1e9"], capture_output=True, text=True)
    assert r.returncode == 1 and "shift" in r.stderr
