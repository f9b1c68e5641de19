"""The IQ balance correction on the device (sdrx_set_iq_balance; k_iqbal, k_iqbal_step): the frame behind it and every field of
its record bit for bit sdrreceiver_amd.iqbal's, whatever the arithmetic, the format and the way the frame is handed over; the tree
behind it bit for bit the oracle's (exact arithmetic) or a twin receiver's without the stage (the two tolerance arithmetics, where
the tree itself is not held to the oracle's bits), each fed the model's frame.

The cases, frames and settings are tests/iq_ref.py's; tests/test_iq_model.py shows that thirteen wrong devices each change an
output sample or a record field on them."""
import ctypes as C

import numpy as np
import pytest

import blank_ref as br
import front_ref as fx
import iq_ref as ir
import resample_ref as rr
from helpers import bits
from oracle import binding as ob
from sdrreceiver_amd import _lib, blank as bl, front as fr, ingest, iqbal as iq, resample as rs
from sdrreceiver_amd.receiver import Group, Receiver, SdrxError
from test_gpu_parity import _check_exact

pytestmark = pytest.mark.gpu

N = ir.LENGTHS[-1]  # 4368: a workgroup and a short tile
CFG = iq.Cfg(1.0, 0.0)


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
    got = rx.iq_balance
    return {k: got[k] for k in iq.RECORD_FIELDS}


def _cfg32(cfg):
    return iq.Cfg(*(float(np.float32(v)) for v in (cfg.mu, cfg.min_power, cfg.c0, cfg.d0)), cfg.flags)


def _mismatch(got, want, what):
    bad = np.flatnonzero(got.view(np.uint64) != np.ascontiguousarray(want).view(np.uint64))
    assert got.size == want.size and bad.size == 0, (what, bad.size, int(bad[0]))


def _check_stage(rx, y, rec, cfg, what, blanked=None, raw=None):
    """The stage of the last delivered frame against the model: its output -- the blanker's input where one sits behind it (`blanked`:
    what that makes of it), else the resampler's (`raw`: what that makes of it), else the tree's raw frame -- record and settings"""
    if blanked is not None:
        _mismatch(rx.blanker_input(), y, (what, "blanker input"))
        y = blanked
    if raw is not None:
        _mismatch(rx.resampler_input(), y, (what, "resampler input"))
        y = raw
    _mismatch(rx.raw(), y, (what, "raw"))
    got = rx.iq_balance
    assert {k: got[k] for k in iq.RECORD_FIELDS} == rec, (what, got, rec)
    assert got["cfg"] == _cfg32(cfg), (what, got["cfg"])


def _check_twin(rx, twin, topo, what):
    assert rx.published == twin.published and len(rx.published) == len(_leaves(topo)), (what, "published")
    for i in range(len(topo.vfos)):
        assert _same(rx.stream(i), twin.stream(i)), (what, i, "stream")
    for i in _leaves(topo):
        assert np.array_equal(rx.output(i), twin.output(i)), (what, i, "payload")


# ---- 1. every crafted case, in the three arithmetics ------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [1, 0, 2])
@pytest.mark.parametrize("case", ir.crafted(), ids=ir.case_ids())
def test_crafted_case(case, exact):
    topo = ir.tree(case.n)
    ys, recs, zs, raws = ir.model_run(case)
    kw = dict(exact=exact, keep_streams=True)
    rx = Receiver.from_topology(topo, iq_balance=case.cfg, blanker=case.blanker, **ir.receiver_kw(case.n), **kw)
    if exact == 1:
        nodes, roots = ob.build_tree("port", topo)
    else:
        twin = Receiver.from_topology(topo, **kw)
    for f, x in enumerate(case.frames):
        rx.process(x.view(np.float32))
        _check_stage(rx, ys[f], recs[f], case.cfg, (case.name, exact, f), zs[f] if case.blanker else None, raws[f] if ir.rs_case(case.n) else None)
        if exact == 1:
            ob.process_roots(roots, np.ascontiguousarray(raws[f]).view(np.float32))
            _check_exact(rx, nodes, topo, (case.name, f))
        else:
            twin.process(raws[f].view(np.float32))
            _check_twin(rx, twin, topo, (case.name, exact, f))
    rx.close()
    if exact != 1:
        twin.close()


# ---- 2. integer formats, DC removal, host and device frames; cf32 device frames ---------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("correct_dc", [False, True])
@pytest.mark.parametrize("fmt", [ingest.CU8, ingest.CS8, ingest.CS16])
def test_integer_formats_with_and_without_dc_removal(fmt, correct_dc, where):
    topo = ir.tree(N)
    frames = ir.integer_frames(fmt, N)
    rx = Receiver.from_topology(topo, iq_balance=CFG, keep_streams=True, adc_meter=True)
    plain = Receiver.from_topology(topo, adc_meter=True)  # (no stage: the ADC meter sees the samples as they arrived)
    nodes, roots = ob.build_tree("port", topo)
    dev = _device(frames) if where == "device" else None
    state, st = np.zeros(2, np.float32), None
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
        y, rec, st = iq.apply(iqf.view(np.complex64), CFG, st)
        _check_stage(rx, y, rec, CFG, (fmt, correct_dc, where, f))
        assert rx.adc_meter() == plain.adc_meter()
        ob.process_roots(roots, np.ascontiguousarray(y).view(np.float32))
        _check_exact(rx, nodes, topo, (fmt, correct_dc, where, f))
        assert rec["adapted"] == 1
    lv = iq.levels(rec)  # (the pair has moved: the last frame left the stage balanced to what the noise allows)
    assert abs(lv["gain_imbalance"] - 1) < 0.01 and abs(lv["phase_error"]) < 0.01
    rx.close()
    plain.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_cf32_frames(where):
    case = ir.by_name(f"bounds_n{N}")
    topo = ir.tree(N)
    ys, recs, _, _ = ir.model_run(case)
    rx = Receiver.from_topology(topo, iq_balance=case.cfg, keep_streams=True)
    nodes, roots = ob.build_tree("port", topo)
    dev = _device([x.view(np.float32) for x in case.frames]) if where == "device" else None
    for f, x in enumerate(case.frames):
        if dev:
            rx.process_device(dev[f].data_ptr(), N)
            rx.fetch()
        else:
            rx.process(x.view(np.float32))
        _check_stage(rx, ys[f], recs[f], case.cfg, (where, f))
        ob.process_roots(roots, np.ascontiguousarray(ys[f]).view(np.float32))
        _check_exact(rx, nodes, topo, (where, f))
    rx.close()


# ---- 3. frames in flight, frames queued on the device: the pair chains without a host call ------------------------------------------
def test_two_frames_in_flight_and_four_frames_queued_on_the_device():
    topo = ir.tree(N)
    frames = ir.integer_frames(ingest.CS16, N, seed=3)
    ys, recs = iq.run([ingest.to_float(v).view(np.complex64) for v in frames], CFG)
    ref = Receiver.from_topology(topo)  # (no stage, fed the model's frames)
    want = []
    for y in ys:
        ref.process(y.view(np.float32))
        want.append(list(ref.published))
    ref.close()
    assert all(len(m) == 3 for m in want) and all(r["adapted"] for r in recs)
    assert len({(r["c_bits"], r["d_bits"]) for r in recs}) == ir.N_FRAMES  # the pair moves on every frame

    rx = Receiver.from_topology(topo, iq_balance=CFG)  # submit_fmt, two frames in flight
    rx.submit_fmt(frames[0])
    rx.submit_fmt(frames[1])
    rx.wait()
    assert rx.published == want[0] and _rec(rx) == recs[0]
    rx.submit_fmt(frames[2])
    rx.wait()
    assert rx.published == want[1] and _rec(rx) == recs[1]
    rx.submit_fmt(frames[3])
    rx.wait()
    assert rx.published == want[2] and _rec(rx) == recs[2]
    rx.wait()
    assert rx.published == want[3] and _rec(rx) == recs[3]
    assert _same(rx.raw(), ys[3])
    rx.close()

    dev = _device(frames)  # process_device_fmt queued back to back, one fetch: the pair moved across them with no host call
    rx = Receiver.from_topology(topo, iq_balance=CFG)
    for k in range(ir.N_FRAMES):
        rx.process_device_fmt(dev[k].data_ptr(), N, ingest.CS16)
    rx.fetch()
    assert rx.published == want[3] and _rec(rx) == recs[3]
    assert _same(rx.raw(), ys[3])
    rx.close()


# ---- 4. in front of the blanker, of a resampler, of a complex front stage ------------------------------------------------------------
def test_in_front_of_the_blanker():
    topo = ir.tree(N)
    frames = br.integer_frames(ingest.CS16, N, seed=4)  # (noise with pulses near the rails)
    rx = Receiver.from_topology(topo, iq_balance=iq.Cfg(0.25, 0.0, 0.03, 1.1), blanker=br.NP_CFG)
    st, bs, hits = None, bl.State(), 0
    for f, v in enumerate(frames):
        rx.process_fmt(v)
        y, rec, st = iq.apply(ingest.to_float(v).view(np.complex64), iq.Cfg(0.25, 0.0, 0.03, 1.1), st)
        z, brec, bs = bl.apply(y, br.NP_CFG, bs)
        assert _same(rx.blanker_input(), y) and _same(rx.raw(), z), f
        assert _rec(rx) == rec and {k: rx.blanker[k] for k in bl.RECORD_FIELDS} == brec, f
        hits += brec["hits"]
    assert hits
    rx.close()


def test_in_front_of_the_resampler():
    rcase = rr.CASES[3]  # 16/25, T = 24: 3200 -> 2048
    L, M, T, n_in, n = rcase
    h = rr.random_taps(rcase)
    rx = Receiver.from_topology(rr.tree(rcase), input_rate=rr.rates(rcase)[0], resample_taps=h, iq_balance=CFG)
    st, hist = None, None
    for f, v in enumerate(ir.integer_frames(ingest.CS16, n_in, seed=5)):
        rx.process_fmt(v)
        y, rec, st = iq.apply(ingest.to_float(v).view(np.complex64), CFG, st)
        raw, hist = rs.apply(y, h, L, M, hist)
        assert _same(rx.resampler_input(), y) and _same(rx.raw(), raw), f
        assert _rec(rx) == rec, f
    rx.close()


def test_in_front_of_a_complex_front_stage():
    case = fx.CASES[2]  # complex, one stage, K = 7: 2560 -> 1280
    real, stages, K, in_frame, n0, n, _ = case
    h = fx.random_taps(case)
    rx = Receiver.from_topology(fx.tree(case), **fx.receiver_kw(case, h), iq_balance=CFG)
    st, hists = None, None
    for f, v in enumerate(ir.integer_frames(ingest.CS8, in_frame, seed=6)):
        rx.process_fmt(v)
        y, rec, st = iq.apply(ingest.to_float(v).view(np.complex64), CFG, st)
        raw, hists = fr.run(y, h, stages, False, hists)
        assert _same(rx.raw(), raw), f
        assert _rec(rx) == rec, f
    rx.close()


# ---- 5. settings changed between frames -----------------------------------------------------------------------------------------------
def test_set_iq_balance_between_frames_with_and_without_load():
    """mu and min_power change and the pair stays; with SDRX_IQ_LOAD the pair is the caller's, in front of the next frame"""
    topo = ir.tree(N)
    frames = ir.integer_frames(ingest.CS16, N, seed=9, frames=6)
    mu = 2.0 ** -4
    cfgs = [iq.Cfg(1.0, 0.0), iq.Cfg(1.0, 0.0), iq.Cfg(mu, 0.0, 0.4, 1.9), iq.Cfg(mu, 1e6, 0.4, 1.9), iq.Cfg(0.0, 0.0, 0.02, 0.97, iq.IQ_LOAD),
            iq.Cfg(0.5, 0.0, -0.3, 1.2, iq.IQ_LOAD)]
    xs = [ingest.to_float(v).view(np.complex64) for v in frames]
    ys, recs = iq.run(xs, cfgs)
    assert recs[2]["c_bits"] == recs[1]["next_c_bits"] != iq.bits(0.4)                   # without the flag c0, d0 are only checked
    assert recs[3]["measured"] == 0 and recs[3]["next_d_bits"] == recs[3]["d_bits"]      # min_power above the frame's
    assert (recs[4]["c_bits"], recs[4]["d_bits"], recs[4]["adapted"]) == (iq.bits(0.02), iq.bits(0.97), 0)  # loaded and held
    assert (recs[5]["c_bits"], recs[5]["d_bits"], recs[5]["adapted"]) == (iq.bits(-0.3), iq.bits(1.2), 1)
    rx = Receiver.from_topology(topo, iq_balance=cfgs[0])
    loaded = (0.0, 1.0)
    for f, v in enumerate(frames):
        if f and cfgs[f] is not cfgs[f - 1]:
            rx.set_iq_balance(cfgs[f])
            if cfgs[f].flags & iq.IQ_LOAD:
                loaded = (cfgs[f].c0, cfgs[f].d0)
        rx.process_fmt(v)
        told = iq.Cfg(cfgs[f].mu, cfgs[f].min_power, *loaded, cfgs[f].flags)  # (the getter's c0, d0: what sdrx_finalize or the last load wrote)
        _check_stage(rx, ys[f], recs[f], told, f)
    rx.close()


# ---- 6. identity; off means off ----------------------------------------------------------------------------------------------------
def test_hold_at_the_identity_gives_the_inputs_bits():
    """mu = 0 with (c0, d0) = (0, 1): finite frames without a negative zero leave the stage as they came"""
    topo = ir.tree(N)
    leaves = _leaves(topo)
    kw = dict(meter=True, keep_streams=True)
    rx = Receiver.from_topology(topo, iq_balance=iq.Cfg(0.0, 0.0), **kw)
    plain = Receiver.from_topology(topo, **kw)
    for f, v in enumerate(ir.integer_frames(ingest.CS16, N, seed=12)):
        for r in (rx, plain):
            r.process_fmt(v, correct_dc=f == 1)
        assert rx.published == plain.published and len(rx.published) == len(leaves)
        assert _same(rx.raw(), plain.raw())
        a, b = rx.meters(leaves), plain.meters(leaves)
        for key in b:
            assert _same(np.atleast_1d(a[key]), np.atleast_1d(b[key])), (f, key)
        _check_twin(rx, plain, topo, f)
        got = rx.iq_balance
        assert (got["measured"], got["adapted"], got["rejected"], got["next_c_bits"], got["next_d_bits"]) == (1, 0, 0, 0, iq.bits(1.0))
    x = ir.tone(N, 0)  # cf32 as well
    rx.process(x.view(np.float32))
    assert _same(rx.raw(), x)
    rx.close()
    plain.close()


def test_off_means_off_and_what_on_costs():
    topo = ir.tree(N)
    never = Receiver()
    off = Receiver()
    on = Receiver()
    for r in (never, off, on):
        for d in topo.vfos:
            r.add_vfo(d)
    off.set_iq_balance(CFG)
    off.set_iq_balance(None)
    on.set_iq_balance(CFG)
    for r in (never, off, on):
        r.finalize()
        r.enable_kernel_timing(True)
    assert off.stats()["device_bytes"] == never.stats()["device_bytes"]
    # on: the state (the pair, five 64-bit accumulators; 64 bytes) and two records of 96 bytes -- no staging frame, whatever the frame
    assert on.stats()["device_bytes"] - never.stats()["device_bytes"] == iq.STATE_BYTES + 2 * iq.RECORD_BYTES == 256
    v = ir.integer_frames(ingest.CS16, N)[0]
    for r in (never, off, on):
        r.process_fmt(v)
    assert off.published == never.published and _same(off.raw(), never.raw())
    assert _launches(off) == _launches(never) == _launches(on)  # (k_iqbal runs inside the ingest bracket)
    x = ir.tone(N, 1)
    for r in (never, off):
        r.process(x.view(np.float32))
    assert off.published == never.published and _same(off.raw(), never.raw()) and _launches(off) == _launches(never)
    assert off.iq_balance is None and off.L.sdrx_get_iq_balance(off.h, C.byref(_lib.IqCfgC()), C.byref(_lib.IqRecordC())) == _lib.SDRX_ESTATE
    for r in (never, off, on):
        r.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    topo = ir.tree(N)
    lib = _lib.lib()
    good = _lib.IqCfgC(1.0, 0.0, 0.0, 1.0, 0)
    cfg_out, rec_out = _lib.IqCfgC(), _lib.IqRecordC()
    nan, inf = float("nan"), float("inf")
    rx = Receiver()
    for d in topo.vfos:
        rx.add_vfo(d)
    bad = [(-0.1, 0.0, 0.0, 1.0, 0), (1.1, 0.0, 0.0, 1.0, 0), (nan, 0.0, 0.0, 1.0, 0), (0.5, -1.0, 0.0, 1.0, 0), (0.5, inf, 0.0, 1.0, 0), (0.5, nan, 0.0, 1.0, 0),
           (0.5, 0.0, 0.51, 1.0, 0), (0.5, 0.0, -0.51, 1.0, 0), (0.5, 0.0, nan, 1.0, 0), (0.5, 0.0, 0.0, 0.49, 0), (0.5, 0.0, 0.0, 2.01, 0), (0.5, 0.0, 0.0, nan, 0),
           (0.5, 0.0, 0.0, 1.0, 2), (0.5, 0.0, 0.0, 1.0, 0x80000001)]
    reserved = _lib.IqCfgC(1.0, 0.0, 0.0, 1.0, 0)
    reserved.reserved[2] = 1
    for b in bad:
        assert iq.check_cfg(iq.Cfg(*b)) and lib.sdrx_set_iq_balance(rx.h, C.byref(_lib.IqCfgC(*b))) == _lib.SDRX_EINVAL, b
    assert lib.sdrx_set_iq_balance(rx.h, C.byref(reserved)) == _lib.SDRX_EINVAL
    assert lib.sdrx_get_iq_balance(rx.h, C.byref(cfg_out), C.byref(rec_out)) == _lib.SDRX_ESTATE  # before sdrx_finalize, and not on
    assert lib.sdrx_set_iq_balance(rx.h, C.byref(good)) == 0
    rx._iq_balance = CFG
    rx.finalize()
    for b in bad:
        assert lib.sdrx_set_iq_balance(rx.h, C.byref(_lib.IqCfgC(*b))) == _lib.SDRX_EINVAL, b
    assert lib.sdrx_set_iq_balance(rx.h, C.byref(reserved)) == _lib.SDRX_EINVAL
    assert lib.sdrx_set_iq_balance(rx.h, None) == _lib.SDRX_ESTATE
    # the getter before a frame
    assert lib.sdrx_get_iq_balance(rx.h, C.byref(cfg_out), C.byref(rec_out)) == _lib.SDRX_ESTATE
    assert _code(lambda: rx.process(np.zeros(2 * (N - 16), np.float32))) == _lib.SDRX_EINVAL  # in_frame is the tree's
    rx.process(np.zeros(2 * N, np.float32))
    assert lib.sdrx_get_iq_balance(rx.h, None, None) == _lib.SDRX_EINVAL and lib.sdrx_get_iq_balance(rx.h, C.byref(cfg_out), None) == 0
    assert lib.sdrx_get_iq_balance(rx.h, None, C.byref(rec_out)) == 0 and (rec_out.measured, rec_out.n_complex) == (0, N)  # (an all-zero frame: A = 0)
    # frames in flight: not the setter
    rx.submit(np.zeros(2 * N, np.float32))
    assert lib.sdrx_set_iq_balance(rx.h, C.byref(good)) == _lib.SDRX_ESTATE
    rx.wait()
    assert lib.sdrx_set_iq_balance(rx.h, C.byref(good)) == 0
    # shared frames: neither as the reader nor as the source
    plain = Receiver.from_topology(topo)
    floats = np.zeros(2 * N, np.float32)
    plain.process(floats)
    assert _code(lambda: rx.process_shared(plain)) == _lib.SDRX_ESTATE and _code(lambda: plain.process_shared(rx)) == _lib.SDRX_ESTATE
    assert _code(lambda: rx.submit_shared(plain)) == _lib.SDRX_ESTATE and _code(lambda: plain.submit_shared(rx)) == _lib.SDRX_ESTATE
    assert _code(lambda: plain.process_if_same(rx, floats)) == _lib.SDRX_ESTATE and _code(lambda: rx.submit_if_same(plain, floats)) == _lib.SDRX_ESTATE
    # a context without the stage: the setter after sdrx_finalize, the getter
    assert lib.sdrx_set_iq_balance(plain.h, C.byref(good)) == _lib.SDRX_ESTATE
    assert lib.sdrx_get_iq_balance(plain.h, C.byref(cfg_out), C.byref(rec_out)) == _lib.SDRX_ESTATE
    assert lib.sdrx_set_iq_balance(None, C.byref(good)) == _lib.SDRX_EINVAL and lib.sdrx_get_iq_balance(None, C.byref(cfg_out), None) == _lib.SDRX_EINVAL
    plain.close()
    rx.close()


def test_a_real_first_front_stage_is_refused_at_finalize():
    case = fx.CASES[0]  # real, one stage
    rx = Receiver(**fx.receiver_kw(case, fx.random_taps(case)), iq_balance=CFG)
    for d in fx.tree(case).vfos:
        rx.add_vfo(d)
    rx._set_front()
    rx.set_iq_balance(CFG)
    assert rx.L.sdrx_finalize(rx.h) == _lib.SDRX_EUNSUPPORTED and b"real first front stage" in rx.L.sdrx_last_error(rx.h)
    rx.close()


def test_a_group_does_not_offer_it():
    g = Group.from_topology(ir.tree(N), [0, 0])
    ctx, _ = g.member_context(0)
    assert g.L.sdrx_set_iq_balance(ctx, C.byref(_lib.IqCfgC(1.0, 0.0, 0.0, 1.0, 0))) == _lib.SDRX_ESTATE
    assert g.L.sdrx_get_iq_balance(ctx, C.byref(_lib.IqCfgC()), C.byref(_lib.IqRecordC())) == _lib.SDRX_ESTATE
    g.close()


# ---- the C++ host layer: sdrj::setIqBalance behind sdrx_demo --iq-balance -----------------------------------------------------------
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
    # held at the identity: the same messages, and a record per frame
    lines = subprocess.check_output([demo, str(profile), "--frames", "3", "--format", "cs16", "--iq-balance", "0,0"], text=True).splitlines()
    recs = [ln.split() for ln in lines if ln.startswith("iq ")]
    assert [ln for ln in lines if not ln.startswith("iq ")] == plain and len(recs) == 3
    one = f"{iq.bits(1.0):08x}"
    for f, r in enumerate(recs):
        assert r[1:9] == [str(f), "1", "0", "0", "00000000", one, "00000000", one] and int(r[12]) > 0 and int(r[13]) > 0
    # mu = 1 from a calibration: the pair used is the one the frame before left
    lines = subprocess.check_output([demo, str(profile), "--frames", "3", "--format", "cs16", "--iq-balance", "1,0,0.25,1.5"], text=True).splitlines()
    recs = [ln.split() for ln in lines if ln.startswith("iq ")]
    assert len(recs) == 3 and recs[0][5:7] == [f"{iq.bits(0.25):08x}", f"{iq.bits(1.5):08x}"] and recs[0][2:4] == ["1", "1"]
    for f in (1, 2):
        assert recs[f][5:7] == recs[f - 1][7:9]
    assert recs[0][7:9] != recs[0][5:7]
    # bad settings are the library's to refuse
    r = subprocess.run([demo, str(profile), "--frames", "1", "--iq-balance", "1.5,0"], capture_output=True, text=True)
    assert r.returncode == 1 and "mu" in r.stderr
