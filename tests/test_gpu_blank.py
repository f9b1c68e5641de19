"""The impulse blanker on the device (sdrx_set_blanker; k_blank, k_blank_step): the frame that reached it, the frame behind it and
every figure of its record bit for bit sdrreceiver_amd.blank's, whatever the arithmetic, the format and the way the frame is
handed over; the tree behind it bit for bit the oracle's (exact arithmetic) or a twin receiver's without the stage (the two
tolerance arithmetics, where the tree itself is not held to the oracle's bits), each fed the model's frame.

The cases, frames and settings are tests/blank_ref.py's; tests/test_blank_model.py shows that twelve wrong devices each change an
output sample or a record figure on them."""
import ctypes as C

import numpy as np
import pytest

import blank_ref as br
import front_ref as fx
import resample_ref as rr
from helpers import bits
from oracle import binding as ob
from sdrreceiver_amd import _lib, blank as bl, front as fr, ingest, resample as rs
from sdrreceiver_amd.receiver import Group, Receiver, SdrxError
from test_gpu_parity import _check_exact

pytestmark = pytest.mark.gpu

N = br.LENGTHS[-1]  # 4368: a workgroup and a short tile


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


def _check_stage(rx, x, y, rec, cfg, what, raw=None):
    """The stage of the last delivered frame against the model: input, output (the tree's raw frame, or with `raw` what the
    resampler read and made of it), record, settings"""
    got = rx.blanker_input()
    bad = np.flatnonzero(got.view(np.uint64) != np.ascontiguousarray(x).view(np.uint64))
    assert got.size == x.size and bad.size == 0, (what, "blanker input", bad.size, int(bad[0]))
    got = rx.raw() if raw is None else rx.resampler_input()
    bad = np.flatnonzero(got.view(np.uint64) != y.view(np.uint64))
    assert got.size == y.size and bad.size == 0, (what, "output", bad.size, int(bad[0]))
    if raw is not None:
        assert _same(rx.raw(), raw), (what, "raw")
    got = rx.blanker
    assert {k: got[k] for k in bl.RECORD_FIELDS} == rec, (what, got, rec)
    assert got["cfg"] == bl.Cfg(float(np.float32(cfg.ratio)), float(np.float32(cfg.floor)), cfg.rank_q16, cfg.guard), (what, got["cfg"])


def _check_twin(rx, twin, topo, what):
    assert rx.published == twin.published and len(rx.published) == len(_leaves(topo)), (what, "published")
    for i in range(len(topo.vfos)):
        assert _same(rx.stream(i), twin.stream(i)), (what, i, "stream")
    for i in _leaves(topo):
        assert np.array_equal(rx.output(i), twin.output(i)), (what, i, "payload")


# ---- 1. every crafted case, in the three arithmetics ------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [1, 0, 2])
@pytest.mark.parametrize("case", br.crafted(), ids=br.case_ids())
def test_crafted_case(case, exact):
    topo = br.tree(case.n)
    ys, recs, raws = br.model_run(case)
    kw = dict(exact=exact, keep_streams=True)
    rx = Receiver.from_topology(topo, blanker=case.cfgs[0], **br.receiver_kw(case.n), **kw)
    if exact == 1:
        nodes, roots = ob.build_tree("port", topo)
    else:
        twin = Receiver.from_topology(topo, **kw)
    for f, x in enumerate(case.frames):
        if f and case.cfgs[f] != case.cfgs[f - 1]:
            rx.set_blanker(case.cfgs[f])
        rx.process(x.view(np.float32))
        _check_stage(rx, x, ys[f], recs[f], case.cfgs[f], (case.name, exact, f), raws[f] if br.rs_case(case.n) else None)
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
    topo = br.tree(N)
    frames = br.integer_frames(fmt, N)
    rx = Receiver.from_topology(topo, blanker=br.NP_CFG, keep_streams=True, adc_meter=True)
    plain = Receiver.from_topology(topo, adc_meter=True)  # (no blanker: the ADC meter sees the samples as they arrived)
    nodes, roots = ob.build_tree("port", topo)
    dev = _device(frames) if where == "device" else None
    state, st, hits = np.zeros(2, np.float32), bl.State(), 0
    for f, v in enumerate(frames):
        if dev:
            rx.process_device_fmt(dev[f].data_ptr(), N, fmt, correct_dc)
            rx.fetch()
        else:
            rx.process_fmt(v, correct_dc=correct_dc)
        plain.process_fmt(v, correct_dc=correct_dc)
        iq = ingest.to_float(v)
        if correct_dc:
            ob.dc_correct(iq, state)
        x = iq.view(np.complex64)
        y, rec, st = bl.apply(x, br.NP_CFG, st)
        _check_stage(rx, x, y, rec, br.NP_CFG, (fmt, correct_dc, where, f))
        assert rx.adc_meter() == plain.adc_meter()
        ob.process_roots(roots, np.ascontiguousarray(y).view(np.float32))
        _check_exact(rx, nodes, topo, (fmt, correct_dc, where, f))
        hits += rec["hits"]
    assert hits >= 2 * br.NP_PULSES * br.NP_LEN  # (the pulses of frames 1 and 2 at the least: the stage had work)
    rx.close()
    plain.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_cf32_frames(where):
    case = next(c for c in br.crafted() if c.name == f"pairs_n{N}_G17")
    topo = br.tree(N)
    ys, recs, _ = br.model_run(case)
    rx = Receiver.from_topology(topo, blanker=case.cfgs[0], keep_streams=True)
    nodes, roots = ob.build_tree("port", topo)
    dev = _device([x.view(np.float32) for x in case.frames]) if where == "device" else None
    for f, x in enumerate(case.frames):
        if dev:
            rx.process_device(dev[f].data_ptr(), N)
            rx.fetch()
        else:
            rx.process(x.view(np.float32))
        _check_stage(rx, x, ys[f], recs[f], case.cfgs[f], (where, f))
        ob.process_roots(roots, np.ascontiguousarray(ys[f]).view(np.float32))
        _check_exact(rx, nodes, topo, (where, f))
    rx.close()


# ---- 3. frames in flight, frames queued on the device: the state chains without a host call -----------------------------------------
def test_two_frames_in_flight_and_frames_queued_on_the_device():
    topo = br.tree(N)
    frames = br.integer_frames(ingest.CS16, N, seed=3)
    ys, recs = bl.run([ingest.to_float(v).view(np.complex64) for v in frames], br.NP_CFG)
    ref = Receiver.from_topology(topo)  # (no blanker, fed the model's frames)
    want = []
    for y in ys:
        ref.process(y.view(np.float32))
        want.append(list(ref.published))
    ref.close()
    assert all(len(m) == 3 for m in want) and recs[1]["hits"] and recs[2]["hits"]

    rx = Receiver.from_topology(topo, blanker=br.NP_CFG)  # submit_fmt, two frames in flight
    rx.submit_fmt(frames[0])
    rx.submit_fmt(frames[1])
    rx.wait()
    assert rx.published == want[0] and {k: rx.blanker[k] for k in bl.RECORD_FIELDS} == recs[0]
    rx.submit_fmt(frames[2])
    rx.wait()
    assert rx.published == want[1] and {k: rx.blanker[k] for k in bl.RECORD_FIELDS} == recs[1]
    rx.wait()
    assert rx.published == want[2] and {k: rx.blanker[k] for k in bl.RECORD_FIELDS} == recs[2]
    assert _same(rx.raw(), ys[2])
    rx.close()

    dev = _device(frames)  # process_device_fmt queued back to back, one fetch
    rx = Receiver.from_topology(topo, blanker=br.NP_CFG)
    for k in range(br.N_FRAMES):
        rx.process_device_fmt(dev[k].data_ptr(), N, ingest.CS16)
    rx.fetch()
    assert rx.published == want[2] and {k: rx.blanker[k] for k in bl.RECORD_FIELDS} == recs[2]
    assert _same(rx.raw(), ys[2]) and _same(rx.blanker_input(), ingest.to_float(frames[2]).view(np.complex64))
    rx.close()


# ---- 4. in front of a resampler, in front of a complex front stage ------------------------------------------------------------------
def test_in_front_of_the_resampler():
    rcase = rr.CASES[3]  # 16/25, T = 24: 3200 -> 2048
    L, M, T, n_in, n = rcase
    h = rr.random_taps(rcase)
    rx = Receiver.from_topology(rr.tree(rcase), input_rate=rr.rates(rcase)[0], resample_taps=h, blanker=br.NP_CFG)
    st, hist, hits = bl.State(), None, 0
    for f, v in enumerate(br.integer_frames(ingest.CS16, n_in, seed=5)):
        rx.process_fmt(v)
        x = ingest.to_float(v).view(np.complex64)
        y, rec, st = bl.apply(x, br.NP_CFG, st)
        raw, hist = rs.apply(y, h, L, M, hist)
        assert _same(rx.blanker_input(), x) and _same(rx.resampler_input(), y) and _same(rx.raw(), raw), f
        assert {k: rx.blanker[k] for k in bl.RECORD_FIELDS} == rec, f
        hits += rec["hits"]
    assert hits
    rx.close()


def test_in_front_of_a_complex_front_stage():
    case = fx.CASES[2]  # complex, one stage, K = 7: 2560 -> 1280
    real, stages, K, in_frame, n0, n, _ = case
    h = fx.random_taps(case)
    rx = Receiver.from_topology(fx.tree(case), **fx.receiver_kw(case, h), blanker=br.NP_CFG)
    st, hists, hits = bl.State(), None, 0
    for f, v in enumerate(br.integer_frames(ingest.CS8, in_frame, seed=6)):
        rx.process_fmt(v)
        x = ingest.to_float(v).view(np.complex64)
        y, rec, st = bl.apply(x, br.NP_CFG, st)
        raw, hists = fr.run(y, h, stages, False, hists)
        assert _same(rx.blanker_input(), x) and _same(rx.raw(), raw), f
        assert {k: rx.blanker[k] for k in bl.RECORD_FIELDS} == rec, f
        hits += rec["hits"]
    assert hits
    rx.close()


# ---- 5. settings changed between frames -----------------------------------------------------------------------------------------------
def test_set_blanker_between_frames():
    """ratio, floor and guard change; the next frame follows the new settings with the reference the frame before left"""
    topo = br.tree(N)
    frames = br.integer_frames(ingest.CS16, N, seed=9, frames=5)
    cfgs = [br.NP_CFG, br.NP_CFG, bl.Cfg(2.0, 0.0, br.MEDIAN, 8), bl.Cfg(2.0, 5000.0, br.MEDIAN, 8), bl.Cfg(2.0, 5000.0, br.MEDIAN, 33)]
    xs = [ingest.to_float(v).view(np.complex64) for v in frames]
    ys, recs = bl.run(xs, cfgs)
    assert recs[2]["hits"] > recs[1]["hits"] > 0 and recs[3]["hits"] < recs[2]["hits"] and recs[4]["blanked"] > recs[3]["blanked"]
    rx = Receiver.from_topology(topo, blanker=cfgs[0])
    for f, v in enumerate(frames):
        if f and cfgs[f] != cfgs[f - 1]:
            rx.set_blanker(cfgs[f])
        rx.process_fmt(v)
        _check_stage(rx, xs[f], ys[f], recs[f], cfgs[f], f)
        if f:
            assert rx.blanker["ref_bin"] == recs[f - 1]["next_ref_bin"]
    rx.close()


# ---- 6. identity; off means off ----------------------------------------------------------------------------------------------------
def test_a_floor_nothing_reaches_is_the_identity():
    topo = br.tree(N)
    leaves = _leaves(topo)
    kw = dict(meter=True, keep_streams=True)
    rx = Receiver.from_topology(topo, blanker=bl.Cfg(1.0, br.F32_MAX, 1, 64), **kw)
    plain = Receiver.from_topology(topo, **kw)
    for f, v in enumerate(br.integer_frames(ingest.CS16, N, seed=12)):
        for r in (rx, plain):
            r.process_fmt(v, correct_dc=f == 1)
        assert rx.published == plain.published and len(rx.published) == len(leaves)
        assert _same(rx.raw(), plain.raw())
        a, b = rx.meters(leaves), plain.meters(leaves)
        for key in b:
            assert _same(np.atleast_1d(a[key]), np.atleast_1d(b[key])), (f, key)
        _check_twin(rx, plain, topo, f)
        assert (rx.blanker["hits"], rx.blanker["blanked"], rx.blanker["thr_bits"]) == (0, 0, bl.INF_BITS if f == 0 else bl.thr_bits(br.F32_MAX))
    rx.close()
    plain.close()


def test_off_means_off_and_what_on_costs():
    topo = br.tree(N)
    never = Receiver()
    off = Receiver()
    on = Receiver()
    for r in (never, off, on):
        for d in topo.vfos:
            r.add_vfo(d)
    off.set_blanker(br.NP_CFG)
    off.set_blanker(None)
    on.set_blanker(br.NP_CFG)
    for r in (never, off, on):
        r.finalize()
        r.enable_kernel_timing(True)
    assert off.stats()["device_bytes"] == never.stats()["device_bytes"]
    # on: the staging frame in whole tiles plus one, the state (8 words and 2048 counters), two records of 64 bytes
    assert on.stats()["device_bytes"] - never.stats()["device_bytes"] == 8 * (-(-N // 1024) * 1024 + 1024) + 4 * (8 + 2048) + 2 * 64
    v = br.integer_frames(ingest.CS16, N)[0]
    for r in (never, off, on):
        r.process_fmt(v)
    assert off.published == never.published and _same(off.raw(), never.raw())
    assert _launches(off) == _launches(never) == _launches(on)  # (k_blank runs inside the ingest bracket)
    assert off.blanker is None and off.L.sdrx_get_blanker(off.h, C.byref(_lib.BlankerCfgC()), C.byref(_lib.BlankerRecordC())) == _lib.SDRX_ESTATE
    for r in (never, off, on):
        r.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    topo = br.tree(N)
    lib = _lib.lib()
    good = _lib.BlankerCfgC(4.0, 0.0, br.MEDIAN, 8)
    cfg_out, rec_out, buf = _lib.BlankerCfgC(), _lib.BlankerRecordC(), np.zeros(2 * N, np.float32)
    # bad settings, before and after sdrx_finalize
    rx = Receiver()
    for d in topo.vfos:
        rx.add_vfo(d)
    bad = [(0.5, 0.0, 1, 0), (float("inf"), 0.0, 1, 0), (float("nan"), 0.0, 1, 0), (2.0, -1.0, 1, 0), (2.0, float("inf"), 1, 0), (2.0, float("nan"), 1, 0),
           (2.0, 0.0, 0, 0), (2.0, 0.0, 65537, 0), (2.0, 0.0, 1, -1), (2.0, 0.0, 1, 65)]
    for b in bad:
        assert bl.check_cfg(bl.Cfg(*b)) and lib.sdrx_set_blanker(rx.h, C.byref(_lib.BlankerCfgC(*b))) == _lib.SDRX_EINVAL, b
    assert lib.sdrx_get_blanker(rx.h, C.byref(cfg_out), C.byref(rec_out)) == _lib.SDRX_ESTATE  # before sdrx_finalize, and not on
    assert lib.sdrx_set_blanker(rx.h, C.byref(good)) == 0
    rx._blanker = br.cfg(8)
    rx.finalize()
    for b in bad:
        assert lib.sdrx_set_blanker(rx.h, C.byref(_lib.BlankerCfgC(*b))) == _lib.SDRX_EINVAL, b
    assert lib.sdrx_set_blanker(rx.h, None) == _lib.SDRX_ESTATE
    # the getters before a frame
    assert lib.sdrx_get_blanker(rx.h, C.byref(cfg_out), C.byref(rec_out)) == _lib.SDRX_ESTATE
    assert lib.sdrx_get_blanker_input(rx.h, buf.ctypes.data, N) == _lib.SDRX_ESTATE
    assert _code(lambda: rx.process(np.zeros(2 * (N - 16), np.float32))) == _lib.SDRX_EINVAL  # in_frame is the tree's
    rx.process(np.zeros(2 * N, np.float32))
    assert lib.sdrx_get_blanker(rx.h, None, None) == _lib.SDRX_EINVAL and lib.sdrx_get_blanker(rx.h, C.byref(cfg_out), None) == 0
    assert lib.sdrx_get_blanker_input(rx.h, None, N) == _lib.SDRX_EINVAL
    # frames in flight: neither the setter nor the staged frame
    rx.submit(np.zeros(2 * N, np.float32))
    assert lib.sdrx_set_blanker(rx.h, C.byref(good)) == _lib.SDRX_ESTATE and lib.sdrx_get_blanker_input(rx.h, buf.ctypes.data, N) == _lib.SDRX_ESTATE
    rx.wait()
    assert lib.sdrx_set_blanker(rx.h, C.byref(good)) == 0
    # shared frames: neither as the reader nor as the source
    plain = Receiver.from_topology(topo)
    floats = np.zeros(2 * N, np.float32)
    plain.process(floats)
    assert _code(lambda: rx.process_shared(plain)) == _lib.SDRX_ESTATE and _code(lambda: plain.process_shared(rx)) == _lib.SDRX_ESTATE
    assert _code(lambda: rx.submit_shared(plain)) == _lib.SDRX_ESTATE and _code(lambda: plain.submit_shared(rx)) == _lib.SDRX_ESTATE
    assert _code(lambda: plain.process_if_same(rx, floats)) == _lib.SDRX_ESTATE and _code(lambda: rx.submit_if_same(plain, floats)) == _lib.SDRX_ESTATE
    # a context without the stage: the setter after sdrx_finalize, the getters
    assert lib.sdrx_set_blanker(plain.h, C.byref(good)) == _lib.SDRX_ESTATE
    assert lib.sdrx_get_blanker(plain.h, C.byref(cfg_out), C.byref(rec_out)) == _lib.SDRX_ESTATE
    assert lib.sdrx_get_blanker_input(plain.h, buf.ctypes.data, N) == _lib.SDRX_ESTATE
    plain.close()
    rx.close()


def test_a_real_first_front_stage_is_refused_at_finalize():
    case = fx.CASES[0]  # real, one stage
    rx = Receiver(**fx.receiver_kw(case, fx.random_taps(case)), blanker=br.NP_CFG)
    for d in fx.tree(case).vfos:
        rx.add_vfo(d)
    rx._set_front()
    rx.set_blanker(br.NP_CFG)
    assert rx.L.sdrx_finalize(rx.h) == _lib.SDRX_EUNSUPPORTED and b"real first front stage" in rx.L.sdrx_last_error(rx.h)
    rx.close()


def test_a_group_does_not_offer_it():
    g = Group.from_topology(br.tree(N), [0, 0])
    ctx, _ = g.member_context(0)
    assert g.L.sdrx_set_blanker(ctx, C.byref(_lib.BlankerCfgC(4.0, 0.0, br.MEDIAN, 8))) == _lib.SDRX_ESTATE
    assert g.L.sdrx_get_blanker(ctx, C.byref(_lib.BlankerCfgC()), C.byref(_lib.BlankerRecordC())) == _lib.SDRX_ESTATE
    g.close()


# ---- the C++ host layer: sdrj::setBlanker behind sdrx_demo --blanker --------------------------------------------------------------
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
    # a floor nothing reaches: the same messages, and a record per frame whose references chain
    lines = subprocess.check_output([demo, str(profile), "--frames", "3", "--format", "cs16", "--blanker", "1,64,3e38,1"], text=True).splitlines()
    recs = [ln.split() for ln in lines if ln.startswith("blanker ")]
    assert [ln for ln in lines if not ln.startswith("blanker ")] == plain and len(recs) == 3
    assert recs[0][1:4] == ["0", f"{bl.INF_BITS:08x}", "-1"] and all(r[5:] == ["0", "0", "0", "0"] for r in recs)
    for f in (1, 2):
        assert recs[f][1] == str(f) and recs[f][3] == recs[f - 1][4] and recs[f][2] == f"{bl.thr_bits(np.float32(3e38)):08x}"
    # ratio 1 at the lowest occupied bin, no guard: the LCG's components are -8 .. 8, so most samples are above the reference
    lines = subprocess.check_output([demo, str(profile), "--frames", "2", "--format", "cs16", "--blanker", "1,0,0,1"], text=True).splitlines()
    recs = [ln.split() for ln in lines if ln.startswith("blanker ")]
    assert len(recs) == 2 and int(recs[0][5]) == 0 and int(recs[1][5]) > 0 and recs[1][5] == recs[1][6] and int(recs[1][7]) > 0
    # bad settings are the library's to refuse
    r = subprocess.run([demo, str(profile), "--frames", "1", "--blanker", "0.5,8"], capture_output=True, text=True)
    assert r.returncode == 1 and "ratio" in r.stderr
