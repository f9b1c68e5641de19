"""The composed model of the ingest chain (tests/chain_ref.py): equal to the stage models applied by hand, told apart from eleven
wrong launch paths by the cases the device is run on, and not vacuous -- the cases hold the hits, the carries, the runs across
workgroup boundaries and the payloads the GPU test's comparisons rest on.  No GPU."""
import numpy as np
import pytest

import adc_ref as ar
import chain_ref as cr
import front_ref as fx
from oracle import binding as ob
from sdrreceiver_amd import blank as bl, front as fr, ingest, resample as rs

BLANKED = [c for c in cr.CASES.values() if c.guard is not None]


def _same(a, b):
    return a.size == b.size and np.array_equal(cr._bits(a), cr._bits(b))


def test_the_chain_is_the_stage_models_applied_by_hand():
    """Case B (DC removal, blanker, one front stage, resampler) and case E (real samples, three stages, resampler), written out"""
    c = cr.CASES["B"]
    h, h_rs, (L, M) = c.front_taps(), c.rs_taps(), c.rs[:2]
    dc, st, hists, rs_hist = np.zeros(2, np.float32), bl.State(), None, None
    for f, ((v, fmt), got) in enumerate(zip(cr.frames(c), cr.model_run(c))):
        iq = ingest.to_float(v)
        ob.dc_correct(iq, dc)
        x = iq.view(np.complex64)
        y, rec, st = bl.apply(x, c.cfg(f), st)
        z, hists = fr.run(y, h, 1, False, hists)
        raw, rs_hist = rs.apply(z, h_rs, L, M, rs_hist)
        assert _same(got.blank_in, x) and _same(got.blank_out, y) and _same(got.front_out, z) and _same(got.raw, raw), f
        assert got.rec == rec and got.adc == ar.model(v, fmt, frame=f), f
        assert raw.size == c.n and z.size == c.n0 and x.size == c.in_frame
    c = cr.CASES["E"]
    h, h_rs, (L, M) = c.front_taps(), c.rs_taps(), c.rs[:2]
    hists, rs_hist = None, None
    for f, ((v, fmt), got) in enumerate(zip(cr.frames(c), cr.model_run(c))):
        assert fmt == (ingest.RS16, ingest.RU12)[f & 1]
        z, hists = fr.run(ingest.to_float(v, fmt), h, 3, True, hists)
        raw, rs_hist = rs.apply(z, h_rs, L, M, rs_hist)
        assert got.blank_in is None and got.blank_out is None and got.rec is None
        assert _same(got.front_out, z) and _same(got.raw, raw) and got.adc == fx.adc_pair_model(v, fmt, frame=f), f
        assert raw.size == c.n and z.size == c.n0


def test_the_workgroup_writing_of_the_blanker_is_the_model():
    for c in BLANKED:
        st = bl.State()
        for f, s in enumerate(cr.model_run(c)):
            y, rec, nxt = cr.blank_by_workgroups(s.blank_in, c.cfg(f), st)
            want = bl.apply(s.blank_in, c.cfg(f), st)
            assert _same(y, want[0]) and rec == want[1] == s.rec and nxt == want[2] and _same(y, s.blank_out), (c.name, f)
            st = nxt


def test_the_cases_have_the_geometry_they_are_named_for():
    wgs = {c.name: -(-c.in_frame // bl.WORKGROUP) for c in BLANKED}
    assert wgs == {"A": 3, "B": 2, "C": 4, "D": 3, "F": 6, "W": 3}
    a = cr.CASES["A"]
    assert bl.WORKGROUP - bl.HALO >= 0 and 2 * bl.WORKGROUP + bl.HALO <= a.in_frame and a.n % 1024 == 320  # the middle workgroup's halos
    d = cr.CASES["D"]
    assert d.in_frame - 2 * bl.WORKGROUP == 32 and d.n0 % 1024 == 16
    c = cr.CASES["C"]
    assert [n % 1024 for _, n in fr.frames(c.n0, c.stages)] == [768, 384, 704] and c.n % 1024 == 272
    assert cr.CASES["B"].K == fr.MAX_K and cr.CASES["E"].rs[0] > cr.CASES["E"].rs[1]
    w = cr.CASES["W"].topo()
    assert len(w.roots()) == 7 and len(w.vfos) == 9 and len(w.children(0)) == 2  # more than the four level 0 reads the frame itself for


@pytest.mark.parametrize("how", cr.WRONG)
def test_every_wrong_device_shows_on_the_case_named_for_it(how):
    c = cr.CASES[cr.CAUGHT_BY[how]]
    assert not cr.same_run(cr.model_run(c, how), cr.model_run(c)), (how, c.name)
    print(how, "caught by", [k.name for k in cr.CASES.values() if not cr.same_run(cr.model_run(k, how), cr.model_run(k))])


@pytest.mark.parametrize("case", BLANKED, ids=[c.name for c in BLANKED])
def test_the_blanker_has_work_in_every_case(case):
    recs = [s.rec for s in cr.model_run(case)]
    assert recs[0]["hits"] == 0 and recs[0]["thr_bits"] == bl.INF_BITS  # frame 0 only sets the reference
    assert sum(r["hits"] > 0 for r in recs) >= 5, [r["hits"] for r in recs]
    assert any(r["carry_in"] > 0 for r in recs), [r["carry_in"] for r in recs]
    for f in range(1, cr.N_FRAMES):
        assert recs[f]["ref_bin"] == recs[f - 1]["next_ref_bin"]
    # the frame whose run crosses 4095 | 4096: fewer runs than clusters counted per workgroup
    f = cr.F_G64_FRAME if case.name == "F" else cr.BOUNDARY_FRAME
    st = bl.State()
    for k, s in enumerate(cr.model_run(case)):
        _, per_wg, nxt = cr.blank_by_workgroups(s.blank_in, case.cfg(k), st, "clusters" if k == f else None)
        if k == f:
            assert s.blank_out[4095] == 0 and s.blank_out[4096] == 0 and s.rec["runs"] < per_wg["runs"], (s.rec, per_wg)
        st = nxt
    if case.name != "F":  # the hand-placed pulses are the hits, and nothing else is
        n, plan = case.in_frame, cr.pulse_plan(case.in_frame, case.guard)
        for k in range(1, cr.N_FRAMES):
            assert recs[k]["hits"] == cr.PULSE_LEN * len(plan[k]), (k, recs[k])
        assert recs[cr.CARRY_FRAME]["carry_in"] == case.guard - case.guard // 2
        assert recs[5]["runs"] == len(plan[5]) and recs[4]["blanked"] == cr.PULSE_LEN + case.guard


def test_case_f_fills_a_workgroup_and_reaches_every_workgroup():
    c = cr.CASES["F"]
    run = cr.model_run(c)
    n = c.in_frame
    thr = np.float32(4.0)
    full = run[cr.F_FULL_FRAME]
    hit = bl.power(full.blank_in) > thr
    assert full.rec["thr_bits"] == bl.thr_bits(thr) and hit[bl.WORKGROUP: 2 * bl.WORKGROUP].all() and int(hit[bl.WORKGROUP: 2 * bl.WORKGROUP].sum()) == 4096
    assert not full.blank_out[bl.WORKGROUP: 2 * bl.WORKGROUP].any()
    assert (full.rec["hits"], full.rec["runs"], full.rec["blanked"]) == (cr.F_RUN[1], 1, cr.F_RUN[1] + 2 * 64)
    g64, g0 = run[cr.F_G64_FRAME].rec, run[cr.F_G0_FRAME].rec
    assert (g64["hits"], g64["runs"], g64["blanked"]) == (6, 3, 3 * (2 + 2 * 64)) and (g0["hits"], g0["runs"], g0["blanked"]) == (6, 3, 6)
    each = run[cr.F_EACH_FRAME]
    hit = bl.power(each.blank_in) > thr
    assert [int(hit[b: b + bl.WORKGROUP].sum()) for b in range(0, n, bl.WORKGROUP)] == [1] * 6 and each.rec["hits"] == 6
    assert len(set(bl.bin_of(bl.power(each.blank_in[hit])).tolist())) == 1  # one histogram bin takes all six
    assert run[6].rec["carry_in"] == 32 and run[7].rec["hits"] == 2


@pytest.mark.parametrize("case", list(cr.CASES.values()), ids=list(cr.CASES))
def test_no_payload_of_the_oracles_tree_is_all_zeros(case):
    topo = case.topo()
    nodes, roots = ob.build_tree("port", topo)
    leaves = [i for i in range(len(topo.vfos)) if not topo.children(i)]
    for f, s in enumerate(cr.model_run(case)):
        assert s.raw.size == topo.frame == case.n
        ob.process_roots(roots, np.ascontiguousarray(s.raw).view(np.float32))
        for i in leaves:
            p = nodes[i].usb() if topo.vfos[i].demod_usb else nodes[i].iq()
            assert p.any(), (case.name, f, i)
