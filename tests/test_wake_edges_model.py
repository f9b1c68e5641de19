"""What makes tests/wake_edges_ref.py a yardstick for tests/test_gpu_wake_edges.py, on the model's own figures
(wake_ref.figures): every plan is well formed and every crafted decision stands on the condition it names, sdrreceiver_amd's
rule decides each one as the plan says, and each wrong rule of WRONG_RULES gives another record somewhere.  No GPU."""
import math

import numpy as np
import pytest

import catchup_ref as cu
import live_ref
import wake_edges_ref as er
import wake_ref as kr
import watch_ref as wr
from sdrreceiver_amd import wake

U32 = er.U32


def _plans():
    out = []
    for name in ("deep", "watch"):
        for hold in (0, er.HOLD_LONG):
            out.append(er.plan_band(name, kr.figures(name), hold))
            out.append(er.plan_contrast(name, kr.figures(name), hold))
    out += [er.plan_always(), er.plan_hold(kr.figures("deep")), er.plan_full(None, 1), er.plan_full(None, 0)]
    return out


PLANS = {p.key: p for p in _plans()}
BY_CASE = {"band": [k for k in PLANS if k.startswith("band")], "contrast": [k for k in PLANS if k.startswith("contrast")]}


def _records(key, wrong=None):
    p = PLANS[key]
    return er.decide(p, er.model_figs(p), wrong)


def _differ(a, b, frames=None):
    return [(f, i) for f, (x, y) in enumerate(zip(a, b)) if frames is None or f in frames for i in x if x[i] != y[i]]


def test_bracket_q8_hand_worked():
    # n = 4096: contrast = b / (t - b); b = 2 (t - b): q8 = 512 passes, 513 does not
    assert er.bracket_q8(2.0, 3.0, 4096) == 512
    assert er.bracket_q8(math.nextafter(2.0, 0.0), 3.0, 4096) == 511
    # n = 1: contrast = 8191 b / (t - b)
    assert er.bracket_q8(5.0, 10.0, 1) == 256 * 8191
    # no bracket: q8 = 1 is cold (contrast below 1/256); q8 = 2^32 - 1 is hot (t - b == 0, t < b); n == N is never hot
    assert er.bracket_q8(1.0, 1e6, 4096) is None
    assert er.bracket_q8(1.0, 1.0, 4096) is None and er.bracket_q8(1.0, math.nextafter(1.0, 0.0), 4096) is None
    assert er.bracket_q8(1e30, 1e30, 8192) is None
    # the largest q8 there is: contrast = (2^32 - 2) / 256 exactly
    assert er.bracket_q8(float(U32 - 1), float(U32 - 1) + 256.0, 4096) == U32 - 1


@pytest.mark.parametrize("key", PLANS)
def test_a_plan_is_well_formed(key):
    p = PLANS[key]
    figs = er.model_figs(p)
    n = len(p.scn.frames)
    assert n <= 9 and sorted(p.cfgs)[0] == 0 and all(0 <= f < n for f in p.cfgs)
    for f, row in p.cfgs.items():
        for i, c in row.items():
            assert wake.invalid(c) is None and c.on == 1, (f, i, c)
            assert i in p.scn.topo.leaves_in_publish_order()
    # a queued run fetches the frame before every later setting (sdrx_set_wake needs it delivered), and the last one
    assert all(f - 1 in p.fetch_at for f in p.cfgs if f) and p.fetch_at[-1] == n - 1 and list(p.fetch_at) == sorted(set(p.fetch_at))
    assert p.crafted
    for c in p.crafted:
        cfg = er.cfg_at(p.cfgs, c.frame, c.leaf)
        assert er.holds(c.cond, cfg, *figs[c.frame][c.leaf]), c
        if c.cond in (er.BR, er.BR1):
            q = er.bracket_q8(*figs[c.frame][c.leaf])
            assert q is not None and 1 <= q < U32 - 1, (c, q)
    assert {c.frame & 1 for c in p.crafted} == {0, 1}, "both record parities"
    if key.startswith(("band", "contrast")):
        assert {c.frame & 1 for c in p.crafted if c.hot} == {0, 1} and {c.frame & 1 for c in p.crafted if not c.hot} == {0, 1}
        assert set(range(n)) - set(p.fetch_at) & {c.frame for c in p.crafted}, "a queued run leaves crafted frames unfetched"


@pytest.mark.parametrize("key", PLANS)
def test_every_planned_decision_is_what_the_plan_says(key):
    recs = _records(key)
    for c in PLANS[key].crafted:
        assert recs[c.frame][c.leaf]["hot"] == int(c.hot), c


def test_the_band_cases_cover_every_kind_of_source():
    deep = {c.leaf for c in PLANS["band-deep-0"].crafted}
    topo = cu.deep_tree()
    assert {live_ref.depth(topo, i) for i in deep} == {0, 1, 2}  # the raw frame, the main's stream, the inner node's
    for key in ("band-deep-0", "band-watch-0"):
        for i in {c.leaf for c in PLANS[key].crafted}:
            assert {c.cond for c in PLANS[key].crafted if c.leaf == i} == {er.EQ, er.ABOVE}, (key, i)
    assert {c.leaf for c in PLANS["band-watch-0"].crafted} >= {1, 6, 9}  # USB, fused /5, compress


def test_the_contrast_cases_hold_tone_and_quiet_frames_and_a_product_past_32_bits():
    for name in ("deep", "watch"):
        p = PLANS[f"contrast-{name}-0"]
        qs = [er.cfg_at(p.cfgs, c.frame, c.leaf).contrast_q8 for c in p.crafted if c.cond in (er.BR, er.BR1)]
        assert min(qs) < 512 and max(qs) > 256 * 1000, (name, sorted(qs))  # contrast below 2 and above 1 000
    prod = [c for c in PLANS["contrast-watch-0"].crafted if c.cond == er.PROD]
    assert {c.hot for c in prod} == {True, False}, prod  # (the cold one is the decision a 32-bit product flips)
    figs = er.model_figs(PLANS["contrast-watch-0"])
    for c in prod:
        q, n = er.cfg_at(PLANS["contrast-watch-0"].cfgs, c.frame, c.leaf).contrast_q8, figs[c.frame][c.leaf][2]
        assert q * n >= 2 ** 32 and float(q * n) == q * n


def test_the_full_band_leaf():
    """No tree of the wake tests has an IQ leaf without half-band stages; the one of full_tree() has all 8192 bins."""
    for topo in (wr.watch_tree(), cu.deep_tree(), cu.flat_tree()):
        assert all(wr.band(topo.vfos[i])[1] < er.N for i in topo.leaves_in_publish_order())
    topo = er.full_tree()
    d = topo.vfos[er.FULL_LEAF]
    assert d.parent == 0 and topo.vfos[0].parent < 0 and not d.demod_usb and d.decimate_count == 0
    assert wr.band(d)[1] == 8192 and wr.band(topo.vfos[er.FULL_USB])[1] < 8192
    never, always = _records("full-1"), _records("full-0")
    assert all(r[er.FULL_LEAF]["active"] == 0 and r[er.FULL_LEAF]["hot"] == 0 for r in never)
    assert all(r[er.FULL_LEAF]["active"] == 1 and r[er.FULL_LEAF]["since_frame"] == 0 for r in always)
    assert [r[er.FULL_USB]["hot"] for r in never] == [0, 0, 1, 0]  # (the leaf beside it wakes and parks meanwhile)
    # hot throughout: the leaf's payloads are those of a run without the option
    p = PLANS["full-0"]
    want = kr.run(p.scn, figs=er.model_figs(p), cfgs=p.cfgs)
    plain = live_ref.ModelTree(topo)
    for f, iq in enumerate(p.scn.frames):
        ref = plain.process(iq)["payload"][er.FULL_LEAF]
        assert ref is not None and np.array_equal(want[f]["payload"][er.FULL_LEAF], ref), f
    assert all(w["payload"][er.FULL_LEAF] is None for w in kr.run(PLANS["full-1"].scn, figs=er.model_figs(p), cfgs=PLANS["full-1"].cfgs))


def test_min_band_pwr_zero_is_hot_in_every_frame():
    recs = _records("always-flat")
    scn = PLANS["always-flat"].scn
    assert all(r[i]["hot"] == 1 and r[i]["active"] == 1 for r in recs for i in scn.controlled)
    assert all(r[i]["since_frame"] == 0 for r in recs for i in scn.controlled)  # woken in frame 0 or active from the start
    quiet = kr.figures("flat")[5]
    assert max(b for b, _, _ in quiet.values()) < 1e6  # (frame 5 carries no tone)


def test_the_hold_plan_holds_what_its_comment_says():
    p = PLANS["hold-deep"]
    recs = _records("hold-deep")
    col = lambda i, k: [r[i][k] for r in recs]  # noqa: E731
    for f, row in enumerate(er.model_figs(p)):  # no decision of this plan is near a threshold
        assert all(not 1 / kr.MARGIN <= b / p.cfgs[0][i].min_band_pwr <= kr.MARGIN for i, (b, _, _) in row.items()), f
    assert col(5, "hot") == [1, 1, 1, 0, 0, 0, 1, 0] and col(5, "active") == [1] * 8
    assert col(5, "hold_left") == [U32, U32, U32, U32 - 1, U32 - 2, U32 - 3, U32, U32 - 1]
    assert col(4, "hot") == [0, 0, 1, 0, 0, 0, 0, 0] == col(4, "active") and col(4, "hold_left") == [0] * 8
    assert col(2, "hot") == [1, 1, 1, 0, 0, 0, 1, 0] and col(2, "hold_left") == [5, 5, 5, 4, 3, 0, 5, 4] and col(2, "active") == [1, 1, 1, 1, 1, 0, 1, 1]
    assert col(3, "hot")[4:] == [1, 0, 0, 0] and col(3, "hold_left")[4:] == [5, 4, 3, 2] and col(3, "active")[4:] == [1, 1, 1, 1]
    assert col(6, "hot")[4:] == [1, 1, 0, 0] and col(6, "hold_left")[4:] == [5, 5, 4, 0] and col(6, "active")[4:] == [1, 1, 1, 0]
    assert p.cfgs[5] == {2: p.cfgs[0][2]} and p.cfgs[7] == {6: p.cfgs[0][6]}  # unchanged settings, one leaf named


# Which plans tell a wrong rule apart; in a queued run through the records of the fetched frames alone (HOLD_LONG plans).
TOLD_BY = {"gt": BY_CASE["band"], "f32": BY_CASE["contrast"], "mul32": ["contrast-watch-0", f"contrast-watch-{er.HOLD_LONG}"],
           "no_n_lt_N": ["full-1"], "hold_wrap": ["hold-deep"], "no_hold_reset": ["hold-deep"]}


@pytest.mark.parametrize("wrong", er.WRONG_RULES)
def test_a_wrong_rule_is_told_from_the_right_one(wrong):
    assert set(TOLD_BY) == set(er.WRONG_RULES)
    for key in TOLD_BY[wrong]:
        p = PLANS[key]
        right, other = _records(key), _records(key, wrong)
        assert _differ(right, other), (wrong, key)
        assert _differ(right, other, p.fetch_at), (wrong, key, "not seen in the frames a queued run fetches")
        if wrong in ("gt", "f32", "mul32"):  # ... and in a crafted decision itself
            flipped = [c for c in p.crafted if other[c.frame][c.leaf]["hot"] != int(c.hot)]
            assert flipped, (wrong, key)
    if wrong == "no_hold_reset":  # exactly the two leaves that were named while held
        assert {i for _, i in _differ(_records("hold-deep"), _records("hold-deep", wrong))} == {2, 6}


def test_the_float32_rule_has_another_bracket():
    """Without a planned case whose bracket a float32 evaluation moves by a step or more, the contrast cases would not tell
    the two arithmetics apart."""
    f32 = er.WRONG_RULES["f32"][0]
    for key in BY_CASE["contrast"]:
        p = PLANS[key]
        figs = er.model_figs(p)
        moved = [c for c in p.crafted if c.cond in (er.BR, er.BR1)
                 and er.bracket_q8(*figs[c.frame][c.leaf], step=f32) != er.bracket_q8(*figs[c.frame][c.leaf])]
        assert moved, key
