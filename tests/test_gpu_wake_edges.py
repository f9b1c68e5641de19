"""The wake rule on the device at its thresholds (k_watch_wake / wake_hot, csrc/wake.hip) against the plans of
tests/wake_edges_ref.py: `>=` on the band power at equality and one double above, the contrast at the last contrast_q8 that
passes and the next one -- with products contrast_q8 * n_bins past 2^32 --, a leaf whose band is the whole spectrum, min_band_pwr
0, hold_frames 2^32 - 1 and 0, and the restart of hold_left by sdrx_set_wake.  What the plans hold, and that each wrong rule of
wake_edges_ref.WRONG_RULES would give another record, is asserted without a GPU by tests/test_wake_edges_model.py.

Two receivers per case.  Pass A (park, watch, no wake) measures every (frame, leaf) through sdrx_process; the plan is built from
its records.  Pass B runs under the plan: in every fetched frame its wake records, payloads, streams, meters, callbacks and
sdrx_get_active are those of wake_ref.run on pass B's OWN watch figures (test_gpu_wake.check_frame), and every crafted decision
of that frame stands on its condition -- band_pwr == min_band_pwr as doubles, ... -- for pass B's own record.  No tolerance on a
decision or a record; a watch record that did not repeat pass A's fails the crafted decision it carries."""
import functools

import pytest

import wake_edges_ref as er
import wake_ref as kr
from sdrreceiver_amd.receiver import Receiver
from test_gpu_wake import check_frame, drive, make, set_wake

pytestmark = pytest.mark.gpu

_WANT: dict = {}  # (plan, figures as bit patterns) -> wake_ref.run's frames: shared, nobody writes into them


def _figs_of(rx, leaves, f):
    w = rx.watch(leaves)
    assert all(int(v) == f for v in w["frame"]) and all(int(v) == 1 for v in w["watched"]), (f, w)
    return {i: (float(w["band_pwr"][k]), float(w["total_pwr"][k]), int(w["n_bins"][k])) for k, i in enumerate(leaves)}


def pass_a(name, leaves, exact, opts):
    """The watch records of every frame of scenario `name` from a receiver without the wake, every frame fetched."""
    scn = kr.scenario(name)
    rx = Receiver.from_topology(scn.topo, exact=exact, keep_streams=True, meter=True, park=True, watch=True, **opts)
    rx.set_watch(list(leaves), [1] * len(leaves))
    figs = []
    for f, iq in enumerate(scn.frames):
        rx.process(iq)
        figs.append(_figs_of(rx, list(leaves), f))
    rx.close()
    return tuple(figs)


def _want(plan, figs):
    key = (plan.key, tuple(er.bits(row) for row in figs))
    if key not in _WANT:
        _WANT[key] = kr.run(plan.scn, figs=tuple(figs), cfgs=plan.cfgs)
    return _WANT[key]


def run_plan(name, leaves, build, mode, exact=True, **opts):
    figs = list(pass_a(name, sorted(leaves), exact, opts))
    plan = build(tuple(figs))
    scn = plan.scn
    assert scn.controlled == sorted(leaves)
    tag = (plan.key, mode, exact, opts)
    want = [_want(plan, figs)]
    rx = make(scn, exact=exact, **opts)
    crafted_seen = []

    def check(f):
        row = _figs_of(rx, scn.controlled, f)
        if er.bits(row) != er.bits(figs[f]):  # the expectation comes from pass B's own figures
            print("watch record not reproduced", tag, f, er.bits(figs[f]), er.bits(row))
            figs[f] = row
            want[0] = _want(plan, figs)
        check_frame(rx, scn, want[0][f], f, tag, exact)
        for c in plan.crafted:
            if c.frame != f:
                continue
            cfg = er.cfg_at(plan.cfgs, f, c.leaf)
            b, t, n = row[c.leaf]
            k = rx.wake([c.leaf])
            print("crafted", plan.key, mode, "frame", f, "leaf", c.leaf, c.cond, "| min_band_pwr", float(cfg.min_band_pwr).hex(), "contrast_q8",
                  cfg.contrast_q8, "hold_frames", cfg.hold_frames, "| band_pwr", b.hex(), "total_pwr", t.hex(), "n_bins", n, "q8*n", cfg.contrast_q8 * n,
                  "| hot", int(k["hot"][0]), "active", int(k["active"][0]), "hold_left", int(k["hold_left"][0]))
            assert er.holds(c.cond, cfg, b, t, n), (tag, c, "the record does not stand on the crafted condition", cfg, b.hex(), t.hex(), n)
            assert int(k["hot"][0]) == int(c.hot), (tag, c, "decision")
            crafted_seen.append(c)

    before = {f: functools.partial(set_wake, rx, plan.cfgs[f]) for f in plan.cfgs if f}
    seen = drive(rx, scn, mode, check, before=before, fetch_at=plan.fetch_at)
    assert seen == (list(plan.fetch_at) if mode == "device" else list(range(len(scn.frames)))), seen
    assert set(crafted_seen) == {c for c in plan.crafted if c.frame in seen}
    rx.close()
    return plan, want[0]


def _band(name, hold=0):
    return name, er.BAND_LEAVES[name], lambda figs: er.plan_band(name, figs, hold)


def _contrast(name, hold=0):
    return name, [i for i, _ in er.CONTRAST_LEAVES[name]], lambda figs: er.plan_contrast(name, figs, hold)


# 1, 2 and 6.  A queued run (mode "device") leaves crafted frames unfetched: with hold_frames 100 the hold_left of a fetched
# frame tells the last hot frame before it, since_frame the first.
LAUNCH = [("process", 0, dict()), ("submit", 0, dict()), ("device", er.HOLD_LONG, dict()),
          ("submit", 0, dict(pipeline=True)), ("process", 0, dict(fuse=False))]


@pytest.mark.parametrize("mode,hold,opts", LAUNCH, ids=[f"{m}-{'-'.join(f'{a}{int(b)}' for a, b in o.items())}" for m, _, o in LAUNCH])
@pytest.mark.parametrize("name", ["deep", "watch"])
def test_band_power_at_equality_and_one_double_above(name, mode, hold, opts):
    """min_band_pwr == band_pwr: hot; min_band_pwr the next double above band_pwr: cold.  Sources: the raw frame, the main's
    stream and an inner node's ("deep"); USB, fused /5 and compress leaves ("watch"); even and odd frames."""
    run_plan(*_band(name, hold), mode, **opts)


@pytest.mark.parametrize("mode,hold,opts", LAUNCH, ids=[f"{m}-{'-'.join(f'{a}{int(b)}' for a, b in o.items())}" for m, _, o in LAUNCH])
@pytest.mark.parametrize("name", ["deep", "watch"])
def test_contrast_at_the_last_q8_that_passes_and_the_next(name, mode, hold, opts):
    """contrast_q8 == bracket_q8(record): hot; one more: cold.  Tone frames (q8 up to 1.3e8) and quiet frames (q8 near 256); on
    "watch" two of the products contrast_q8 * n_bins are past 2^32, one hot and one cold."""
    plan, _ = run_plan(*_contrast(name, hold), mode, **opts)
    if name == "watch":
        assert {c.hot for c in plan.crafted if c.cond == er.PROD} == {True, False}, plan.crafted


@pytest.mark.parametrize("exact", [False, 2])
@pytest.mark.parametrize("case,name,mode", [("band", "watch", "submit"), ("contrast", "deep", "process"), ("contrast", "watch", "device")])
def test_thresholds_in_the_tolerance_arithmetics(case, name, mode, exact):
    """exact = 0 and 2, both passes in that arithmetic: wake and watch records bit for bit, payloads within 1 LSB."""
    run_plan(*{"band": _band, "contrast": _contrast}[case](name, er.HOLD_LONG if mode == "device" else 0), mode, exact=exact)


# 3
@pytest.mark.parametrize("mode", ["process", "device"])
@pytest.mark.parametrize("contrast_q8", [1, 0])
def test_a_band_that_is_the_whole_spectrum(contrast_q8, mode):
    """n_bins == N: with a contrast condition, however small, never hot -- parked in every frame; without one (and min_band_pwr
    0) hot in every frame, and the leaf's payloads are those of a run without the option (the model's, bit for bit)."""
    plan, want = run_plan("full", (er.FULL_LEAF, er.FULL_USB), lambda figs: er.plan_full(figs, contrast_q8), mode)
    assert all((w["payload"][er.FULL_LEAF] is not None) == (contrast_q8 == 0) for w in want)
    assert all(w["wake"][er.FULL_LEAF]["active"] == (contrast_q8 == 0) for w in want)


# 4
@pytest.mark.parametrize("mode", ["process", "submit"])
def test_min_band_pwr_zero_is_hot_in_every_frame(mode):
    plan, want = run_plan("flat", kr.scenario("flat").controlled, er.plan_always, mode)
    assert all(r["hot"] == 1 and r["active"] == 1 and r["since_frame"] == 0 for w in want for r in w["wake"].values())


# 5
@pytest.mark.parametrize("mode", ["process", "submit", "device"])
def test_hold_frames_at_its_ends_and_the_restart_by_set_wake(mode):
    """hold_frames 2^32 - 1 counts down from 2^32 - 1 and is put back by a hot frame; hold_frames 0 parks at once and hold_left
    stays 0 in a cold frame; a held leaf named by sdrx_set_wake with unchanged settings is parked by the next cold frame, one
    that the batch does not name stays held."""
    U32 = er.U32
    plan, want = run_plan("deep", er.HOLD_FRAMES, er.plan_hold, mode)
    col = lambda i, k: [w["wake"][i][k] for w in want]  # noqa: E731  (what the device was held to, from its own figures)
    assert col(5, "hold_left") == [U32, U32, U32, U32 - 1, U32 - 2, U32 - 3, U32, U32 - 1] and col(5, "active") == [1] * 8
    assert col(4, "hold_left") == [0] * 8 and col(4, "active") == [0, 0, 1, 0, 0, 0, 0, 0]
    assert col(2, "hold_left")[3:6] == [4, 3, 0] and col(2, "active")[3:6] == [1, 1, 0]
    assert col(3, "hold_left")[4:] == [5, 4, 3, 2] and col(3, "active")[4:] == [1, 1, 1, 1]
    assert col(6, "hold_left")[5:] == [5, 4, 0] and col(6, "active")[5:] == [1, 1, 0]
