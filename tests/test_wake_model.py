"""Device-side wake (option "wake"): the ABI additions, the rule (sdrreceiver_amd.wake.step) on hand-worked sequences, and what
makes tests/wake_ref.py a yardstick for tests/test_gpu_wake.py -- the margin of every scheduled decision, the coverage of the
three scenarios, and a list of wrong devices each of which the scenarios tell from the right one.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import live_ref
import wake_ref as kr
from sdrreceiver_amd import _lib, wake
from test_park_model import gate_with_parking

SCENARIOS = ("watch", "deep", "flat")
U32 = 2 ** 32 - 1


def test_the_abi_carries_the_new_symbols_and_keeps_its_version():
    names = ("sdrx_set_wake", "sdrx_get_wake", "sdrx_group_set_wake", "sdrx_group_get_wake")
    for name in names:
        assert name in _lib.SYMBOLS, name
    L = _lib.lib()  # binds every symbol: AttributeError if the library lacks one
    for name in names:
        assert getattr(L, name).argtypes is not None
    assert L.sdrx_abi_version() == 5
    assert C.sizeof(_lib.WakeCfgC) == 32 and C.sizeof(_lib.WakeStateC) == 32
    assert _lib.WakeCfgC.on.offset == 16 and _lib.WakeStateC.hold_left.offset == 24 and _lib.WakeStateC.controlled.offset == 28


def _run(cfg, rows, hold_left=0):
    """(active, hot, hold_left) per row of (band_pwr, total_pwr, n_bins)"""
    out = []
    for b, t, n in rows:
        a, h, hold_left = wake.step(cfg, hold_left, b, t, n)
        out.append((a, h, hold_left))
    return out


HOT, COLD = (1e9, 1e9 + 1e5, 256), (1e3, 1e5, 256)


def test_the_rule_hold_frames_hand_worked():
    rows = [COLD, HOT, COLD, COLD, COLD, HOT, HOT, COLD]
    assert _run(wake.Cfg(1e8, 0, 0), rows) == [(0, 0, 0), (1, 1, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (1, 1, 0), (1, 1, 0), (0, 0, 0)]
    assert _run(wake.Cfg(1e8, 0, 1), rows) == [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 0, 0), (0, 0, 0), (1, 1, 1), (1, 1, 1), (1, 0, 0)]
    assert _run(wake.Cfg(1e8, 0, 2), rows) == [(0, 0, 0), (1, 1, 2), (1, 0, 1), (1, 0, 0), (0, 0, 0), (1, 1, 2), (1, 1, 2), (1, 0, 1)]
    # the longest hold: it counts down from 2^32 - 1, and a hot frame puts it back
    assert _run(wake.Cfg(1e8, 0, U32), [HOT, COLD, COLD, HOT]) == [(1, 1, U32), (1, 0, U32 - 1), (1, 0, U32 - 2), (1, 1, U32)]
    # hold_left left behind by the frame before is honoured in a cold frame, whatever hold_frames says now
    assert wake.step(wake.Cfg(1e8, 0, 0), 3, *COLD) == (1, 0, 2)


def test_the_rule_thresholds_hand_worked():
    # band power: >= is hot, one ulp below is not; 0 is a threshold too (everything is hot, a NaN is not)
    assert wake.step(wake.Cfg(1e8, 0, 0), 0, 1e8, 2e8, 10)[:2] == (1, 1)
    assert wake.step(wake.Cfg(1e8, 0, 0), 0, math.nextafter(1e8, 0.0), 2e8, 10)[:2] == (0, 0)
    assert wake.step(wake.Cfg(0.0, 0, 0), 0, 0.0, 0.0, 10)[:2] == (1, 1)
    assert wake.step(wake.Cfg(0.0, 0, 0), 0, float("nan"), 1.0, 10)[:2] == (0, 0)
    assert wake.step(wake.Cfg(0.0, 256, 0), 0, 1.0, float("nan"), 10)[:2] == (0, 0)
    # contrast: b / n over (t - b) / (N - n) against q8 / 256, without the division.  n = 4096: the band is half the
    # spectrum, contrast = b / (t - b).  q8 = 512 asks for 2: b = 2 (t - b) exactly is hot, the next double below is not
    assert wake.step(wake.Cfg(0.0, 512, 0), 0, 2.0, 3.0, 4096)[:2] == (1, 1)
    assert wake.step(wake.Cfg(0.0, 512, 0), 0, math.nextafter(2.0, 0.0), 3.0, 4096)[:2] == (0, 0)
    # n = 1, N - n = 8191: contrast = 8191 b / (t - b); q8 = 256 * 8191 asks for exactly that with b = t - b
    assert wake.step(wake.Cfg(0.0, 256 * 8191, 0), 0, 5.0, 10.0, 1)[:2] == (1, 1)
    assert wake.step(wake.Cfg(0.0, 256 * 8191 + 1, 0), 0, 5.0, 10.0, 1)[:2] == (0, 0)
    # contrast_q8 = 0: no contrast condition, whatever the figures
    assert wake.step(wake.Cfg(1.0, 0, 0), 0, 1.0, 1e30, 8192)[:2] == (1, 1)
    # n = 8192: the band is the whole spectrum, there is no outside -- with a contrast condition never hot
    assert wake.step(wake.Cfg(0.0, 1, 0), 0, 1e30, 1e30, 8192)[:2] == (0, 0)
    # t < b (the two sums are rounded separately): t - b is negative, the right side too, any b >= 0 passes
    assert wake.step(wake.Cfg(0.0, U32, 0), 0, 1.0, math.nextafter(1.0, 0.0), 8191)[:2] == (1, 1)
    # the largest factors are exact in double: (2^32 - 1) * 8191 < 2^53
    assert float(U32 * 8191) == U32 * 8191 and wake.step(wake.Cfg(0.0, U32, 0), 0, float(U32 * 8191), float(U32 * 8191) + 256.0, 8191)[:2] == (1, 1)


def test_invalid_settings():
    assert wake.invalid(wake.Cfg(0.0)) is None and wake.invalid(wake.Cfg(1e8, U32, U32, 0)) is None
    for bad in (wake.Cfg(-1.0), wake.Cfg(float("nan")), wake.Cfg(float("inf")), wake.Cfg(1.0, on=2), wake.Cfg(1.0, reserved=(0, 1, 0))):
        assert wake.invalid(bad) is not None, bad


@pytest.mark.parametrize("name", SCENARIOS)
def test_no_scheduled_decision_is_near_a_threshold(name):
    """The device's parallel sums (n_terms * 2^-53 relative) and the tolerance arithmetics' slightly different parent streams
    (1e-5) cannot flip a decision that is a factor 4 from its threshold."""
    scn = kr.scenario(name)
    m = kr.margins(scn, kr.figures(name))
    assert m and all(math.isfinite(r) for *_, r in m)
    near = [x for x in m if 1.0 / kr.MARGIN <= x[3] <= kr.MARGIN]
    assert not near, near
    if name == "watch":  # the issue's table: the thresholds separate by more than a factor of 30 on both conditions
        assert all(r < 1 / 30 or r > 30 for *_, r in m), [x for x in m if 1 / 30 <= x[3] <= 30]


def test_every_leaf_kind_wakes_and_parks():
    woke, parked, kinds = set(), set(), set()
    for name in SCENARIOS:
        scn, want = kr.reference(name)
        for i in scn.topo.leaves_in_publish_order():
            kinds |= live_ref.leaf_kinds(scn.topo, i)
        for w in want:
            for i, e in w["events"].items():
                (woke if e == "u" else parked).update(live_ref.leaf_kinds(scn.topo, i))
    assert kinds >= {"usb_plain", "usb_lpf", "late5", "late6", "iq_cstyle0", "iq_cstyle1", "childless_main", "level2", "d0_no_late"}
    assert woke == kinds and parked == kinds, (kinds - woke, kinds - parked)


def test_the_schedules_hold_what_the_issue_lists():
    scn, want = kr.reference("watch")
    ev = {(f, i): e for f, w in enumerate(want) for i, e in w["events"].items()}
    assert ev[(0, 1)] == "u"                                           # a wake in frame 0
    assert ev[(2, 3)] == "u" and (3, 2.5, 4.5) in scn.bursts           # a burst that begins mid-frame: woken in that frame
    assert want[4]["wake"][3]["hot"] and not want[5]["wake"][3]["hot"]  # ... and ends mid-frame 4
    assert want[5]["wake"][3]["active"] and ev[(6, 3)] == "p"          # held one frame, then parked
    assert ev[(7, 6)] == ev[(7, 9)] == "u"                             # two leaves hot in one frame
    assert {f & 1 for (f, i), e in ev.items() if e == "u"} == {0, 1}   # wakes in frames of both parities
    assert ev[(2, 1)] == "p" and ev[(5, 1)] == "u"                     # active with signal, parked, woken again: stale state
    assert all(want[f]["active"][i] for f in range(len(want)) for i in (4, 5, 7, 8))  # the leaves beside them run throughout
    deep, dwant = kr.reference("deep")
    dev = {(f, i): e for f, w in enumerate(dwant) for i, e in w["events"].items()}
    assert deep.topo.vfos[5].parent < 0 and dev[(0, 5)] == "u" and dev[(6, 5)] == "u"  # the parent-less leaf
    assert {live_ref.depth(deep.topo, i) for (f, i), e in dev.items() if e == "u"} == {0, 1, 2}


@pytest.mark.parametrize("wrong", kr.WRONG)
def test_a_wrong_device_is_told_from_the_right_one(wrong):
    """Each wrong device changes at least one scheduled payload, callback or record of some scenario."""
    seen = False
    for name in SCENARIOS:
        scn, want = kr.reference(name)
        other = kr.run(scn, wrong)
        if wrong == "prev_open":  # what the gate makes of the event: pre = open && !prev_open in the frame the leaf wakes
            for i in scn.controlled:
                s = [w["meters"][i]["sum_sq"] for w in want]
                a = gate_with_parking(s, kr.events_of(scn, want, i), 0, 0)
                b = gate_with_parking(s, kr.events_of(scn, other, i), 0, 0)
                seen |= [r["pre"] for r in a] != [r["pre"] for r in b]
        else:
            seen |= kr.differs(want, other)
    assert seen, wrong


def test_a_wake_is_a_fresh_node_on_the_source_of_that_frame():
    """The model's own claim, spelled out once: leaf 3's payload of frame 2 -- the frame its burst begins in -- is that of a
    fresh node fed the main's stream of frame 2."""
    import retune_ref as rr
    scn, want = kr.reference("watch")
    fresh = rr.Node(scn.topo.vfos[3])
    fresh.process(kr.sources("watch")[2][0])
    assert np.array_equal(want[2]["payload"][3], fresh.payload()) and want[1]["payload"][3] is None
    assert np.abs(want[2]["payload"][3].astype(np.int32)).max() > 100  # (the tone is in it)
