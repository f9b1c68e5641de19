"""Parking (sdrx_set_active): the ABI, a pure-Python model of the squelch gate with parking, and the reference of an unparked leaf.

The gate model extends the integer rules of test_squelch_auto_model.py (sdrreceiver_amd.squelch.decide_auto, preroll_flags) by
two sentences: a PARKED frame gives open = 0, pre = 0 and leaves hang_left, prev_open, cur_min, prev_min and age as they are;
an UNPARK puts that state back to what sdrx_finalize leaves (hang_left 0, prev_open 1, no floor observation, age 0) and keeps
the settings.  tests/test_gpu_park.py imports it.

An unparked leaf is the reference's `new vfo`: tests/retune_ref.Node created at that moment.  The last test pins that model to
the plain-C oracle -- a fresh Node fed a parent's streams from frame K equals a fresh oracle node fed the same, bit for bit."""
import dataclasses

import numpy as np

import retune_ref as rr
from oracle import binding as ob
from sdrreceiver_amd import _lib, squelch as sq, synth
from sdrreceiver_amd.topology import Topology, VfoDesc

NONE = sq.NONE


def gate_with_parking(sum_sq, events, thr, hang_frames, ratio_q8=0, window_frames=0):
    """One leaf over the frames of `sum_sq` (python ints; the value of a parked frame is never looked at).  `events[f]`: what
    happens before frame f, a string of 'p' (park), 'u' (unpark) and 'c' (an unpark that catches up, option "catchup": as 'u',
    but prev_open = 0, so that an open frame K pre-rolls the caught-up frame) applied in order -- "pu" restarts the leaf.  Returns one
    dict per frame: active, open, pre, hang_left, prev_open, cur_min, prev_min, age (the state AFTER the frame), thr_eff and
    floor (what decided it; floor NONE = no observation).  `thr` may be a list: the threshold in force in each frame (with
    hang_frames 0, where sdrx_set_squelch's restart of hang_left changes nothing)."""
    thr_of = (lambda f: int(thr[f])) if isinstance(thr, (list, tuple)) else (lambda f: int(thr))
    hang_frames, ratio, window = int(hang_frames), int(ratio_q8), int(window_frames)
    active, left, prev_open, cur, prev, age = 1, 0, 1, NONE, NONE, 0
    out = []
    for f, s in enumerate(sum_sq):
        for e in events.get(f, ""):
            if e == "p":
                active = 0
            elif e in "uc" and not active:
                active, left, prev_open, cur, prev, age = 1, 0, int(e == "u"), NONE, NONE, 0
        floor = min(cur, prev)
        auto = 0 if ratio == 0 or floor == NONE else min(NONE, (floor * ratio) >> 8)
        eff = max(thr_of(f), auto)
        is_open = pre = 0
        if active:
            s = int(s)
            if s >= eff:
                is_open, left = 1, hang_frames
            elif left > 0:
                is_open, left = 1, left - 1
            pre = int(is_open and not prev_open)
            prev_open = is_open
            cur = min(cur, s)
            age += 1
            if age == window:
                prev, cur, age = cur, NONE, 0
        out.append(dict(active=active, open=is_open, pre=pre, hang_left=left, prev_open=prev_open, cur_min=cur, prev_min=prev,
                        age=age, thr_eff=eff, floor=floor))
    return out


def test_the_abi_carries_the_new_symbols_and_keeps_its_version():
    for name in ("sdrx_set_active", "sdrx_get_active", "sdrx_group_set_active", "sdrx_group_get_active"):
        assert name in _lib.SYMBOLS, name
    L = _lib.lib()  # binds every symbol: AttributeError if the library lacks one
    for name in ("sdrx_set_active", "sdrx_get_active", "sdrx_group_set_active", "sdrx_group_get_active"):
        assert getattr(L, name).argtypes is not None
    assert L.sdrx_abi_version() == 5
    import ctypes as C
    assert C.sizeof(_lib.ActiveStateC) == 16


def test_nothing_parked_is_the_plain_rules():
    s = [5, 50, 7, 3, 2, 60, 1, 1, 1, 1]
    got = gate_with_parking(s, {}, thr=40, hang_frames=2)
    flags, lefts = sq.decide(s, 40, 2, return_state=True)
    assert [g["open"] for g in got] == list(flags) and [g["hang_left"] for g in got] == list(lefts)
    assert [g["pre"] for g in got] == list(sq.preroll_flags(flags))
    a = sq.decide_auto(s, 4, 1, 512, 2)
    got = gate_with_parking(s, {}, thr=4, hang_frames=1, ratio_q8=512, window_frames=2)
    assert [g["open"] for g in got] == list(a["open"]) and [g["thr_eff"] for g in got] == [int(v) for v in a["thr_eff"]]
    assert [0 if g["floor"] == NONE else g["floor"] for g in got] == [int(v) for v in a["floor"]]


def test_parked_while_the_hang_time_runs_hand_worked():
    # thr 40, hang 3: frame 1 opens (50), hang_left 3; frame 2 runs it down to 2; parked in 3 and 4: closed, hang_left stays 2;
    # unparked before 5: the state of finalize -- hang_left 0, so a weak frame 5 is closed at once
    got = gate_with_parking([5, 50, 7, 99, 99, 3, 45, 1], {3: "p", 5: "u"}, thr=40, hang_frames=3)
    assert [g["open"] for g in got] == [0, 1, 1, 0, 0, 0, 1, 1]
    assert [g["hang_left"] for g in got] == [0, 3, 2, 2, 2, 0, 3, 2]
    assert [g["active"] for g in got] == [1, 1, 1, 0, 0, 1, 1, 1]


def test_unparked_into_a_frame_that_would_have_prerolled_hand_worked():
    # closed in frame 1 (prev_open 0), parked in 2, unparked before 3 where it opens: prev_open is 1 again -> no pre-roll of the
    # stale payload; without the parking frame 3 would pre-roll
    s = [50, 1, 1, 50, 1, 50]
    got = gate_with_parking(s, {2: "p", 3: "u"}, thr=40, hang_frames=0)
    assert [g["open"] for g in got] == [1, 0, 0, 1, 0, 1]
    assert [g["pre"] for g in got] == [0, 0, 0, 0, 0, 1]
    assert [g["pre"] for g in gate_with_parking(s, {}, thr=40, hang_frames=0)] == [0, 0, 0, 1, 0, 1]
    # park and unpark before the same frame restart the leaf
    got = gate_with_parking(s, {3: "pu"}, thr=40, hang_frames=0)
    assert [g["pre"] for g in got] == [0, 0, 0, 0, 0, 1] and got[3]["active"] == 1


def test_a_parked_frame_is_no_floor_observation_and_threshold_zero_stays_closed_hand_worked():
    # ratio 2.0 (512), window 2: floors after frames 0, 1 = 10, 10 -> rotation: prev 10, cur NONE.  Parked in 2 and 3 (whatever the
    # records hold, here 0): the floor stays 10 -- not 0 --, age stays 0.  Active again in 4 through a restart: no observation.
    got = gate_with_parking([10, 30, 0, 0, 25, 8, 30], {2: "p", 4: "u"}, thr=0, hang_frames=0, ratio_q8=512, window_frames=2)
    assert [g["open"] for g in got] == [1, 1, 0, 0, 1, 0, 1]  # thr 0 and no floor yet: open -- for an active leaf only
    assert [g["floor"] for g in got] == [NONE, 10, 10, 10, NONE, 25, 8]
    assert [g["thr_eff"] for g in got] == [0, 20, 20, 20, 0, 50, 16]
    assert (got[3]["cur_min"], got[3]["prev_min"], got[3]["age"]) == (NONE, 10, 0)
    assert (got[4]["cur_min"], got[4]["prev_min"], got[4]["age"]) == (25, NONE, 1)
    # an unpark of a leaf that is active is ignored: no reset
    same = gate_with_parking([10, 30, 12, 40], {2: "u"}, thr=0, hang_frames=0, ratio_q8=512, window_frames=2)
    assert [g["floor"] for g in same] == [NONE, 10, 10, 10] and same[2]["prev_min"] == 10


def test_a_fresh_model_node_from_frame_k_equals_a_fresh_oracle_node():
    """retune_ref.Node created before frame K and fed the parent's decimate[d] from K on == an oracle node built then and fed
    the same: streams and payloads bit for bit (a d = 2 leaf with the audio low-pass, a /5 late-decimation leaf)."""
    K, n = 2, 4
    cases = [
        (192000, 48000, VfoDesc(parent=-1, fs=192000, decimate_count=2, mixer_freq=-41300.0, filter_bw=10000,
                                gain=float(np.float32(0.03)), cstyle=1, samples_per_buffer=48000, topic="VFO19")),
        (240000, 60000, VfoDesc(parent=-1, fs=240000, decimate_count=0, late_decimate=5, mixer_freq=12000.0, filter_bw=10000,
                                gain=float(np.float32(0.04)), cstyle=1, samples_per_buffer=60000, topic="VFO41")),
    ]
    for fs, frame, desc in cases:
        lcg = synth.Lcg(5)
        frames = [synth.lcg_frame(frame, lcg) for _ in range(n)]
        topo = Topology(fs=fs, frame=frame, vfos=[dataclasses.replace(desc)])
        model = rr.Node(desc)
        onodes, _ = ob.build_tree("port", topo)
        for f in range(K, n):  # both are created "before frame K": neither has seen frames 0 .. K-1
            z = model.process(frames[f].view(np.complex64))
            onodes[0].process(frames[f])
            assert np.array_equal(z.view(np.uint64), onodes[0].stream().view(np.uint64)), (fs, f, "stream")
            assert np.array_equal(model.payload(), onodes[0].usb()), (fs, f, "payload")
