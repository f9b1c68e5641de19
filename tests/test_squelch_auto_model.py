"""Auto-squelch (option "squelch_auto"), the part that needs no GPU: the rule (squelch.decide_auto, next to squelch.decide) on
hand-built sequences, the dB helper, and the new symbols of the C ABI in the built library and in the ctypes binding."""
import ctypes as C

import pytest

from sdrreceiver_amd import _lib, squelch

NONE = squelch.NONE
Q = 512  # ratio 2.0


def auto(s, thr=0, hang=0, ratio=Q, window=2, **kw):
    return squelch.decide_auto(s, thr, hang, ratio, window, **kw)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def test_ratio_zero_is_decide():
    s = [0, 9, 0, 0, 0, 0, 0, 9, 0, 9, 0, 0, 0, 0, 9]
    for thr, hang in ((5, 3), (5, 0), (0, 2), (squelch.NEVER_OPEN, 1)):
        flags, left = squelch.decide(s, thr, hang, return_state=True)
        for window in (0, 1, 4):  # (no window is needed where the ratio is 0)
            a = auto(s, thr, hang, ratio=0, window=window)
            assert a["open"].tolist() == flags.tolist() and a["hang_left"].tolist() == left.tolist()
            assert a["thr_eff"].tolist() == [thr] * len(s)
    # ... from a starting hang_left too
    a = auto([0, 0, 0], 5, 3, ratio=0, window=1, hang_left=2)
    assert a["open"].tolist() == squelch.decide([0, 0, 0], 5, 3, hang_left=2).tolist() == [1, 1, 0]
    assert auto([], ratio=0)["open"].tolist() == []
    with pytest.raises(ValueError):
        auto([1], ratio=1, window=0)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
def test_the_first_frame_decides_with_thr_then_thr_eff_follows_the_floor():
    a = auto([100, 150, 250, 90, 300], thr=0, ratio=Q, window=10)
    assert a["floor_valid"].tolist() == [0, 1, 1, 1, 1]
    assert a["floor"].tolist() == [0, 100, 100, 100, 90]
    assert a["thr_eff"].tolist() == [0, 200, 200, 200, 180]
    assert a["open"].tolist() == [1, 0, 1, 0, 1]  # frame 0: thr = 0 alone, open
    # a manual threshold decides the first frame, whatever the ratio
    a = auto([100, 100], thr=101, ratio=Q, window=10)
    assert (a["thr_eff"].tolist(), a["open"].tolist(), a["floor_valid"].tolist()) == ([101, 200], [0, 0], [0, 1])
    # the product is shifted, not rounded: floor 3, ratio 257/256 -> 771 >> 8 = 3
    assert auto([3, 3], ratio=257, window=4)["thr_eff"].tolist() == [0, 3]


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_boundary_equal_opens_one_less_does_not():
    for floor, ratio in ((100, 512), (1000, 257), (7, 4096), (1 << 40, 260)):
        eff = (floor * ratio) >> 8
        a = auto([floor, eff], ratio=ratio, window=8)
        assert int(a["thr_eff"][1]) == eff and a["open"].tolist() == [1, 1]
        a = auto([floor, eff - 1], ratio=ratio, window=8)
        assert int(a["thr_eff"][1]) == eff and a["open"].tolist() == [1, 0]


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_window_rotation_against_hand_computed_floors():
    s = [10, 10, 50, 50, 50, 50, 50, 50]
    # window 1: every frame rotates; floor(f) = s(f-1) (cur is always NONE in front of a frame)
    a = auto(s, ratio=Q, window=1)
    assert a["floor"].tolist() == [0, 10, 10, 50, 50, 50, 50, 50]
    assert a["floor_valid"].tolist() == [0, 1, 1, 1, 1, 1, 1, 1]
    # the rise at frame 2 is open against the old floor (50 >= 20), then the level IS the floor and ratio 2 closes it
    assert a["open"].tolist() == [1, 0, 1, 0, 0, 0, 0, 0]
    # window 2: buckets {0,1} {2,3} {4,5} ...; in front of f: prev = the last whole bucket, cur = the running one
    #   f=2: prev {0,1} = 10, cur NONE -> 10 | f=3: min(10, 50) | f=4: prev {2,3} = 50, cur NONE: the old minimum has left
    a = auto(s, ratio=Q, window=2)
    assert a["floor"].tolist() == [0, 10, 10, 10, 50, 50, 50, 50]
    assert a["open"].tolist() == [1, 0, 1, 1, 0, 0, 0, 0]
    # window 3: buckets {0,1,2} {3,4,5} {6,7,..}: 10 stays until {0,1,2} has left BOTH buckets, in front of frame 6
    a = auto(s, ratio=Q, window=3)
    assert a["floor"].tolist() == [0, 10, 10, 10, 10, 10, 50, 50]
    assert a["open"].tolist() == [1, 0, 1, 1, 1, 1, 0, 0]
    # a fall in level is followed at once
    assert auto([50, 50, 50, 10, 50], ratio=Q, window=3)["floor"].tolist() == [0, 50, 50, 50, 10]
    # a burst never lifts its own threshold -- while the frames in front of it are still inside the window, which covers
    # the last window .. 2 * window - 1 frames: a burst that begins with a bucket (frame 3) is open for `window` frames ...
    a = auto([10, 10, 10] + [90] * 5 + [10, 10], ratio=Q, window=3)
    assert a["floor"].tolist() == [0, 10, 10, 10, 10, 10, 90, 90, 90, 10]
    assert a["open"].tolist() == [1, 0, 0, 1, 1, 1, 0, 0, 0, 0]
    # ... one that begins in a bucket's second frame (frame 4) for 2 * window - 1 = 5: a burst of 5 is open to its end
    a = auto([10, 10, 10, 10] + [90] * 5 + [10, 10], ratio=Q, window=3)
    assert a["floor"].tolist() == [0, 10, 10, 10, 10, 10, 10, 10, 10, 90, 10]
    assert a["open"].tolist() == [1, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0]
    # ... and a longer one becomes the floor and closes, wherever it begins
    a = auto([10, 10, 10, 10] + [90] * 8, ratio=Q, window=3)
    assert a["floor"].tolist() == [0, 10, 10, 10, 10, 10, 10, 10, 10, 90, 90, 90]
    assert a["open"].tolist() == [1, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0]


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_a_zero_frame_fails_open_and_recovers():
    s = [100, 100, 100, 0, 100, 100, 100, 100, 100]
    a = auto(s, thr=0, ratio=1024, window=2)
    # buckets {0,1} {2,3} {4,5} {6,7}: the 0 of frame 3 is in the floor in front of frames 4 and 5 -- and 6 and 7 would see it
    # were it in the FIRST frame of its bucket: at most 2 * window - 1 = 3 frames
    assert a["floor"].tolist() == [0, 100, 100, 100, 0, 0, 100, 100, 100]
    assert a["floor_valid"].tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 1]  # a floor of 0 is an observation
    assert a["thr_eff"].tolist() == [0, 400, 400, 400, 0, 0, 400, 400, 400]
    assert a["open"].tolist() == [1, 0, 0, 0, 1, 1, 0, 0, 0]
    worst = auto([100, 100, 0, 100, 100, 100, 100, 100], ratio=1024, window=2)
    assert worst["thr_eff"].tolist() == [0, 400, 400, 0, 0, 0, 400, 400]
    # with a manual threshold the gap does not open anything: thr_eff = thr
    a = auto(s, thr=150, ratio=1024, window=2)
    assert a["thr_eff"].tolist() == [150, 400, 400, 400, 150, 150, 400, 400, 400] and not a["open"].any()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_saturation():
    a = auto([1 << 60, NONE - 1, NONE], ratio=(1 << 32) - 1, window=1)
    assert [int(x) for x in a["thr_eff"]] == [0, NONE, NONE]
    assert a["open"].tolist() == [1, 0, 1]  # only sum_sq = 2^64 - 1 itself reaches a saturated threshold
    # the largest product that still fits: floor * ratio >> 8 = 2^64 - 1 - something, no saturation
    floor = (NONE << 8) // ((1 << 32) - 1)
    eff = (floor * ((1 << 32) - 1)) >> 8
    assert eff <= NONE and int(auto([floor, 0], ratio=(1 << 32) - 1, window=1)["thr_eff"][1]) == eff
    assert int(auto([floor + 1, 0], ratio=(1 << 32) - 1, window=1)["thr_eff"][1]) == NONE


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_the_manual_threshold_is_a_lower_bound():
    s = [100, 250, 150, 250]
    assert auto(s, thr=0, ratio=Q, window=8)["thr_eff"].tolist() == [0, 200, 200, 200]
    assert auto(s, thr=199, ratio=Q, window=8)["thr_eff"].tolist() == [199, 200, 200, 200]
    a = auto(s, thr=251, ratio=Q, window=8)
    assert a["thr_eff"].tolist() == [251] * 4 and a["open"].tolist() == [0, 0, 0, 0]
    assert a["floor"].tolist() == [0, 100, 100, 100]  # the floor is tracked all the same
    # hang time works on thr_eff as it does on thr
    a = auto([100, 250, 150, 150, 150, 150], thr=0, hang=2, ratio=Q, window=8)
    assert a["open"].tolist() == [1, 1, 1, 1, 0, 0] and a["hang_left"].tolist() == [2, 2, 1, 0, 0, 0]


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_reset_and_continuation_through_the_starting_state():
    s = [100, 100, 300, 100, 300, 300, 100]
    whole = auto(s, thr=0, hang=1, ratio=Q, window=2, return_state=True)
    # a chain cut in two and carried on from the returned state is the whole chain
    for cut in range(len(s) + 1):
        a = auto(s[:cut], thr=0, hang=1, ratio=Q, window=2, return_state=True)
        left, cur, prev, age = a["state"]
        b = auto(s[cut:], thr=0, hang=1, ratio=Q, window=2, hang_left=left, cur_min=cur, prev_min=prev, age=age, return_state=True)
        for key in ("open", "hang_left", "thr_eff", "floor", "floor_valid"):
            assert a[key].tolist() + b[key].tolist() == whole[key].tolist(), (cut, key)
        assert b["state"] == whole["state"]
    # set_squelch_auto between frames 3 and 4: the floor restarts, hang_left does not -- frame 4 decides with thr alone
    a = auto(s[:4], thr=150, hang=1, ratio=Q, window=2, return_state=True)
    assert a["open"].tolist() == [0, 0, 1, 1] and a["state"][0] == 0
    b = auto(s[4:], thr=150, hang=1, ratio=1024, window=3, hang_left=a["state"][0])
    assert b["floor_valid"].tolist() == [0, 1, 1] and b["thr_eff"].tolist() == [150, 1200, 1200]
    assert b["open"].tolist() == [1, 1, 0]
    # set_squelch between frames: hang_left restarts at 0, the floor state goes on
    left, cur, prev, age = a["state"]
    c = auto(s[4:], thr=0, hang=0, ratio=Q, window=2, hang_left=0, cur_min=cur, prev_min=prev, age=age)
    assert c["floor"].tolist() == whole["floor"].tolist()[4:] and c["floor_valid"].tolist() == [1, 1, 1]


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
def test_ratio_q8_from_db():
    assert squelch.ratio_q8_from_db(0) == 256
    assert squelch.ratio_q8_from_db(3.0103) == 512
    assert squelch.ratio_q8_from_db(10) == 2560
    assert squelch.ratio_q8_from_db(-10) == 26
    assert squelch.ratio_q8_from_db(-27) == 1
    for db in (-28, -100, 73):  # 0 would mean "off"; 2^32 does not fit
        with pytest.raises(ValueError):
            squelch.ratio_q8_from_db(db)


# ---- 10 --------------------------------------------------------------------------------------------------------------------
def test_the_abi_carries_the_new_symbols_and_keeps_its_version():
    L = _lib.lib()
    assert L.sdrx_abi_version() == 5
    for name in ("sdrx_set_squelch_auto", "sdrx_get_squelch_auto", "sdrx_group_set_squelch_auto", "sdrx_group_get_squelch_auto"):
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name) is not None
    st = _lib.SquelchAutoStateC
    assert C.sizeof(st) == 40
    assert [(n, getattr(st, n).offset) for n, _ in st._fields_] == [
        ("frame", 0), ("floor_sum_sq", 8), ("thr_eff_sum_sq", 16), ("ratio_q8", 24), ("window_frames", 28), ("floor_valid", 32),
        ("reserved", 36)]
    assert C.sizeof(_lib.SquelchStateC) == 32 and C.sizeof(_lib.MeterC) == 32 and _lib.NKERNELS == 8  # nothing that existed moved
    # without a context every entry point refuses politely
    assert L.sdrx_set_squelch_auto(None, None, None, None, 0) == _lib.SDRX_EINVAL
    assert L.sdrx_get_squelch_auto(None, None, 0, None) == _lib.SDRX_EINVAL
    assert L.sdrx_group_set_squelch_auto(None, None, None, None, 0) == _lib.SDRX_EINVAL
    assert L.sdrx_group_get_squelch_auto(None, None, 0, None) == _lib.SDRX_EINVAL
    assert L.sdrx_set_option(None, b"squelch_auto", 1) == _lib.SDRX_EINVAL
    rec = [st(frame=3, floor_sum_sq=7, thr_eff_sum_sq=(1 << 64) - 1, ratio_q8=(1 << 32) - 1, window_frames=2, floor_valid=1)]
    d = squelch.squelch_auto_dict(rec)
    assert {k: int(v[0]) for k, v in d.items()} == {"frame": 3, "floor_sum_sq": 7, "thr_eff_sum_sq": (1 << 64) - 1,
                                                    "ratio_q8": (1 << 32) - 1, "window_frames": 2, "floor_valid": 1}
