"""Squelch-gated egress, the part that needs no GPU: the decision rule (squelch.decide), the threshold helper, and the new
symbols of the C ABI in the built library and in the ctypes binding."""
import ctypes as C
import math

import numpy as np

from sdrreceiver_amd import _lib, squelch


def test_threshold_zero_is_always_open():
    assert squelch.decide([0, 0, 5, 0, 2 ** 63], 0, 0).tolist() == [1, 1, 1, 1, 1]
    assert squelch.decide([0, 0], 0, 3).tolist() == [1, 1]


def test_the_threshold_itself_opens_and_one_below_does_not():
    thr = 123456789012345
    assert squelch.decide([thr], thr, 0).tolist() == [1]
    assert squelch.decide([thr - 1], thr, 0).tolist() == [0]
    assert squelch.decide([thr - 1, thr, thr + 1, thr - 1], thr, 0).tolist() == [0, 1, 1, 0]
    assert squelch.decide([2 ** 63 - 1, 2 ** 64 - 1], squelch.NEVER_OPEN, 0).tolist() == [0, 1]  # (exact above 2^53)


def test_hang_times_and_a_retrigger_inside_the_tail():
    s = [9, 0, 0, 0, 0, 0, 9, 0, 9, 0, 0, 0, 0]
    assert squelch.decide(s, 5, 0).tolist() == [1, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0]
    assert squelch.decide(s, 5, 1).tolist() == [1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0]
    flags, left = squelch.decide(s, 5, 3, return_state=True)
    assert flags.tolist() == [1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 0]  # frame 8 re-arms the tail frame 6 started
    assert left.tolist() == [3, 2, 1, 0, 0, 0, 3, 2, 3, 2, 1, 0, 0]
    # a leaf that never reached its threshold has nothing to hang on
    assert squelch.decide([0, 1, 2], 5, 3).tolist() == [0, 0, 0]


def test_a_set_resets_hang_left():
    flags, left = squelch.decide([9, 0], 5, 3, return_state=True)
    assert (flags.tolist(), left.tolist()) == ([1, 1], [3, 2])
    # going on with the state kept: still open; after set_squelch (hang_left = 0): closed at once
    assert squelch.decide([0, 0], 5, 3, hang_left=int(left[-1])).tolist() == [1, 1]
    assert squelch.decide([0, 0], 5, 3, hang_left=0).tolist() == [0, 0]


def test_threshold_is_monotone_and_exact_at_hand_computed_points():
    assert squelch.threshold(0.0, 1000, 32768.0) == 32768 ** 2 * 1000      # full scale: 2^30 per value
    assert squelch.threshold(-20.0, 100, 128.0) == math.ceil(12.8 * 12.8 * 100)  # a tenth of full scale (16384 up to rounding)
    assert abs(squelch.threshold(-20.0, 100, 128.0) - 16384) <= 1
    assert squelch.threshold(-6.020599913279624, 4, 128.0) in (16384, 16385)  # half of full scale: 64^2 * 4
    assert squelch.threshold(-300.0, 1, 128.0) == 1                          # ceil: never 0 ("always open") by accident
    last = 0
    for db in np.arange(-90.0, 0.5, 0.5):
        t = squelch.threshold(float(db), 3000, 32768.0)
        assert t >= last
        last = t
    assert squelch.threshold(-30.0, 6000, 32768.0) >= 2 * squelch.threshold(-30.0, 3000, 32768.0) - 1
    assert squelch.align64(0) == 0 and squelch.align64(1) == 64 and squelch.align64(64) == 64 and squelch.align64(6000) == 6016


def test_the_abi_carries_the_new_symbols_and_keeps_its_version():
    L = _lib.lib()
    assert L.sdrx_abi_version() == 5
    assert C.sizeof(_lib.SquelchStateC) == 32
    for name in ("sdrx_set_squelch", "sdrx_get_squelch", "sdrx_get_egress", "sdrx_group_set_squelch", "sdrx_group_get_squelch",
                 "sdrx_group_get_egress"):
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name) is not None
    assert _lib.NKERNELS == 8
    # without a context every entry point refuses politely
    assert L.sdrx_set_squelch(None, None, None, None, 0) == _lib.SDRX_EINVAL
    assert L.sdrx_get_squelch(None, None, 0, None) == _lib.SDRX_EINVAL
    assert L.sdrx_get_egress(None, None, None, None, None) == _lib.SDRX_EINVAL
