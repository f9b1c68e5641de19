"""Squelch pre-roll (option "preroll"), the part that needs no GPU: the rule (squelch.preroll_flags, next to squelch.decide),
the new symbols of the C ABI in the built library and in the ctypes binding, and that nothing that existed moved."""
import ctypes as C

from sdrreceiver_amd import _lib, squelch


def test_the_first_frame_never_prerolls():
    assert squelch.preroll_flags([1]).tolist() == [0]
    assert squelch.preroll_flags([0]).tolist() == [0]
    assert squelch.preroll_flags([1, 1, 1]).tolist() == [0, 0, 0]
    assert squelch.preroll_flags([]).tolist() == []
    # ... because prev_open starts at 1; a chain that is continued from a closed frame does
    assert squelch.preroll_flags([1], prev_open=0).tolist() == [1]
    assert squelch.preroll_flags([0, 1], prev_open=0).tolist() == [0, 1]


def test_closed_to_open_fires_and_nothing_else_does():
    assert squelch.preroll_flags([0, 1]).tolist() == [0, 1]
    assert squelch.preroll_flags([1, 0]).tolist() == [0, 0]
    assert squelch.preroll_flags([0, 0, 1, 1, 1, 0, 0, 1]).tolist() == [0, 0, 1, 0, 0, 0, 0, 1]
    assert squelch.preroll_flags([1, 0, 1, 0, 1]).tolist() == [0, 0, 1, 0, 1]  # one frame each: every re-open fires


def test_hang_held_frames_do_not_fire_and_a_reopen_after_the_hang_ran_out_does():
    s = [0, 9, 0, 0, 0, 0, 0, 9, 0, 9, 0, 0, 0, 0, 9]
    flags, left = squelch.decide(s, 5, 3, return_state=True)
    assert flags.tolist() == [0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 0, 1]
    assert left.tolist() == [0, 3, 2, 1, 0, 0, 0, 3, 2, 3, 2, 1, 0, 0, 3]
    # frames 2-4 and 8, 10-12 are open on the hang time alone: open -> open, no pre-roll; frame 9 re-arms inside the tail;
    # frames 7 and 14 open after the hang ran out
    assert squelch.preroll_flags(flags).tolist() == [0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1]
    # no hang time: the same levels re-open at frame 9 as well
    assert squelch.preroll_flags(squelch.decide(s, 5, 0)).tolist() == [0, 1, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1]


def test_together_with_decide_over_a_threshold_change():
    """set_squelch resets hang_left and leaves prev_open alone: the chain of `decide` restarts, that of `preroll_flags`
    goes on from the last frame's open flag"""
    s1, s2 = [9, 9, 0, 0], [4, 4, 0, 4]
    f1, l1 = squelch.decide(s1, 5, 2, return_state=True)
    assert (f1.tolist(), l1.tolist()) == ([1, 1, 1, 1], [2, 2, 1, 0])
    p1 = squelch.preroll_flags(f1)
    assert p1.tolist() == [0, 0, 0, 0]
    # threshold lowered to 3 while the leaf is still open on its hang time: it stays open, no pre-roll
    f2 = squelch.decide(s2, 3, 0, hang_left=0)
    assert f2.tolist() == [1, 1, 0, 1]
    assert squelch.preroll_flags(f2, prev_open=int(f1[-1])).tolist() == [0, 0, 0, 1]
    # threshold raised out of reach, then lowered: the leaf was closed in the frame before -> the first open frame fires
    f3 = squelch.decide([9, 9], squelch.NEVER_OPEN, 0)
    assert f3.tolist() == [0, 0]
    assert squelch.preroll_flags(f3, prev_open=int(f2[-1])).tolist() == [0, 0]
    f4 = squelch.decide([9, 9], 5, 0)
    assert squelch.preroll_flags(f4, prev_open=int(f3[-1])).tolist() == [1, 0]
    # `decide` itself is as it was
    assert squelch.decide([9, 0], 5, 3, return_state=True)[1].tolist() == [3, 2]


def test_the_abi_carries_the_new_symbols_and_keeps_its_version_and_structs():
    L = _lib.lib()
    assert L.sdrx_abi_version() == 5
    for name in ("sdrx_get_preroll", "sdrx_get_preroll_count", "sdrx_group_get_preroll", "sdrx_group_get_preroll_count"):
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name) is not None
    assert _lib.NKERNELS == 8
    sq, m = _lib.SquelchStateC, _lib.MeterC
    assert C.sizeof(sq) == 32
    assert [(n, getattr(sq, n).offset) for n, _ in sq._fields_] == [
        ("frame", 0), ("thr_sum_sq", 8), ("hang_frames", 16), ("hang_left", 20), ("open", 24), ("reserved", 28)]
    assert C.sizeof(m) == 32
    assert [(n, getattr(m, n).offset) for n, _ in m._fields_] == [
        ("frame", 0), ("sum_sq", 8), ("n_values", 16), ("clipped", 20), ("peak", 24), ("reserved", 28)]
    # without a context every entry point refuses politely
    assert L.sdrx_get_preroll(None, 0, None, None, None) == _lib.SDRX_EINVAL
    assert L.sdrx_get_preroll_count(None, None, None) == _lib.SDRX_EINVAL
    assert L.sdrx_group_get_preroll(None, 0, None, None, None) == _lib.SDRX_EINVAL
    assert L.sdrx_group_get_preroll_count(None, None, None) == _lib.SDRX_EINVAL
    assert L.sdrx_set_option(None, b"preroll", 1) == _lib.SDRX_EINVAL
