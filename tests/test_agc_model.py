"""Option "agc" without a GPU: the rule of sdrreceiver_amd.agc.step on hand-built boundary cases, what the closed loop on the
model trees (tests/agc_ref.py) covers -- which is what tests/test_gpu_agc.py relies on -- and the binding."""
import ctypes as C

import numpy as np
import pytest

import agc_ref as ar
from sdrreceiver_amd import agc

CFG = agc.Cfg(lo_ms=100, hi_ms=400, silent_ms=10, hold_frames=0, up=2.0, down=0.5, gain_min=0.015625, gain_max=100.0)  # (every float exact in fp32)
N = 1000


def _m(ms_times_n, clipped=0, n=N):
    return {"sum_sq": int(ms_times_n), "n_values": n, "clipped": clipped}


def _step(cfg, q, g, m, parked=False):
    g2, q2, a = agc.step(cfg, q, g, m, parked)
    assert isinstance(g2, np.float32)
    return float(g2), q2, a


def test_window_boundaries():
    """s == hi_ms * n is not hot, one more is; s == lo_ms * n is not cold, one less is; s == silent_ms * n is cold, not silent."""
    assert _step(CFG, 3, 1.0, _m(400 * N)) == (1.0, 0, 0)
    assert _step(CFG, 3, 1.0, _m(400 * N + 1)) == (0.5, 0, -1)
    assert _step(CFG, 3, 1.0, _m(100 * N)) == (1.0, 0, 0)
    assert _step(CFG, 3, 1.0, _m(100 * N - 1)) == (2.0, 4, 1)
    assert _step(CFG, 3, 1.0, _m(10 * N)) == (2.0, 4, 1)
    assert _step(CFG, 3, 1.0, _m(10 * N - 1)) == (1.0, 3, 0)


def test_clipped_is_hot_whatever_the_sum():
    assert _step(CFG, 5, 1.0, _m(0, clipped=1)) == (0.5, 0, -1)
    assert _step(CFG, 5, 1.0, _m(50 * N, clipped=7)) == (0.5, 0, -1)


@pytest.mark.parametrize("hold", [0, 1, 3])
def test_hold_frames(hold):
    """The gain rises in the cold frame that makes quiet_run exceed hold_frames, and in every cold frame after it."""
    import dataclasses
    cfg = dataclasses.replace(CFG, hold_frames=hold)
    q, g, actions = 0, 1.0, []
    for _ in range(hold + 3):
        g, q, a = _step(cfg, q, g, _m(50 * N))
        actions.append(a)
    assert actions == [0] * hold + [1, 1, 1] and q == hold + 3 and g == 8.0


def test_silent_keeps_and_in_window_resets_quiet_run():
    assert _step(CFG, 2, 1.0, _m(5 * N)) == (1.0, 2, 0)
    assert _step(CFG, 2, 1.0, _m(200 * N)) == (1.0, 0, 0)
    assert _step(CFG, agc.QUIET_MAX, 1.0, _m(50 * N))[1] == agc.QUIET_MAX  # saturates


def test_clamps():
    assert _step(CFG, 0, 80.0, _m(50 * N)) == (100.0, 1, 1)
    assert _step(CFG, 0, 0.02, _m(500 * N)) == (0.015625, 0, -1)
    big = float(np.finfo(np.float32).max)
    assert _step(CFG, 0, big, _m(50 * N)) == (100.0, 1, 1)  # g * up = +inf clamps to gain_max
    # the clamp acts only when the AGC moves the gain: a host's gain outside the limits stays inside the window
    assert _step(CFG, 0, 1000.0, _m(200 * N)) == (1000.0, 0, 0)
    assert _step(CFG, 0, 1000.0, _m(500 * N)) == (100.0, 0, -1)  # 500 -> clamped down to gain_max
    assert _step(CFG, 0, 0.001, _m(50 * N)) == (0.015625, 1, 1)  # 0.002 -> clamped up to gain_min


def test_single_fp32_multiply():
    g, up = np.float32(1.23456789), np.float32(1.1)
    import dataclasses
    cfg = dataclasses.replace(CFG, up=float(up))
    got = agc.step(cfg, 0, g, _m(50 * N))[0]
    assert got.view(np.uint32) == (g * up).view(np.uint32) and got.dtype == np.float32


def test_no_observation():
    import dataclasses
    for m, parked, cfg in ((_m(500 * N), True, CFG), (_m(0, n=0), False, CFG), (_m(500 * N, clipped=3), False, dataclasses.replace(CFG, hi_ms=0))):
        assert _step(cfg, 4, 1.5, m, parked) == (1.5, 4, 0)


def test_validation_list():
    import dataclasses
    r = dataclasses.replace
    assert agc.invalid(CFG) is None
    assert agc.invalid(r(CFG, hi_ms=0, up=float("nan"), lo_ms=7)) is None
    assert agc.invalid(r(CFG, hi_ms=0), usb=False) is None
    for bad in (r(CFG, silent_ms=101), r(CFG, lo_ms=401), r(CFG, hi_ms=(1 << 30) + 1), r(CFG, up=0.99), r(CFG, down=0.0), r(CFG, down=1.01),
                r(CFG, gain_min=0.0), r(CFG, gain_min=101.0), r(CFG, up=float("inf")), r(CFG, gain_max=float("nan"))):
        assert agc.invalid(bad) is not None, bad
    assert agc.invalid(CFG, usb=False) is not None
    assert agc.invalid(r(CFG, hi_ms=1 << 30)) is None


def test_window_from_dbfs():
    lo, hi = agc.window_from_dbfs(-30.0, -20.0)
    assert (lo, hi) == (round(2 ** 30 * 1e-3), round(2 ** 30 * 1e-2))
    assert agc.window_from_dbfs(-400.0, -300.0) == (0, 1)  # hi_ms 0 would switch the AGC off
    assert agc.window_from_dbfs(0.0, 10.0) == (1 << 30, 1 << 30)
    assert agc.window_is_stable(agc.Cfg(100, 400, 0, 0, 2.0, 0.5, 1, 1)) and not agc.window_is_stable(agc.Cfg(100, 399, 0, 0, 2.0, 0.5, 1, 1))


def test_steady_input_never_alternates():
    """With hi_ms >= lo_ms * max(up^2, 1 / down^2) a steady input -- mean square P g^2, wrapping where its peak passes full
    scale -- never takes a +1 directly after a -1 or the reverse, whatever hold_frames is.  The input is synthetic, not a
    model tree: the trees' frames are not steady (every filter fills during the first frames, and a deep leaf has a few dozen
    outputs per frame), and the property is one of the rule alone."""
    rng = np.random.default_rng(5)
    for _ in range(300):
        up, down = float(np.float32(rng.uniform(1.0, 3.0))), float(np.float32(rng.uniform(0.2, 1.0)))
        lo = int(rng.integers(1, 1 << 20))
        hi = min(1 << 30, int(np.ceil(lo * max(up * up, 1.0 / (down * down)) * (1.0 + 1e-6))) + 1)
        cfg = agc.Cfg(lo, hi, int(rng.integers(0, lo + 1)), int(rng.integers(0, 3)), up, down, 1e-6, 1e6)
        assert agc.window_is_stable(cfg)
        P, crest = float(10.0 ** rng.uniform(-2, 6)), float(rng.uniform(1.5, 6.0))
        g, q, last = np.float32(10.0 ** rng.uniform(-3, 3)), 0, 0
        for _f in range(40):
            ms = P * float(g) ** 2
            clipped = int(np.sqrt(ms) * crest >= 32768.0)
            s = int(min(ms, float(1 << 30)) * N) if not clipped else int(rng.integers(0, (1 << 30) * N))
            g, q, a = agc.step(cfg, q, g, _m(s, clipped))
            assert not (a and last and a != last), (cfg, P, crest, _f)
            last = a


def test_the_closed_loop_covers_every_case():
    """Over the trees the GPU test runs: hot, cold with a raise, cold held, in window, silent and both clamps occur, at least
    half of the USB leaves change gain, and the loop is a loop: the gain a frame used is the one the frame before left."""
    cov = ar.coverage()
    print(cov)
    for c in ar.CASES:
        assert cov[c] > 0, (c, cov)
    assert 2 * cov["moved"] >= cov["leaves"] > 0, cov
    for name in ar.TREES:
        topo, _, sets, want = ar.reference(name)
        for i in sets:
            for f in range(1, len(want)):
                assert want[f]["agc"][i]["gain_used"] == want[f - 1]["agc"][i]["gain_next"], (name, i, f)
    assert any(len(ar.reference(n)[2]) == 1 for n in ar.TREES), "a tree with a single USB leaf"


def test_the_trees_hold_what_the_step_can_get_wrong():
    """A leaf behind k_lpf_long whose gain moves, /5 and /6 leaves, compress() leaves, a childless main."""
    import lattice
    long_moved = late = iq = main = False
    for name in ar.TREES:
        topo, _, sets, want = ar.reference(name)
        for i in topo.leaves_in_publish_order():
            d = topo.vfos[i]
            iq |= not d.demod_usb
            main |= d.parent < 0
            late |= d.demod_usb and d.late_decimate in (5, 6)
            if d.demod_usb and lattice.lpf_taps(d) > 256:
                long_moved |= any(w["agc"][i]["action"] for w in want)
    assert long_moved and late and iq and main


def test_parking_in_the_loop():
    """A parked frame is no observation; an unpark restarts quiet_run and keeps the gain; set_agc restarts quiet_run."""
    topo, frames = ar.tree("small-flat")
    _, _, sets, _ = ar.reference("small-flat")
    leaf = next(i for i, (cfg, _, cls) in sets.items() if cls == "cold" and cfg.hold_frames == 3)
    model = ar.AgcTree(topo)
    for i, (cfg, g0, _) in sets.items():
        model.set_gain(i, g0)
        model.set_agc(i, cfg)
    recs = []
    for f, iq in enumerate(frames):
        if f == 2:
            model.apply([("park", [leaf])])
        if f == 4:
            model.apply([("unpark", [leaf])])
        if f == 6:
            model.apply([("agc", leaf, sets[leaf][0])])
        recs.append(model.process(iq)["agc"][leaf])
    assert [r["quiet_run"] for r in recs] == [1, 2, 2, 2, 1, 2, 1, 2], recs
    assert all(r["action"] == 0 and r["gain_next"] == recs[0]["gain_used"] for r in recs)


def test_binding():
    """The four symbols, the struct sizes and field offsets of include/sdrx.h."""
    from sdrreceiver_amd import _lib
    for name in ("sdrx_set_agc", "sdrx_get_agc", "sdrx_group_set_agc", "sdrx_group_get_agc"):
        assert name in _lib.SYMBOLS, name
    assert C.sizeof(_lib.AgcCfgC) == 32 and C.sizeof(_lib.AgcStateC) == 56
    assert [f[0] for f in _lib.AgcCfgC._fields_] == ["lo_ms", "hi_ms", "silent_ms", "hold_frames", "up", "down", "gain_min", "gain_max"]
    assert (_lib.AgcStateC.frame.offset, _lib.AgcStateC.gain_used.offset, _lib.AgcStateC.gain_next.offset, _lib.AgcStateC.action.offset,
            _lib.AgcStateC.quiet_run.offset, _lib.AgcStateC.cfg.offset) == (0, 8, 12, 16, 20, 24)
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdrx.h")).read()
    for name in ("sdrx_set_agc", "sdrx_get_agc", "sdrx_group_set_agc", "sdrx_group_get_agc", "typedef struct sdrx_agc_cfg", "typedef struct sdrx_agc_state"):
        assert name in header, name
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()  # resolves every symbol
        assert L.sdrx_set_agc and L.sdrx_group_get_agc
