"""Auto-squelch (option "squelch_auto") on the GPU.  The yardstick is the TWIN of tests/test_gpu_squelch.py: a second Receiver
of the same topology, arithmetic and launch options with meter=True and no squelch, fed the same frames.  squelch.decide_auto
runs on the TWIN's sum_sq history -- never on the receiver under test -- and the receiver must reproduce, for every leaf of
every delivered frame, the model's open flag, hang_left, thr_eff, floor and floor_valid, and everything option squelch
delivers for those flags.  Everything is compared for equality; no tolerance enters anywhere.

Shapes: tp.config3(1100) has 1 100 leaves -- k_squelch_scan takes two passes and its last wave is partial (1 100 = 1 024 + 64 +
12), the smallest shape at which the carry-over between passes and the tail can go wrong; helpers.tree_mixed has k_lpf_long,
both compress styles and payloads of different lengths."""
import numpy as np
import pytest

from sdrreceiver_amd import _lib, squelch, topology as tp
from helpers import tree_mixed
from test_gpu_squelch import PATH_KW, Run, check_frame, lcg_frames, tone_frames, twin_history
from test_gpu_preroll import check_frame as check_frame_preroll

pytestmark = pytest.mark.gpu

NONE = squelch.NONE
RATIOS = (0, 257, 260, 512, 1024, 4096)
WINDOWS = (1, 2, 3, 5)
HANGS = (0, 1, 2)
RULE_SEED, RULE_FRAMES = 81, 12


@pytest.fixture(scope="module")
def R():
    from sdrreceiver_amd.receiver import Receiver
    return Receiver


def history(hist):
    """[frame][leaf] sum_sq of a twin's record, as python ints"""
    return np.array([[int(x) for x in h["meters"]["sum_sq"]] for h in hist], dtype=object)


def seeded_settings(ss, seed):
    """Per leaf: ratio_q8, window_frames and hang_frames drawn from RATIOS, WINDOWS and HANGS, and for every 7th leaf a manual
    threshold near its idle sum_sq (9/8 of the smallest one of its history: above the idle frames, below a tone)."""
    n = ss.shape[1]
    rng = np.random.default_rng(seed)
    ratio = [int(RATIOS[j]) for j in rng.integers(0, len(RATIOS), n)]
    window = [int(WINDOWS[j]) for j in rng.integers(0, len(WINDOWS), n)]
    hang = [int(HANGS[j]) for j in rng.integers(0, len(HANGS), n)]
    thr = [int(min(ss[:, k])) * 9 // 8 if k % 7 == 0 else 0 for k in range(n)]
    return thr, hang, ratio, window


def auto_model(ss, thr, hang, ratio, window):
    """squelch.decide_auto for every leaf: [frame][leaf] arrays"""
    n_frames, n = ss.shape
    M = {"open": np.zeros((n_frames, n), np.int32), "hang_left": np.zeros((n_frames, n), np.int64),
         "thr_eff": np.zeros((n_frames, n), np.uint64), "floor": np.zeros((n_frames, n), np.uint64),
         "floor_valid": np.zeros((n_frames, n), np.int32)}
    for k in range(n):
        a = squelch.decide_auto(list(ss[:, k]), thr[k], hang[k], ratio[k], window[k])
        for key in M:
            M[key][:, k] = a[key]
    return M


def check_auto(rx, lv, M, f, ratio, window, ctx):
    """sdrx_get_squelch_auto of ALL leaves for the delivered frame f against the model"""
    a = rx.squelch_auto(lv)
    assert (a["frame"] == f).all(), ctx
    for key, want in (("thr_eff_sum_sq", M["thr_eff"][f]), ("floor_sum_sq", M["floor"][f]), ("floor_valid", M["floor_valid"][f]),
                      ("ratio_q8", np.asarray(ratio, np.int64)), ("window_frames", np.asarray(window, np.int64))):
        assert np.array_equal(a[key], want), (ctx, key, np.flatnonzero(a[key] != want)[:8])


def rule_conditions(M, thr, ctx):
    """the conditions on the input, on the MODEL's output alone"""
    flags = M["open"]
    share = float(flags.mean())
    assert 0.10 <= share <= 0.90, (ctx, "open share", share)
    lifted = int((M["thr_eff"] > np.asarray(thr, np.uint64)[None, :]).any(axis=0).sum())
    assert lifted >= 100, (ctx, "leaves with thr_eff > thr in some frame", lifted)
    reopened = 0
    for k in range(flags.shape[1]):
        col = flags[:, k]
        closed_at = np.flatnonzero((col[1:] == 0) & (col[:-1] == 1)) + 1
        reopened += bool(closed_at.size and col[closed_at[0]:].any())
    assert reopened >= 100, (ctx, "leaves that close and re-open", reopened)


# ---- 1. ratio 0 is the plain gate ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["process", "submit_wait", "device_tail"])
def test_ratio_zero_is_the_plain_gate(R, path):
    topo = tree_mixed()
    frames = tone_frames(topo, 3, seed=23)
    lv, hist = twin_history(R, topo, path, 1, frames)
    ss = history(hist)
    # a threshold per leaf that its own history crosses (the middle one of its three sum_sq), hang times mixed
    thr = [sorted(int(x) for x in ss[:, k])[1] if k % 2 else 0 for k in range(len(lv))]
    hang = [k % 3 for k in range(len(lv))]
    M = auto_model(ss, thr, hang, [0] * len(lv), [0] * len(lv))
    plain = R.from_topology(topo, device=0, squelch=True, **PATH_KW.get(path, {}))
    rx = R.from_topology(topo, device=0, squelch_auto=True, **PATH_KW.get(path, {}))
    got = {}
    for name, r in (("plain", plain), ("auto", rx)):
        r.set_squelch(lv, thr, hang)
        rec = got.setdefault(name, [])

        def visit(f, r=r, rec=rec, name=name):
            check_frame(r, topo, lv, hist[f], f, M["open"][f], M["hang_left"][f], ("ratio0", name, path, f))
            rec.append((f, r.squelch(lv), [r.output(v).tobytes() for v in lv], list(r.published), r.egress()))

        Run(r, topo, path, frames, group=2 if path.startswith("device") else 1).go(visit)
    assert len(got["plain"]) == len(got["auto"]) > 0 and got["auto"][-1][0] == len(frames) - 1
    for a, b in zip(got["plain"], got["auto"]):
        assert a[0] == b[0] and a[2] == b[2] and a[3] == b[3] and a[4] == b[4], (path, a[0])
        for key in a[1]:
            assert np.array_equal(a[1][key], b[1][key]), (path, a[0], key)
    check_auto(rx, lv, M, len(frames) - 1, [0] * len(lv), [0] * len(lv), ("ratio0", path))
    assert np.array_equal(M["thr_eff"][-1], np.asarray(thr, np.uint64))  # ... which says thr_eff = thr, and a floor all the same
    assert M["floor_valid"][-1].all()
    plain.close()
    rx.close()


# ---- 2. the rule --------------------------------------------------------------------------------------------------------------
RULE_CASES = [("process", 1), ("process_u8_dc", 1), ("submit_wait", 1), ("device_tail", 1), ("device_no_tail", 1), ("fuse_demod", 1),
              ("process", 0), ("device_tail", 2)]


@pytest.mark.parametrize("path,exact", RULE_CASES)
def test_the_rule_on_the_twins_meters(R, path, exact):
    topo = tp.config3(1100)
    ctx = ("rule", path, exact)
    frames = tone_frames(topo, RULE_FRAMES, seed=RULE_SEED)
    lv, hist = twin_history(R, topo, path, exact, frames)
    assert len(lv) == 1100
    ss = history(hist)
    thr, hang, ratio, window = seeded_settings(ss, RULE_SEED)
    M = auto_model(ss, thr, hang, ratio, window)
    rule_conditions(M, thr, ctx)
    rx = R.from_topology(topo, device=0, exact=exact, squelch_auto=True, **PATH_KW.get(path, {}))
    rx.set_squelch(lv, thr, hang)
    rx.set_squelch_auto(lv, ratio, window)
    seen = []

    def visit(f):
        check_auto(rx, lv, M, f, ratio, window, ctx + (f,))
        check_frame(rx, topo, lv, hist[f], f, M["open"][f], M["hang_left"][f], ctx + (f,))
        seen.append(f)

    group = 3 if path == "device_tail" else 2 if path.startswith("device") else 1
    Run(rx, topo, path, frames, group=group).go(visit)
    assert seen and seen[-1] == len(frames) - 1
    rx.close()


# ---- 3. saturation on the device -------------------------------------------------------------------------------------------
def test_saturation_and_zero_frames_on_the_device(R):
    topo = tree_mixed()
    lv = topo.leaves_in_publish_order()
    twin = R.from_topology(topo, device=0, meter=True)
    rx = R.from_topology(topo, device=0, squelch_auto=True)
    # the USB leaf with the most samples per frame, 100 times its gain: its audio wraps (an RMS of some 1e5 LSB: inside int32,
    # whose low 16 bits are kept), int16 values all over their range
    loud = max((v for v in lv if topo.vfos[v].demod_usb), key=lambda v: topo.vfos[v].samples_per_buffer >> topo.vfos[v].decimate_count)
    kl = lv.index(loud)
    for r_ in (twin, rx):
        r_.set_gains([loud], [topo.vfos[loud].gain * 100.0])
    thr = [1000 * (k % 3) for k in range(len(lv))]  # manual thresholds 0, 1000, 2000: "thr_eff == thr" says something
    ratio = [(1 << 32) - 1 if v == loud else 512 for v in lv]
    window = [1] * len(lv)
    rx.set_squelch(lv, thr, [0] * len(lv))
    rx.set_squelch_auto(lv, ratio, window)
    zero = np.zeros(2 * topo.frame, np.float32)
    frames = lcg_frames(topo, 3, seed=91) + [zero] * 4 + lcg_frames(topo, 1, seed=92)
    rows, got = [], []
    for f, x in enumerate(frames):
        twin.process(x)
        rx.process(x)
        m = twin.meters(lv)
        rows.append([int(s) for s in m["sum_sq"]])
        if f < 3:
            assert rows[f][kl] > 1 << 40 and int(m["clipped"][kl]) > 0, (f, rows[f][kl])
        got.append((rx.squelch(lv), rx.squelch_auto(lv), [rx.output(v).tobytes() for v in lv], [twin.output(v).tobytes() for v in lv]))
    ss = np.array(rows, dtype=object)
    M = auto_model(ss, thr, [0] * len(lv), ratio, window)
    # on the twin: the filters have run empty within the zero frames -- some frame z has sum_sq 0 on EVERY leaf, and a frame follows
    z = next(f for f in range(3, 7) if not any(rows[f]))
    assert z + 1 < len(frames)
    for f, (sq, au, out, want) in enumerate(got):
        for key, w in (("thr_eff_sum_sq", M["thr_eff"][f]), ("floor_sum_sq", M["floor"][f]), ("floor_valid", M["floor_valid"][f])):
            assert np.array_equal(au[key], w), (f, key)
        assert np.array_equal(sq["open"], M["open"][f]), f
        assert out == [w if o else b"" for w, o in zip(want, M["open"][f])], f
    for f in (1, 2):  # from the second frame on: saturated, and closed
        assert int(got[f][1]["thr_eff_sum_sq"][kl]) == NONE and int(got[f][0]["open"][kl]) == 0 and int(got[f][1]["floor_valid"][kl]) == 1
        assert int(got[f][1]["floor_sum_sq"][kl]) == rows[f - 1][kl] > 1 << 40
    assert int(got[0][1]["thr_eff_sum_sq"][kl]) == thr[kl] and int(got[0][1]["floor_valid"][kl]) == 0
    au = got[z + 1][1]  # behind the all-zero frame: floor 0 -- an observation -- and thr_eff == thr, on every leaf
    assert not au["floor_sum_sq"].any() and au["floor_valid"].all()
    assert np.array_equal(au["thr_eff_sum_sq"], np.asarray(thr, np.uint64))
    twin.close()
    rx.close()


# ---- 4. live changes ------------------------------------------------------------------------------------------------------------
def test_live_changes_and_calling_rules(R):
    from sdrreceiver_amd.receiver import SdrxError
    topo = tp.config3(1100)
    lv = topo.leaves_in_publish_order()
    n = len(lv)
    frames = lcg_frames(topo, 9, seed=53)
    twin = R.from_topology(topo, device=0, meter=True)
    rx = R.from_topology(topo, device=0, squelch_auto=True)
    gate_only = R.from_topology(topo, device=0, squelch=True)

    def code(fn):
        with pytest.raises(SdrxError) as e:
            fn()
        return e.value.code

    assert code(lambda: gate_only.set_squelch_auto([lv[0]], [512], [2])) == _lib.SDRX_ESTATE  # the option is off
    assert code(lambda: gate_only.squelch_auto([lv[0]])) == _lib.SDRX_ESTATE
    assert code(lambda: rx.squelch_auto([lv[0]])) == _lib.SDRX_ESTATE  # nothing delivered yet
    # the model, leaf by leaf, carried from frame to frame: settings and (hang_left, cur_min, prev_min, age)
    cfg = [dict(thr=0, hang=0, ratio=0, window=0) for _ in range(n)]
    state = [(0, NONE, NONE, 0) for _ in range(n)]

    def step(f, x):
        twin.process(x)
        rx.process(x)
        s = [int(v) for v in twin.meters(lv)["sum_sq"]]
        want = {key: [] for key in ("open", "hang_left", "thr_eff", "floor", "floor_valid")}
        for k in range(n):
            left, cur, prev, age = state[k]
            a = squelch.decide_auto([s[k]], cfg[k]["thr"], cfg[k]["hang"], cfg[k]["ratio"], cfg[k]["window"], hang_left=left,
                                    cur_min=cur, prev_min=prev, age=age, return_state=True)
            state[k] = a["state"]
            for key in want:
                want[key].append(int(a[key][0]))
        sq, au = rx.squelch(lv), rx.squelch_auto(lv)
        assert (sq["frame"] == f).all() and (au["frame"] == f).all()
        for key, got in (("open", sq["open"]), ("hang_left", sq["hang_left"]), ("thr_eff", au["thr_eff_sum_sq"]),
                         ("floor", au["floor_sum_sq"]), ("floor_valid", au["floor_valid"])):
            assert [int(v) for v in got] == want[key], (f, key)
        assert [int(v) for v in au["ratio_q8"]] == [c["ratio"] for c in cfg] and [int(v) for v in au["window_frames"]] == [c["window"] for c in cfg]
        assert [int(v) for v in sq["thr_sum_sq"]] == [c["thr"] for c in cfg] and [int(v) for v in sq["hang_frames"]] == [c["hang"] for c in cfg]
        return want

    def set_auto(ks, ratio, window):
        rx.set_squelch_auto([lv[k] for k in ks], ratio, window)
        for k, r_, w in zip(ks, ratio, window):
            cfg[k].update(ratio=int(r_), window=int(w))
            state[k] = (state[k][0], NONE, NONE, 0)  # the floor restarts; hang_left stays

    def set_manual(ks, thr, hang):
        rx.set_squelch([lv[k] for k in ks], thr, hang)
        for k, t, h in zip(ks, thr, hang):
            cfg[k].update(thr=int(t), hang=int(h))
            state[k] = (0,) + tuple(state[k][1:])  # hang_left restarts; the floor state stays

    everyone = list(range(n))
    set_auto(everyone, [(257, 260, 300, 0)[k % 4] for k in everyone], [(1, 2, 3, 5)[k % 4] if k % 4 != 3 else 0 for k in everyone])
    set_manual(everyone[::3], [0] * len(everyone[::3]), [2] * len(everyone[::3]))
    w0 = step(0, frames[0])
    assert all(w0["open"]) and not any(w0["floor_valid"])  # the first frame decides with thr = 0 alone
    w2 = [step(f, frames[f]) for f in (1, 2)][-1]
    assert all(w2["floor_valid"]) and 0 < sum(w2["open"]) < n  # the floor decides by now: the noise alone opens some, not all
    # a subset restarts: its next frame decides with thr, floor_valid 0; everyone else goes on
    sub = everyone[5::11]
    others = [k for k in everyone if k not in set(sub)]
    set_auto(sub, [300] * len(sub), [4] * len(sub))
    w3 = step(3, frames[3])
    assert not any(w3["floor_valid"][k] for k in sub) and all(w3["thr_eff"][k] == cfg[k]["thr"] for k in sub)
    assert all(w3["open"][k] for k in sub) and all(w3["floor_valid"][k] for k in others)
    w4 = step(4, frames[4])
    assert all(w4["floor_valid"])
    # set_squelch on other leaves: hang_left restarts, their floor goes on as if nothing had been set
    man = everyone[2::13]
    s_idle = [int(v) for v in twin.meters([lv[k] for k in man])["sum_sq"]]
    set_manual(man, [v // 2 if j % 2 else squelch.NEVER_OPEN for j, v in enumerate(s_idle)], [1] * len(man))
    w5 = step(5, frames[5])
    assert all(w5["floor_valid"][k] for k in man) and all(w5["thr_eff"][k] >= cfg[k]["thr"] for k in man)
    assert not any(w5["open"][k] for k in man[0::2])  # NEVER_OPEN is a lower bound the floor cannot undercut
    step(6, frames[6])
    # every SDRX_EINVAL list leaves everything unchanged
    before_a, before_s = rx.squelch_auto(lv), rx.squelch(lv)
    a = lv[7]
    for bad, rr, ww in (([a, a], [512, 512], [2, 2]), ([0], [512], [2]), ([len(topo.vfos)], [512], [2]), ([-1], [512], [2]),
                        ([lv[3], 1], [512, 512], [2, 2]), ([lv[3], a], [0, 1], [0, 0])):  # the last: window 0 with a ratio
        assert code(lambda: rx.set_squelch_auto(bad, rr, ww)) == _lib.SDRX_EINVAL, bad
    assert rx.L.sdrx_set_squelch_auto(rx.h, None, None, None, -1) == _lib.SDRX_EINVAL
    rx.set_squelch_auto([], [], [])
    rx.set_squelch_auto([lv[3]], [0], [0])  # (allowed: off needs no window) -- and put back, with the model
    set_auto([3], [cfg[3]["ratio"]], [cfg[3]["window"]])
    after_a, after_s = rx.squelch_auto(lv), rx.squelch(lv)
    for b_, a_ in ((before_a, after_a), (before_s, after_s)):
        for key in b_:
            assert np.array_equal(b_[key], a_[key]), key
    step(7, frames[7])  # ... on the device too: the model never saw the refused lists
    # SDRX_ESTATE while a frame is in flight
    rx.submit(frames[8])
    assert code(lambda: rx.set_squelch_auto([a], [512], [2])) == _lib.SDRX_ESTATE
    rx.wait()
    for r_ in (rx, twin, gate_only):
        r_.close()


# ---- 5. with pre-roll -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["process", "device_no_tail"])
def test_with_preroll(R, path):
    topo = tree_mixed()
    ctx = ("preroll", path)
    frames = tone_frames(topo, 8, seed=63)
    lv, hist = twin_history(R, topo, path, 1, frames)
    ss = history(hist)
    n = len(lv)
    thr, hang = [0] * n, [k % 2 for k in range(n)]
    ratio, window = [(257, 260, 512)[k % 3] for k in range(n)], [(1, 2)[(k // 3) % 2] for k in range(n)]
    M = auto_model(ss, thr, hang, ratio, window)
    pre = np.zeros_like(M["open"])
    for k in range(n):
        pre[:, k] = squelch.preroll_flags(M["open"][:, k])
    assert int(pre.sum()) >= 4 and pre[0].sum() == 0, (ctx, "re-open events", int(pre.sum()))  # on the model's output alone
    rx = R.from_topology(topo, device=0, preroll=True, squelch_auto=True, **PATH_KW.get(path, {}))
    rx.set_squelch(lv, thr, hang)
    rx.set_squelch_auto(lv, ratio, window)
    seen = []

    def visit(f):
        check_auto(rx, lv, M, f, ratio, window, ctx + (f,))
        check_frame_preroll(rx, topo, lv, hist, f, M["open"][f], M["hang_left"][f], pre[f], ctx + (f,))
        seen.append(f)

    Run(rx, topo, path, frames, group=2 if path.startswith("device") else 1).go(visit)
    assert seen and seen[-1] == len(frames) - 1
    rx.close()


# ---- 6. group ------------------------------------------------------------------------------------------------------------------------
def test_a_group_of_four_equals_the_single_context(R):
    from sdrreceiver_amd.receiver import Group, SdrxError
    topo = tp.config3(1100)
    lv = topo.leaves_in_publish_order()
    frames = tone_frames(topo, 6, seed=RULE_SEED)
    _, hist = twin_history(R, topo, "process", 1, frames)
    thr, hang, ratio, window = seeded_settings(history(hist), 73)
    single = R.from_topology(topo, device=0, squelch_auto=True)
    grp = Group.from_topology(topo, devices=[0, 0, 0, 0], squelch_auto=1)
    owner = np.array([grp.locate(v)[0] for v in lv])
    assert len(set(owner.tolist())) == 4
    for r_ in (single, grp):
        r_.set_squelch(lv, thr, hang)
        r_.set_squelch_auto(lv[::-1], ratio[::-1], window[::-1])  # (a list in another order than the members hold the leaves)
    lifted = np.zeros(len(lv), bool)
    for f, x in enumerate(frames):
        single.published.clear()
        single.process(x)
        grp.process(x)
        for a, b in ((single.squelch(lv), grp.squelch(lv)), (single.squelch_auto(lv), grp.squelch_auto(lv))):
            for key in a:
                assert np.array_equal(a[key], b[key]), (f, key)
        au = grp.squelch_auto(lv)
        assert np.array_equal(au["ratio_q8"], np.asarray(ratio)) and np.array_equal(au["window_frames"], np.asarray(window))
        lifted |= au["thr_eff_sum_sq"] > np.asarray(thr, np.uint64)
        assert 0 < single.squelch(lv)["open"].sum() < len(lv)
        for v in lv:
            assert single.output(v).tobytes() == grp.output(v).tobytes(), (f, v)
        assert single.published == grp.published and single.egress() == grp.egress(), f
    assert all(lifted[owner == m].any() for m in range(4))  # the floor decided something on every member
    # routing: one leaf of every member, each with values of its own, read back through the group and through its member
    picks = [lv[int(np.flatnonzero(owner == m)[0])] for m in range(4)]
    grp.set_squelch_auto(picks, [1000 + m for m in range(4)], [7 + m for m in range(4)])
    grp.process(frames[0])
    au = grp.squelch_auto(picks)
    assert au["ratio_q8"].tolist() == [1000, 1001, 1002, 1003] and au["window_frames"].tolist() == [7, 8, 9, 10]
    assert not au["floor_valid"].any() and (grp.squelch_auto(lv)["floor_valid"].sum() == len(lv) - 4)
    for m, v in enumerate(picks):
        ctxp, _ = grp.member_context(m)
        rec = (_lib.SquelchAutoStateC * 1)()
        lid = np.array([grp.locate(v)[1]], np.int32)
        assert grp.L.sdrx_get_squelch_auto(ctxp, lid.ctypes.data, 1, rec) == 0
        assert (rec[0].ratio_q8, rec[0].window_frames, rec[0].floor_valid) == (1000 + m, 7 + m, 0)
    with pytest.raises(SdrxError) as e:
        grp.set_squelch_auto([picks[0], picks[1]], [512, 512], [2, 0])
    assert e.value.code == _lib.SDRX_EINVAL and grp.squelch_auto(picks)["ratio_q8"].tolist() == [1000, 1001, 1002, 1003]
    single.close()
    grp.close()


# ---- 7. memory -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", ["config3_1100", "mixed"])
def test_memory_formula(R, tree):
    """32 L for the per-leaf records, and per frame parity the directory's growth: thr_eff[L] | floor[L] on 8
    bytes behind what it held, the whole rounded to 64 as before"""
    topo = tp.config3(1100) if tree == "config3_1100" else tree_mixed()
    L = len(topo.leaves_in_publish_order())
    align8 = lambda v: (v + 7) // 8 * 8  # noqa: E731
    for pre, words in ((False, 8), (True, 12)):
        base = R.from_topology(topo, device=0, squelch=True, preroll=pre)
        auto = R.from_topology(topo, device=0, squelch_auto=True, preroll=pre)
        grown = squelch.align64(align8(64 + words * L) + 16 * L) - squelch.align64(64 + words * L)
        assert auto.stats()["device_bytes"] - base.stats()["device_bytes"] == 32 * L + 2 * grown, (tree, pre)
        base.close()
        auto.close()
