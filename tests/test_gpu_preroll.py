"""Squelch pre-roll (option "preroll") on the GPU.  The yardstick is the TWIN of tests/test_gpu_squelch.py: a second Receiver
of the same topology, arithmetic and launch options with meter=True and no squelch, fed the same frames.  Its per-frame
payload bytes, sum_sq and published messages are the expectation; squelch.decide + squelch.preroll_flags on the twin's sum_sq
give the flags.  The receiver under test must deliver, for a leaf that opens in frame f after the gate closed it in f-1, the
twin's payload of f-1 ahead of that of f, bit for bit -- and otherwise exactly what option squelch delivers."""
import hashlib
import math

import numpy as np
import pytest

from sdrreceiver_amd import _lib, squelch, synth, topology as tp
from test_gpu_squelch import PATHS, PATH_KW, TREES, Run, lcg_frames, model, publishing, same_meters, thresholds_from, twin_history

pytestmark = pytest.mark.gpu

N_FRAMES = 10
PATH_KW = dict(PATH_KW, device_fuse_demod=dict(fuse_demod=True))  # fuse_demod on DEVICE frames (the software pipeline)


@pytest.fixture(scope="module")
def R():
    from sdrreceiver_amd.receiver import Receiver
    return Receiver


def moving_tone_frames(topo, n, seed, n_tones=48):
    """LCG noise and tones over the raw band with a PER-FRAME tone set: the energy moves between leaves from frame to frame"""
    rng = np.random.default_rng(seed)
    freqs = rng.uniform(-0.45 * topo.fs, 0.45 * topo.fs, n_tones)
    amps = rng.uniform(6.0, 30.0, n_tones) / np.sqrt(n_tones / 4.0)
    lcg = synth.Lcg(seed)
    out = []
    for f in range(n):
        on = rng.random(n_tones) < 0.4
        tones = [(float(freqs[k]), float(amps[k])) for k in range(n_tones) if on[k]]
        out.append(synth.tone_frame(topo.frame, topo.fs, tones, f * topo.frame, lcg))
    return out


def pre_model(flags):
    pre = np.zeros_like(flags)
    for k in range(flags.shape[1]):
        pre[:, k] = squelch.preroll_flags(flags[:, k])
    return pre


def check_frame(rx, topo, lv, hist, f, open_f, left_f, pre_f, ctx):
    """one delivered frame f against the twin's records of f and f-1 and the model's flags"""
    h = hist[f]
    sq = rx.squelch(lv)
    assert (sq["frame"] == f).all(), ctx
    assert np.array_equal(sq["open"], open_f), (ctx, np.flatnonzero(sq["open"] != open_f)[:8])
    assert np.array_equal(sq["hang_left"], left_f), (ctx, np.flatnonzero(sq["hang_left"] != left_f)[:8])
    same_meters(rx.meters(lv), h["meters"], ctx)
    copied = pre_bytes = 0
    for k, v in enumerate(lv):
        got, pre = rx.output(v), rx.preroll(v)
        dtype = np.int16 if topo.vfos[v].demod_usb else np.int8
        assert pre.dtype == dtype and got.dtype == dtype, (ctx, v)
        if open_f[k]:
            assert got.tobytes() == h["out"][k], (ctx, v, "open payload")
            copied += squelch.align64(len(h["out"][k]))
        else:
            assert got.size == 0, (ctx, v, "closed leaf")
        if pre_f[k]:
            assert pre.tobytes() == hist[f - 1]["out"][k], (ctx, v, "pre-rolled payload = the twin's frame f-1")
            pre_bytes += squelch.align64(len(hist[f - 1]["out"][k]))
        else:
            assert pre.size == 0, (ctx, v, "no pre-roll")
    pubs = publishing(topo, lv)
    assert len(h["pub"]) == len(pubs), ctx
    where = {v: k for k, v in enumerate(lv)}
    want = []
    for j, v in enumerate(pubs):
        k = where[v]
        if pre_f[k]:
            want.append(hist[f - 1]["pub"][j])  # pre-roll first, same topic and rate
        if open_f[k]:
            want.append(h["pub"][j])
    assert rx.published == want, (ctx, len(rx.published), len(want))
    eg = rx.egress()
    assert eg == {"frame": f, "n_open": int(np.sum(open_f)), "n_leaves": len(lv), "payload_bytes_copied": copied + pre_bytes}, (ctx, eg)
    assert rx.preroll_count() == {"n_preroll": int(np.sum(pre_f)), "preroll_bytes": pre_bytes}, (ctx, rx.preroll_count())
    if int(np.sum(pre_f)):  # the ABI call names the frame the pre-roll is of
        import ctypes as C
        buf, ln, fr = C.c_void_p(), C.c_uint32(), C.c_int64()
        v = lv[int(np.flatnonzero(pre_f)[0])]
        assert rx.L.sdrx_get_preroll(rx.h, v, C.byref(buf), C.byref(ln), C.byref(fr)) == 0
        assert (fr.value, ln.value) == (f - 1, len(hist[f - 1]["out"][where[v]])), ctx


def shows_something(ss, thr, flags, pre, ctx):
    """the conditions on the MODEL's output, before anything is compared"""
    above = np.array([[int(ss[f, k]) >= thr[k] for k in range(ss.shape[1])] for f in range(ss.shape[0])])
    assert int(pre.sum()) >= 8, (ctx, "re-open events", int(pre.sum()))
    assert pre[0].sum() == 0, ctx
    assert (flags.min(axis=0) == 1).any(), (ctx, "no leaf stays open")
    assert (flags.max(axis=0) == 0).any(), (ctx, "no leaf stays closed")
    assert ((flags == 1) & ~above).any(), (ctx, "no leaf held by its hang time alone")


def run_case(R, topo, path, exact, frames, ctx, extra_kw=None, timing=False):
    """Returns the launch counts of the eight timed kernel kinds, of the twin and of the receiver under test (`timing`)."""
    kw = dict(PATH_KW.get(path, {}), **(extra_kw or {}))
    run_path = "device" if path == "device_fuse_demod" else path
    twin = R.from_topology(topo, device=0, exact=exact, meter=True, **kw)
    if timing:
        twin.enable_kernel_timing(True)
    lv = topo.leaves_in_publish_order()
    hist = []

    def record(f):
        assert len(hist) == f
        hist.append({"meters": twin.meters(lv), "out": [twin.output(v).tobytes() for v in lv], "pub": list(twin.published)})

    Run(twin, topo, run_path, frames).go(record)
    launches = {"twin": {k: v["launches"] for k, v in twin.kernel_times().items()}} if timing else {}
    twin.close()
    ss, thr, hang = thresholds_from(hist, len(lv))
    flags, left = model(ss, thr, hang)
    pre = pre_model(flags)
    shows_something(ss, thr, flags, pre, ctx)
    rx = R.from_topology(topo, device=0, exact=exact, preroll=True, **kw)
    if timing:
        rx.enable_kernel_timing(True)
    rx.set_squelch(lv, thr, hang)
    seen = []

    def visit(f):
        check_frame(rx, topo, lv, hist, f, flags[f], left[f], pre[f], ctx + (f,))
        seen.append(f)

    # device paths deliver every second frame: the pre-roll of a delivered frame may be a frame that was never delivered
    Run(rx, topo, run_path, frames, group=2 if run_path.startswith("device") else 1).go(visit)
    assert seen and seen[-1] == len(frames) - 1
    if timing:
        launches["rx"] = {k: v["launches"] for k, v in rx.kernel_times().items()}
    rx.close()
    return launches


# ---- 3. the purpose, end to end ----------------------------------------------------------------------------------------------
def burst_frames(topo, leaf, n=8, amp=3.0, audio_hz=3000.0):
    """LCG noise, and a tone `audio_hz` inside `leaf`'s passband (a sub VFO; the mixers ADD their frequency, so the raw
    frequency is the audio offset minus the main's and the sub's mixer frequency) switched on 90 % into frame 3 and off in
    the middle of frame 5.  At amplitude 3 a whole frame of it lifts the leaf's sum_sq by about 12 dB, a tenth by about 4."""
    v = topo.vfos[leaf]
    f_raw = audio_hz - topo.vfos[v.parent].mixer_freq - v.mixer_freq
    lcg = synth.Lcg(5)
    out = []
    for f in range(n):
        x = synth.lcg_frame(topo.frame, lcg)
        if 3 <= f <= 5:
            t = synth.tone_frame(topo.frame, topo.fs, [(f_raw, amp)], f * topo.frame)
            if f == 3:
                t[: 2 * (topo.frame * 9 // 10)] = 0.0
            if f == 5:
                t[2 * (topo.frame // 2):] = 0.0
            x = x + t
        out.append(x)
    return out


def test_a_burst_that_starts_late_in_a_frame_is_delivered_whole(R):
    topo = tp.config3(1024)
    lv = topo.leaves_in_publish_order()
    leaf = lv[512 + 200]  # a 48 kS/s sub of the second main without the audio low-pass
    assert topo.vfos[leaf].decimate_count == 2 and topo.vfos[leaf].filter_bw == 0
    frames = burst_frames(topo, leaf)
    twin = R.from_topology(topo, device=0, meter=True)
    t_out, t_ss, t_pub = [], [], []
    j = publishing(topo, lv).index(leaf)
    for x in frames:
        twin.process(x)
        t_out.append(twin.output(leaf).tobytes())
        t_ss.append(int(twin.meters([leaf])["sum_sq"][0]))
        t_pub.append(twin.published[j])
    twin.close()
    idle = max(t_ss[0], t_ss[1], t_ss[2])
    thr = int(round(math.sqrt(float(idle) * float(t_ss[4]))))  # halfway in dB between the idle frames and frame 4
    print("burst: sum_sq per frame", t_ss, "threshold", thr)
    # conditions on the INPUT, from the twin's figures alone
    assert t_ss[3] < thr <= t_ss[4], (t_ss, thr)
    assert all(s < thr for s in t_ss[:3] + t_ss[6:]) and t_ss[5] >= thr, (t_ss, thr)
    want_open = squelch.decide(t_ss, thr, 1)
    assert want_open.tolist() == [0, 0, 0, 0, 1, 1, 1, 0]
    others = [v for v in lv if v != leaf]
    got = {}
    for name, kw in (("squelch", dict(squelch=True)), ("preroll", dict(preroll=True))):
        rx = R.from_topology(topo, device=0, **kw)
        rx.set_squelch(others, [squelch.NEVER_OPEN] * len(others), [0] * len(others))
        rx.set_squelch([leaf], [thr], [1])
        msgs = []
        for f, x in enumerate(frames):
            rx.published.clear()
            rx.process(x)
            msgs += rx.published
            assert int(rx.squelch([leaf])["open"][0]) == int(want_open[f]), (name, f)
            if name == "preroll":
                pre = rx.preroll(leaf)
                assert pre.tobytes() == (t_out[3] if f == 4 else b""), (f, "frame 3 arrives with the delivery of frame 4")
                assert rx.preroll_count()["n_preroll"] == (1 if f == 4 else 0), f
        got[name] = msgs
        rx.close()
    # with the gate alone frame 3 -- the head of the burst -- is never published
    assert got["squelch"] == [t_pub[4], t_pub[5], t_pub[6]]
    assert t_pub[3] not in got["squelch"]
    # with the pre-roll the decoder behind the socket gets frames 3, 4, 5, 6 in order, byte for byte
    assert got["preroll"] == [t_pub[3], t_pub[4], t_pub[5], t_pub[6]]
    assert b"".join(m[2] for m in got["preroll"]) == b"".join(t_out[3:7])


# ---- 4. every path, arithmetic and tree ------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("exact", [1, 0, 2])
@pytest.mark.parametrize("tree", list(TREES))
def test_preroll_follows_the_model_on_the_twins_meters(R, tree, exact, path):
    topo = TREES[tree]()
    run_case(R, topo, path, exact, moving_tone_frames(topo, N_FRAMES, seed=43), (tree, exact, path))


# ---- 5. thresholds 0 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_thresholds_zero_equal_the_option_off(R, path):
    topo = tp.config3(1024)
    frames = lcg_frames(topo, 3, seed=21)
    lv, hist = twin_history(R, topo, path, 1, frames)
    rx = R.from_topology(topo, device=0, preroll=True, **PATH_KW.get(path, {}))
    ones, zeros, none = np.ones(len(lv), np.int32), np.zeros(len(lv), np.int64), np.zeros(len(lv), np.int32)
    seen = []

    def visit(f):
        check_frame(rx, topo, lv, hist, f, ones, zeros, none, ("thr0", path, f))
        assert rx.published == hist[f]["pub"]
        seen.append(f)

    Run(rx, topo, path, frames, group=2 if path.startswith("device") else 1).go(visit)
    assert seen and seen[-1] == len(frames) - 1
    rx.close()


# ---- 6. the combinations in which frame f+1's payload is written early ------------------------------------------------------
@pytest.mark.parametrize("exact", [1, 0, 2])
def test_fuse_demod_on_device_frames(R, exact):
    """the leaves write their int16 in the levels launch: with preroll such a tree keeps k_mix_levels in every arithmetic
    (DESIGN.md 4g), so that no payload of f+1 is written in front of the gate of f.  Wrong bytes would show a race only by
    luck, so the planner rule itself is asserted from the launch counts: 256 subs are few enough demodulation blocks per CU
    for k_levels_tail in the packed arithmetics (config 3's 1 024 are not), and there the twin -- the same options without
    preroll -- demodulates its 12 kS/s leaves inside the levels launch (no k_usb_demod launch at all), the receiver under
    test in one k_usb_demod launch per frame."""
    topo = tp.config3(256)
    n = run_case(R, topo, "device_fuse_demod", exact, moving_tone_frames(topo, N_FRAMES, seed=47), ("device_fuse_demod", exact),
                 timing=True)
    assert n["rx"].get("k_usb_demod") == N_FRAMES and n["rx"].get("k_mix_levels", 0) > 0, n
    if exact != 1:  # (in the exact arithmetic option meter alone keeps the twin out of k_levels_tail: DESIGN.md 4e)
        assert "k_usb_demod" not in n["twin"], n


def test_two_streams_with_fuse_demod_through_submit_and_wait(R):
    """option pipeline = 1: the levels of f+1 (which write the payloads) wait for the gate of f.  (The event wait has no
    figure to assert: without it this case could still pass by timing.  It is here so that wrong bytes, if the order is
    ever lost, have a place to show.)"""
    topo = tp.config3(1024)
    run_case(R, topo, "submit_wait", 1, moving_tone_frames(topo, N_FRAMES, seed=49), ("pipeline+fuse_demod",),
             extra_kw=dict(pipeline=True, fuse_demod=True))


# ---- 7. the rule follows the gate, not what the host fetched ---------------------------------------------------------------
def test_three_device_frames_then_one_fetch(R):
    import torch
    topo = tp.config3(1024)
    frames = moving_tone_frames(topo, 3, seed=53)
    lv, hist = twin_history(R, topo, "device_tail", 1, frames)
    ss = np.array([[int(x) for x in h["meters"]["sum_sq"]] for h in hist], dtype=object)
    # closed in the second frame, open in the third: the threshold is the third frame's own sum_sq
    rising = [k for k in range(len(lv)) if ss[1, k] < ss[2, k]]
    assert len(rising) >= 8
    thr = [int(ss[2, k]) if k in set(rising) else (0 if k % 2 else squelch.NEVER_OPEN) for k in range(len(lv))]
    hang = [0] * len(lv)
    flags, left = model(ss, thr, hang)
    pre = pre_model(flags)
    assert all(flags[1, k] == 0 and flags[2, k] == 1 and pre[2, k] == 1 for k in rising)
    rx = R.from_topology(topo, device=0, preroll=True)
    rx.set_squelch(lv, thr, hang)
    t = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() for x in frames]
    torch.cuda.synchronize()
    for x in t:
        rx.process_device(x.data_ptr(), topo.frame)
    rx.published.clear()
    rx.fetch()
    check_frame(rx, topo, lv, hist, 2, flags[2], left[2], pre[2], ("three then fetch",))
    rx.close()


# ---- 8. scale and group -----------------------------------------------------------------------------------------------------
def test_north_star_tree_with_a_moving_five_percent(R):
    topo = tp.config3(10240)
    lv = topo.leaves_in_publish_order()
    n = 6
    frames = lcg_frames(topo, n, seed=61)
    rng = np.random.default_rng(7)
    sets = [rng.choice(len(lv), len(lv) // 20, replace=False) for _ in range(n // 2)]  # a different 5 % every other frame
    live = np.zeros((n, len(lv)), np.int32)
    for f in range(n):
        live[f, sets[f // 2]] = 1
    pre = pre_model(live)
    assert all(0.04 * len(lv) <= pre[f].sum() <= 0.05 * len(lv) for f in (2, 4)) and pre[[0, 1, 3, 5]].sum() == 0
    twin = R.from_topology(topo, device=0, meter=True)
    twin.set_publish(False)
    rx = R.from_topology(topo, device=0, preroll=True)
    topic = {v: topo.vfos[v].topic.encode().ljust(5, b"\0")[:5] for v in lv}
    kept = {}
    for f, x in enumerate(frames):
        if f % 2 == 0:
            rx.set_squelch(lv, [0 if o else squelch.NEVER_OPEN for o in live[f]], [0] * len(lv))
        twin.process(x)
        rx.published.clear()
        rx.process(x)
        sq = rx.squelch(lv)
        assert np.array_equal(sq["open"], live[f]), f
        same_meters(rx.meters(lv), twin.meters(lv), f)
        want, topics, copied, pre_bytes = hashlib.sha256(), [], 0, 0
        for k in np.flatnonzero(live[f]):
            v = lv[int(k)]
            if pre[f, k]:
                want.update(kept[v])
                topics.append(topic[v])
                pre_bytes += squelch.align64(len(kept[v]))
            t = twin.output(v).tobytes()
            want.update(t)
            topics.append(topic[v])
            copied += squelch.align64(len(t))
        got = hashlib.sha256()
        for m in rx.published:
            got.update(m[2])
        assert [m[0] for m in rx.published] == topics, f
        assert got.digest() == want.digest(), f
        assert rx.egress() == {"frame": f, "n_open": int(live[f].sum()), "n_leaves": len(lv), "payload_bytes_copied": copied + pre_bytes}
        assert rx.preroll_count() == {"n_preroll": int(pre[f].sum()), "preroll_bytes": pre_bytes}
        if f + 1 < n:  # the twin's payloads of this frame for the leaves that will open in the next
            kept = {lv[int(k)]: twin.output(lv[int(k)]).tobytes() for k in np.flatnonzero(live[f + 1] & (1 - live[f]))}
    twin.close()
    rx.close()


def test_a_group_of_four_equals_the_single_context(R):
    from sdrreceiver_amd.receiver import Group
    topo = tp.config3(1024)
    lv = topo.leaves_in_publish_order()
    frames = moving_tone_frames(topo, 6, seed=71)
    _, hist = twin_history(R, topo, "process", 1, frames)
    ss, thr, hang = thresholds_from(hist, len(lv))
    pre = pre_model(model(ss, thr, hang)[0])
    assert pre.sum() >= 8
    single = R.from_topology(topo, device=0, preroll=True)
    grp = Group.from_topology(topo, devices=[0, 0, 0, 0], preroll=1)
    assert len({grp.locate(v)[0] for v in lv}) == 4
    single.set_squelch(lv, thr, hang)
    grp.set_squelch(lv, thr, hang)
    for f, x in enumerate(frames):
        single.published.clear()
        single.process(x)
        grp.process(x)
        a, b = single.squelch(lv), grp.squelch(lv)
        for key in a:
            assert np.array_equal(a[key], b[key]), (f, key)
        for k, v in enumerate(lv):
            assert single.output(v).tobytes() == grp.output(v).tobytes(), (f, v)
            p = grp.preroll(v)
            assert single.preroll(v).tobytes() == p.tobytes() and (p.size > 0) == bool(pre[f, k]), (f, v)
        assert single.published == grp.published, f  # order over the whole tree, pre-roll first
        assert single.egress() == grp.egress(), f
        assert single.preroll_count() == grp.preroll_count() and grp.preroll_count()["n_preroll"] == int(pre[f].sum()), f
    single.close()
    grp.close()


# ---- 9. memory, and off ---------------------------------------------------------------------------------------------------
def test_memory_formula_calling_rules_and_off(R):
    from sdrreceiver_amd.receiver import SdrxError
    topo = tp.config3(1024)
    lv = topo.leaves_in_publish_order()
    plain = R.from_topology(topo, device=0)
    off = R.from_topology(topo, device=0, squelch=False, preroll=False)
    meter_only = R.from_topology(topo, device=0, meter=True)
    sq = R.from_topology(topo, device=0, squelch=True)
    on = R.from_topology(topo, device=0, preroll=True)
    every = (plain, off, meter_only, sq, on)
    for rx in every:
        rx.enable_kernel_timing(True)
    with pytest.raises(SdrxError) as e:
        on.preroll(lv[0])  # nothing delivered yet
    assert e.value.code == _lib.SDRX_ESTATE
    for f, x in enumerate(lcg_frames(topo, 3, seed=3)):
        for rx in every:
            rx.process(x)
        for v in lv[::37]:
            assert np.array_equal(off.output(v), plain.output(v)) and np.array_equal(on.output(v), plain.output(v)), (f, v)
    for rx in (plain, meter_only, sq):  # the option off: the calls refuse
        for fn in (lambda: rx.preroll(lv[0]), rx.preroll_count):
            with pytest.raises(SdrxError) as e:
                fn()
            assert e.value.code == _lib.SDRX_ESTATE
    with pytest.raises(SdrxError) as e:
        on.preroll(0)  # a VFO with children
    assert e.value.code == _lib.SDRX_EINVAL
    assert on.preroll_count() == {"n_preroll": 0, "preroll_bytes": 0}
    count = lambda rx: {k: v["launches"] for k, v in rx.kernel_times().items()}  # noqa: E731
    # The eight TIMED kinds are launched as often with every option: the gate's own launches are not among them, so this says
    # nothing about which form of the gate runs.  That preroll = 0 leaves the gate alone rests on device_bytes (below, and
    # tests/test_gpu_squelch.py::test_off_is_untouched) and on the kernel-by-kernel comparison of the ISA.
    assert count(plain) == count(off) == count(sq) == count(on)
    assert off.stats()["device_bytes"] == plain.stats()["device_bytes"]
    pay = sum(squelch.align64(plain.output(v).nbytes) for v in lv)
    L = len(lv)
    # squelch over meter: as DESIGN.md 4f has it
    assert sq.stats()["device_bytes"] - meter_only.stats()["device_bytes"] == 2 * pay + 2 * squelch.align64(64 + 8 * L) + (16 + 16 + 4) * L
    # preroll over squelch: the packed buffers double, the directories gain 4 bytes per leaf, prev_open 4 per leaf
    grown = 2 * max(pay, 64) + 2 * (squelch.align64(64 + 12 * L) - squelch.align64(64 + 8 * L)) + 4 * L
    assert on.stats()["device_bytes"] - sq.stats()["device_bytes"] == grown
    for rx in every:
        rx.close()


# ---- 10. a refused finalize ----------------------------------------------------------------------------------------------
def test_a_second_finalize_after_a_refused_one_starts_clean(R):
    """More leaves than the gate handles: sdrx_finalize refuses in squelch_setup, AFTER the payload buffers of the preroll
    layout were laid out.  The caller switches preroll off and finalizes the same context again: nothing of the refused
    attempt may stay behind -- not the squelch and meter options that preroll implied, not the layout of the packed
    buffers -- so the context is then a plain one, byte for byte and in device_bytes."""
    from sdrreceiver_amd.receiver import SdrxError
    topo = tp.config3(65538)
    lv = topo.leaves_in_publish_order()
    assert len(lv) > 65536
    rx = R(device=0, preroll=True)
    for d in topo.vfos:
        rx.add_vfo(d)
    with pytest.raises(SdrxError) as e:
        rx.finalize()
    assert e.value.code == _lib.SDRX_EUNSUPPORTED
    rx._chk(rx.L.sdrx_set_option(rx.h, b"preroll", 0))
    rx.finalize()  # (still refused if "squelch" had stayed implied)
    plain = R.from_topology(topo, device=0)
    assert rx.stats()["device_bytes"] == plain.stats()["device_bytes"]
    for fn in (lambda: rx.squelch(lv[:1]), lambda: rx.meters(lv[:1]), rx.preroll_count):
        with pytest.raises(SdrxError) as e:
            fn()
        assert e.value.code == _lib.SDRX_ESTATE  # the options are off again
    rx.set_publish(False)
    plain.set_publish(False)
    for f, x in enumerate(lcg_frames(topo, 2, seed=9)):
        rx.process(x)
        plain.process(x)
        for v in lv[::997] + lv[-3:]:
            assert rx.output(v).tobytes() == plain.output(v).tobytes() and rx.output(v).size > 0, (f, v)
        assert rx.egress() == plain.egress(), f
    rx.close()
    plain.close()
