"""The device spectrum display and the taps on the lattice of tests/lattice.py and on the random trees of seeds 0-19, every
node a spectrum, under the trees' schedules of live controls, against tests/spectrum_trees_ref.py (spectrum_ref.Display fed
the MODEL streams; nothing of the expectation comes from the device).

What k_spectrum reads here and in no other test: tile-layout streams shorter than 8 192 samples, ending inside a chunk and
shorter than one chunk (spec_tiled_index under n_in < 8192); natural-order leaves of 15 ... 240 samples behind their history
prefix; raw frames of 3 840 ... 6 048 samples; three tree levels under the software pipeline of frames queued back to back
(SpecDesc::level, spec_level_frame) and its draining; several tapped fused leaves at once -- the arena's tap buffer and
buffers of their own -- parked, retuned and unparked, and re-pointed by sdrx_set_tap / sdrx_add_tap between frames.

Bars: bins and `updates` bit for bit; pwr, smooth, maxval and aveval within test_gpu_spectrum.TOL = 1e-9 dB (the kernel
sums aveval as a tree: spectrum.hip bounds that by 1e-12 dB).  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import catchup_ref as cr
import lattice as lt
import live_ref as lr
import spectrum_ref as sr
import spectrum_trees_ref as st
from sdrreceiver_amd import _lib
from test_gpu_live_random import _apply_ops, _create, _drive, _options
from test_gpu_live_random import _check_exact as _check_model
from test_gpu_spectrum import check

pytestmark = pytest.mark.gpu

TREES = lt.trees()
NAMES = sorted(TREES)
SEGMENTS = [0, 1, 2, 3, 5]
FORMS = ["process", "submit", "device"]
RAW = _lib.SPECTRUM_RAW


@pytest.fixture(scope="module")
def Receiver():
    from sdrreceiver_amd.receiver import Receiver as R
    return R


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _frames(name):
    return [np.array(iq) for iq in lt.frames(name)]


def _enable(rx, topo, plan, raw=True):
    """add_tap on every leaf of plan["tapped"] (in id order: the first gets the arena's buffer), then a spectrum on every
    node and on the raw frame."""
    for i in plan["tapped"]:
        rx.add_tap(i)
    for i in range(len(topo.vfos)):
        rx.set_spectrum(i)
    if raw:
        rx.set_spectrum(RAW)


def _check_states(rx, topo, states, raw, plan, streams, ctx):
    """Every node's display against states[i] (the untapped leaf's against the zero state), the raw frame's against `raw`,
    sdrx_get_spectrum_levels of all of them against the single read-outs, and the streams of the fused leaves: a tapped one
    has the model's, bit for bit, in every frame in which it is active; the untapped one has none."""
    n = len(topo.vfos)
    got = {}
    for i in range(n):
        got[i] = rx.spectrum(i)
        assert got[i]["n_in"] == min(st.stream_len(topo, i), sr.N), (ctx, i, "n_in")
        check(got[i], st.ZERO if i in plan["untapped"] else states[i], (ctx, i, st.cell(topo, i)))
    ids = list(range(n))
    if raw is not None:
        got[RAW] = rx.spectrum(RAW)
        assert got[RAW]["n_in"] == min(topo.frame, sr.N), (ctx, "raw n_in")
        check(got[RAW], raw, (ctx, "raw"))
        ids.append(RAW)
    lv = rx.spectrum_levels(ids)
    for k, i in enumerate(ids):
        assert (lv["maxval"][k], lv["aveval"][k], int(lv["updates"][k])) == (got[i]["maxval"], got[i]["aveval"], got[i]["updates"]), (ctx, i, "levels")
    for i in plan["tapped"]:
        z, w = rx.stream(i, missing_ok=True), streams[i]
        if w is None:
            assert z is None, (ctx, i, "a parked tapped leaf has a stream")
        else:
            assert z is not None and np.array_equal(_bits(z), _bits(w)), (ctx, i, "the stream of a tapped fused leaf")
    for i in plan["untapped"]:
        assert got[i]["updates"] == 0 and rx.stream(i, missing_ok=True) is None, (ctx, i, "an untapped fused leaf")


def _run_tree(rx, topo, opts, frames, sched, want, states, form, ctx, seed, alongside=None):
    """The schedule through _drive; the displays after every delivered frame whose spectra can be read: every frame of the
    process form, every fetch of the device form, and in the submit form the frames after which nothing is in flight (in
    front of every schedule step and at the end: sdrx_get_spectrum refuses while a frame is)."""
    plan = st.tap_plan(topo, opts)
    _enable(rx, topo, plan)
    raw = st.raw_display(frames)
    checked = []

    def chk(f, readable):
        if alongside is not None:
            alongside(f, readable)
        if readable:
            _check_states(rx, topo, states[f], raw[f], plan, want[f]["streams"], (ctx, "frame", f))
            checked.append(f)

    seen = _drive(rx, topo, frames, sched, form, chk, seed)
    assert seen and seen[-1] == len(frames) - 1 and checked and checked[-1] == len(frames) - 1, (ctx, seen, checked)
    assert form != "process" or checked == list(range(len(frames))), (ctx, checked)


# ------------------------------------------------------------------------------ the lattice, exact arithmetic
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("form", FORMS)
def test_lattice_every_node_a_spectrum(Receiver, form, name):
    """lattice.schedule -- a d >= 6 leaf, a late leaf (in the late0 trees a tapped fused one) and an IQ leaf parked for two
    frames, the deepest sub leaf and the deepest inner node retuned, a gain change -- with the default streams: the fused
    /5 and /6 leaves are tapped but one."""
    k = NAMES.index(name)
    topo = TREES[name]
    want, _ = lt.model_frames(name)
    opts = dict(segments=SEGMENTS[k % 5])
    rx = Receiver.from_topology(topo, exact=True, park=True, meter=True, **opts)
    _run_tree(rx, topo, opts, _frames(name), lt.schedule(topo), want, st.lattice_displays(name), form, ("lattice", name, form, opts), k)
    rx.close()


@pytest.mark.parametrize("name", NAMES)
def test_lattice_frames_queued_back_to_back_one_fetch(Receiver, name):
    """All frames through sdrx_process_device with nothing between them and ONE fetch at the end: level l of the one launch
    works on frame k - l, so every level's spectrum must pick its own frame's parity (frame_level), and the fetch drains the
    pipeline with spectra on every level.  No schedule: a call between two frames would drain it."""
    import torch
    k = NAMES.index(name)
    topo = TREES[name]
    frames = _frames(name)
    opts = dict(segments=SEGMENTS[k % 5])
    plan = st.tap_plan(topo, opts)
    rx = Receiver.from_topology(topo, exact=True, **opts)
    _enable(rx, topo, plan)
    dev = [torch.from_numpy(iq).cuda() for iq in frames]
    torch.cuda.synchronize()
    for d in dev:
        rx.process_device(d.data_ptr(), topo.frame)
    rx.fetch()
    last = len(frames) - 1
    streams = [s.stream() for s in lt.oracle_frames(name)[last]]
    _check_states(rx, topo, st.lattice_plain_displays(name), st.raw_display(frames)[last], plan, streams, ("queued", name, opts))
    rx.close()


LAUNCH_OPTIONS = {"two streams": dict(pipeline=True), "separate kernels": dict(fuse=False),
                  "no frame pipeline": dict(frame_pipeline=False), "demodulation behind the levels": dict(tail_in_levels=False),
                  "demodulation in the wave": dict(fuse_demod=True)}
OPTION_TREES = ("inner", "sub-3840", "late0-2400", "late-deep")


@pytest.mark.parametrize("mode", sorted(LAUNCH_OPTIONS))
@pytest.mark.parametrize("form", FORMS)
def test_lattice_launch_options(Receiver, form, mode):
    """The options that move the spectrum launch: pipeline = 1 puts it on the tail stream; fuse = 0, frame_pipeline = 0 and
    tail_in_levels = 0 change which launch it follows; fuse_demod = 1 leaves the d = 2 leaves of the sub trees with a tap
    buffer instead of a stream."""
    for name in OPTION_TREES:
        k = NAMES.index(name)
        topo = TREES[name]
        want, _ = lt.model_frames(name)
        opts = dict(LAUNCH_OPTIONS[mode], segments=SEGMENTS[k % 5])
        rx = Receiver.from_topology(topo, exact=True, park=True, meter=True, **opts)
        _run_tree(rx, topo, opts, _frames(name), lt.schedule(topo), want, st.lattice_displays(name), form, ("options", name, form, opts), k)
        rx.close()


# ------------------------------------------------------------------------------ the random trees
@pytest.mark.parametrize("form", FORMS)
def test_random_trees_every_node_a_spectrum(Receiver, form):
    """Seeds 0-19 (every residue of _options' rotation) under live_ref.random_schedule: parks, restarts between two frames,
    retunes of inner nodes above the spectra, three levels on 16 of the trees.  test_gpu_live_random's own checker runs
    alongside: the spectra change no payload, meter or stream."""
    ran = 0
    for seed in st.SEEDS:
        topo, frames, sched, want, _, _ = lr.reference(seed)
        opts = _options(seed)
        rx = _create(lambda: Receiver.from_topology(topo, exact=True, park=True, meter=True, **opts), seed)
        if rx is None:
            continue
        ctx = ("random", seed, form, opts)
        _run_tree(rx, topo, opts, frames, sched, want, st.random_displays(seed), form, ctx, seed,
                  alongside=lambda f, s: _check_model(rx, topo, want[f], f, ctx, s))
        rx.close()
        ran += 1
    print(f"{form}: {ran} of {len(st.SEEDS)} random trees ran")
    assert ran >= 18, ran


# ------------------------------------------------------------------------------ taps that move
@pytest.mark.parametrize("name,keep", [("late0-2400", 1), ("sub-8704", 0)])
def test_taps_move_between_frames(Receiver, name, keep):
    """fuse_demod = 1; every fused leaf tapped for frames 0 and 1; then sdrx_set_tap(one of them) -- the others' buffers are
    freed, their `updates` stop and their display state reads back as it was --; sdrx_add_tap of the others after frame 2 --
    updates resume on frame 3: a tap serves from the next frame on --; sdrx_set_tap(-1) after frame 3.  Under lattice.schedule,
    which in late0-2400 parks the first fused leaf for frames 1 and 2: its tap is dropped and added again while it is parked."""
    topo = TREES[name]
    want, _ = lt.model_frames(name)
    sched = lt.schedule(topo)
    opts = dict(fuse_demod=True)
    fused = [i for i in range(len(topo.vfos)) if st.keeps_no_stream(topo, i, opts)]
    assert len(fused) == (4 if name == "late0-2400" else 2)
    kept = fused[keep]
    tapped_in = [set(fused), set(fused), {kept}, set(fused), set()]
    states = st.displays(want, len(topo.vfos), lambda f, i: i not in fused or i in tapped_in[f])
    rx = Receiver.from_topology(topo, exact=True, park=True, **opts)
    _enable(rx, topo, dict(tapped=fused), raw=False)
    none = dict(tapped=[], untapped=[])
    for f, iq in enumerate(_frames(name)):
        _apply_ops(rx, sched[f])
        rx.process(iq)
        ctx = ("taps", name, f)
        _check_states(rx, topo, states[f], None, none, None, ctx)
        for i in fused:
            z, w = rx.stream(i, missing_ok=True), want[f]["streams"][i]
            if w is None or i not in tapped_in[f]:
                assert z is None, (ctx, i, "a stream without a tap, or of a parked leaf")
            else:
                assert z is not None and np.array_equal(_bits(z), _bits(w)), (ctx, i, "stream")
        if f == 1:
            rx.set_tap(kept)
        elif f == 2:
            for i in fused:
                if i != kept:
                    rx.add_tap(i)
        elif f == 3:
            rx.set_tap(-1)
        if f in (1, 2, 3):  # the call itself changes no display
            _check_states(rx, topo, states[f], None, none, None, (ctx, "after the tap call"))
    others = sorted({states[-1][i].updates for i in fused if i != kept})
    assert states[-1][kept].updates == 4 and others in ([3], [2, 3]), (name, others)  # (2: the leaf the schedule parks)
    rx.close()


def test_disable_and_enable_restart_one_spectrum_and_leave_the_others(Receiver):
    """On `inner`: the level-1 inner node of 4 096 samples (tile layout) and the shortest leaf that the schedule never parks
    lose their spectrum after frame 1 and get it back after frame 2: the state restarts zeroed and counts frames 3 and 4;
    every other spectrum goes on as if nothing had happened."""
    from sdrreceiver_amd.receiver import SdrxError
    name = "inner"
    topo = TREES[name]
    want, _ = lt.model_frames(name)
    sched = lt.schedule(topo)
    parked = {i for ops in sched for op in ops if op[0] == "park" for i in op[1]}
    n = len(topo.vfos)
    tiled = next(i for i in range(n) if st.cell(topo, i) == ("tiled", 1, "full"))
    short = min((i for i in range(n) if not topo.children(i) and i not in parked), key=lambda i: (st.stream_len(topo, i), i))
    assert st.stream_len(topo, short) < 1024 and st.stream_len(topo, tiled) == 4096
    both = (tiled, short)
    states = st.lattice_displays(name)
    again = st.displays(want[3:], n)
    rx = Receiver.from_topology(topo, exact=True, park=True)
    _enable(rx, topo, dict(tapped=[]), raw=False)
    for f, iq in enumerate(_frames(name)):
        _apply_ops(rx, sched[f])
        rx.process(iq)
        for i in range(n):
            ctx = ("re-enable", f, i)
            if i in both and f == 2:
                with pytest.raises(SdrxError) as e:
                    rx.spectrum(i)
                assert e.value.code == _lib.SDRX_ESTATE, ctx
            elif i in both and f > 2:
                check(rx.spectrum(i), again[f - 3][i], ctx)
            else:
                check(rx.spectrum(i), states[f][i], ctx)
        if f == 1:
            for i in both:
                rx.set_spectrum(i, False)
        elif f == 2:
            for i in both:
                rx.set_spectrum(i)
                check(rx.spectrum(i), st.ZERO, ("re-enabled", i))
    assert [again[-1][i].updates for i in both] == [2, 2]
    rx.close()


# ------------------------------------------------------------------------------ tolerance and robust arithmetic
@pytest.mark.parametrize("name", NAMES[::2])
@pytest.mark.parametrize("exact", [0, 2])
def test_lattice_tolerance_arithmetics(Receiver, exact, name):
    """exact = 0 and 2 under the schedule, keep_streams on: the display is fed sdrx_get_stream of each frame, as
    tests/test_gpu_spectrum.py does -- the bins are kiss_fft's, bit for bit, of whatever stream that arithmetic produced."""
    k = NAMES.index(name)
    topo = TREES[name]
    want, _ = lt.model_frames(name)
    sched = lt.schedule(topo)
    n = len(topo.vfos)
    rx = Receiver.from_topology(topo, exact=exact, park=True, keep_streams=True, segments=SEGMENTS[k % 5])
    _enable(rx, topo, dict(tapped=[]), raw=False)
    disp = [sr.Display() for _ in range(n)]
    for f, iq in enumerate(_frames(name)):
        _apply_ops(rx, sched[f])
        rx.process(iq)
        for i in range(n):
            z = rx.stream(i, missing_ok=True)
            assert (z is None) == (want[f]["streams"][i] is None), (name, exact, f, i, "which leaves are parked")
            if z is not None:
                disp[i].update(z)
            check(rx.spectrum(i), disp[i], (name, exact, f, i))
    rx.close()


# ------------------------------------------------------------------------------ a group of three members
def _member_spectrum(L, ctx, lid):
    info = _lib.SpectrumInfoC()
    pwr, smooth = np.zeros(sr.N), np.zeros(sr.N - 10)
    bins = np.zeros(2 * sr.N, np.float32)
    assert L.sdrx_get_spectrum(ctx, lid, C.byref(info), pwr.ctypes.data, smooth.ctypes.data, bins.ctypes.data) == 0
    return {"updates": info.updates, "bins": bins.view(np.complex64), "pwr": pwr, "smooth": smooth, "maxval": info.maxval,
            "aveval": info.aveval}


@pytest.mark.parametrize("name", ["sub-3840", "inner"])
def test_group_of_three_members(name):
    """Every node's spectrum through the member context that sdrx_group_locate names (an inner node is replicated: every
    replica is retuned), sdrx_group_set_active and sdrx_group_set_mixer_freqs from lattice.schedule."""
    from sdrreceiver_amd.receiver import Group
    topo = TREES[name]
    sched = lt.schedule(topo)
    states = st.lattice_displays(name)
    g = Group.from_topology(topo, [0, 0, 0], park=1)
    L = _lib.lib()
    where = {i: g.locate(i) for i in range(len(topo.vfos))}
    assert len({m for m, _ in where.values()}) == 3
    for m, lid in where.values():
        assert L.sdrx_set_spectrum(g.member_context(m)[0], lid, 1) == 0
    for f, iq in enumerate(_frames(name)):
        _apply_ops(g, sched[f])
        g.process(iq)
        for i, (m, lid) in where.items():
            check(_member_spectrum(L, g.member_context(m)[0], lid), states[f][i], ("group", name, f, i))
    g.close()


# ------------------------------------------------------------------------------ unpark with catch-up
def _catchup_run(Receiver, key, topo, frames, sched, want, opts, form, seed):
    rx = _create(lambda: Receiver.from_topology(topo, exact=True, catchup=True, meter=True, **opts), seed)
    if rx is None:
        return False
    _run_tree(rx, topo, opts, frames, sched, want, st.catchup_displays(key), form, ("catchup", key, form, opts), seed)
    rx.close()
    return True


@pytest.mark.parametrize("form", ["process", "device"])
def test_catchup_counts_the_frames_from_k_on(Receiver, form):
    """catchup = 1 on sub-8704 under catchup_ref.lattice_schedule and on seeds 0-5: a caught-up leaf runs frame K-1 in the
    catch-up, which updates no spectrum; its display is fed the streams of K, K+1, ... of catchup_ref.CatchupTree
    -- those of a new vfo started on K-1."""
    topo, frames, sched, want, _, _ = cr.reference_lattice("sub-8704")
    assert _catchup_run(Receiver, "sub-8704", topo, frames, sched, want, dict(segments=2), form, 0)
    assert sum(1 for w in want for c in w["caught"].values()) > 0
    ran = 0
    for seed in range(6):
        topo, frames, sched, want, _, _, _ = cr.reference_random(seed)
        ran += _catchup_run(Receiver, seed, topo, frames, sched, want, _options(seed), form, seed)
    assert ran >= 5, ran
