"""Retuning a running tree (sdrx_set_mixer_freqs, sdrx_set_gains and their group forms).

A retune before frame K is `delete osc_mix; osc_mix = new Oscillator(Fs, f)` with every filter state carried over; the
numpy model of tests/retune_ref.py (pinned to liborc by test_retune_model.py) says what every retuned node computes across the
transition.  Nodes that are not retuned still equal the oracle; gain changes equal orc_vfo_set_gain between two frames."""
import ctypes as C
import dataclasses
import time

import numpy as np
import pytest

import retune_ref as rr
from oracle import binding as ob
from sdrreceiver_amd import _lib, synth, topology as tp
from sdrreceiver_amd.topology import Topology, VfoDesc
from helpers import tree_1536

pytestmark = pytest.mark.gpu

N_FRAMES = 6


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def tree_1920() -> Topology:
    """sdr_54W: one main to 240 k, three /5 leaves (48 k, two with the 10 kHz low-pass)."""
    t = Topology(fs=1920000, frame=480000, bufsplit=4, center_frequency=1545939000, name="retune-1920")
    t.vfos.append(VfoDesc(parent=-1, fs=1920000, decimate_count=3, mixer_freq=819000.0, demod_usb=False, cstyle=1,
                          samples_per_buffer=480000))
    c = dict(parent=0, fs=240000, decimate_count=0, late_decimate=5, gain=float(np.float32(0.04)), cstyle=1,
             samples_per_buffer=60000)
    t.vfos.append(VfoDesc(topic="VFO41", mixer_freq=12000.0, filter_bw=10000, **c))
    t.vfos.append(VfoDesc(topic="VFO42", mixer_freq=-30000.0, **c))
    t.vfos.append(VfoDesc(topic="VFO43", mixer_freq=50000.0, filter_bw=10000, **c))
    return t


RETUNES = {  # frame -> [(id, new mixer)]
    "1536": {2: [(2, 112354.0), (4, -40000.0), (6, -60000.0)], 4: [(4, -39000.0)]},
    "1920": {2: [(1, 15000.0), (3, 52000.0)], 4: [(1, 14000.0)]},
}
TREES = {"1536": tree_1536, "1920": tree_1920}


def _frames(topo, n=N_FRAMES, seed=11):
    lcg = synth.Lcg(seed)
    return [synth.lcg_frame(topo.frame, lcg) for _ in range(n)]


def _leaves(topo):
    return [i for i in range(len(topo.vfos)) if not topo.children(i)]


class Drive:
    """Feeds frames to a Receiver in one of three ways and hands back, per frame, what it delivered.  mode "process":
    sdrx_process; "submit": sdrx_submit with a frame in flight wherever no retune follows; "device": sdrx_process_device under
    the frame pipeline, the two frames before a change left inside the pipeline (the change drains them)."""

    def __init__(self, rx, topo, frames, mode, changes_at):
        self.rx, self.topo, self.frames, self.mode, self.changes_at = rx, topo, frames, mode, set(changes_at)
        if mode == "device":
            import torch
            self.dev = [torch.from_numpy(iq).cuda() for iq in frames]
            torch.cuda.synchronize()

    def run(self, apply, check):
        """apply(f): the changes before frame f (called once or more: applies them once); check(f): frame f's results are
        readable."""
        rx, n = self.rx, len(self.frames)
        if self.mode == "process":
            for f in range(n):
                apply(f)
                rx.process(self.frames[f])
                check(f)
        elif self.mode == "submit":
            delivered = 0
            for f in range(n):
                if f in self.changes_at:
                    while rx.in_flight():
                        rx.wait()
                        check(delivered)
                        delivered += 1
                apply(f)
                rx.submit(self.frames[f])
                if rx.in_flight() == 2:
                    rx.wait()
                    check(delivered)
                    delivered += 1
            while rx.in_flight():
                rx.wait()
                check(delivered)
                delivered += 1
        else:
            for f in range(n):
                apply(f)
                rx.process_device(self.dev[f].data_ptr(), self.topo.frame)
                if f + 2 in self.changes_at and f not in self.changes_at:
                    continue  # stays in the pipeline until the change
                if f + 1 in self.changes_at:
                    apply(f + 1)  # drains what the pipeline holds (frames f - 1 and f) with the old values first
                rx.fetch()
                check(f)


def _run_exact(key, mode, exact=True, **opts):
    from sdrreceiver_amd.receiver import Receiver
    topo = TREES[key]()
    sched = RETUNES[key]
    frames = _frames(topo)
    nodes, roots = ob.build_tree("port", topo)
    retuned = sorted({i for ch in sched.values() for i, _ in ch})
    models = {i: rr.Node(topo.vfos[i]) for i in retuned}
    rx = Receiver.from_topology(topo, exact=exact, keep_streams=True, **opts)
    want = {}
    applied = set()

    def apply(f):
        if f in sched and f not in applied:
            ids, fr = zip(*sched[f])
            rx.set_mixer_freqs(list(ids), list(fr))
            applied.add(f)

    for f, iq in enumerate(frames):  # the references, frame by frame
        ob.process_roots(roots, iq)
        w = {}
        for i in _leaves(topo):
            if i in models:
                if f in sched:
                    for j, fq in sched[f]:
                        if j == i:
                            models[i].retune(fq)
                z = models[i].process(nodes[topo.vfos[i].parent].stream())
                w[i] = (z, models[i].payload())
            else:
                v = nodes[i]
                w[i] = (v.stream(), v.usb() if topo.vfos[i].demod_usb else v.iq())
        want[f] = w
    seen = []

    def check(f):
        for i, (z, pay) in want[f].items():
            got_pay = rx.output(i)
            got_z = rx.stream(i) if rx.in_flight() == 0 else None  # (device read-backs wait for the frames in flight)
            if exact is True:
                assert np.array_equal(_bits(got_pay), _bits(pay)), (key, mode, opts, f, i, "payload")
                assert got_z is None or np.array_equal(_bits(got_z), _bits(z)), (key, mode, opts, f, i, "stream")
            else:
                tol = 1e-5 * float(np.abs(z).max())
                assert got_z is not None and float(np.abs(got_z - z).max()) <= tol, (key, mode, exact, f, i, "stream")
                assert int(np.abs(got_pay.astype(np.int32) - pay.astype(np.int32)).max()) <= 1, (key, mode, exact, f, i)
        seen.append(f)

    Drive(rx, topo, frames, mode, sched.keys()).run(apply, check)
    assert {1, 2, 3, 4, 5} <= set(seen), seen  # every frame around both changes was checked
    # the retuned tables are the new oscillators' (sdrx_get_nco)
    for i in retuned:
        f_new = [fq for fr in sorted(sched) for j, fq in sched[fr] if j == i][-1]
        L = topo.vfos[i].fs
        tab = rr.table(L, f_new)
        assert np.array_equal(_bits(rx.nco(i, L - 64, 64)), _bits(tab[L - 64:])), i
    rx.close()


CASES_EXACT = [
    ("1536", "process", dict()),
    ("1536", "submit", dict(fuse_demod=True, tail_in_levels=False)),
    ("1536", "device", dict(fuse_demod=True, tail_in_levels=True)),
    ("1536", "device", dict(fuse_demod=False, tail_in_levels=False)),
    ("1920", "process", dict(fuse_late=True)),
    ("1920", "submit", dict(fuse_late=False)),
    ("1920", "device", dict(fuse_late=True)),
]


@pytest.mark.parametrize("key,mode,opts", CASES_EXACT, ids=[f"{k}-{m}-{'-'.join(f'{a}{int(b)}' for a, b in o.items())}"
                                                            for k, m, o in CASES_EXACT])
def test_retune_exact_across_the_transition(key, mode, opts):
    _run_exact(key, mode, **opts)


@pytest.mark.parametrize("exact", [False, 2])
def test_retune_tolerance_arithmetics(exact):
    """exact = 0 and exact = 2: within 1e-5 of max|stream| and 1 LSB of the model (fed the oracle's parent streams)."""
    _run_exact("1536", "process", exact=exact)


def test_nco_after_retune_is_the_new_oscillator():
    """sdrx_get_nco after a retune equals orc_osc_table(fs, f_new): the start, the wrap, the last entry; main and sub."""
    from sdrreceiver_amd.receiver import Receiver
    topo = tree_1536()
    rx = Receiver.from_topology(topo)
    rx.process(_frames(topo, 1)[0])
    rx.set_mixer_freqs([1, 3], [-497500.0, -2000.0])
    for i, f in ((1, -497500.0), (3, -2000.0), (0, 484000.0)):
        L = topo.vfos[i].fs
        tab = rr.table(L, f)
        for first, count in ((0, 600), (L - 40, 40), (L - 1, 1)):
            assert np.array_equal(_bits(rx.nco(i, first, count)), _bits(tab[first: first + count])), (i, first)


@pytest.mark.parametrize("mode", ["process", "device"])
def test_retune_a_main(mode):
    """A retuned main: its stream is the model's; its unchanged children equal orc_vfo children fed that stream."""
    from sdrreceiver_amd.receiver import Receiver
    topo = tree_1536()
    frames = _frames(topo)
    K, f_new = 2, -497000.0
    main = rr.Node(topo.vfos[1])
    kids = [i for i in range(len(topo.vfos)) if topo.vfos[i].parent == 1]
    sub = Topology(fs=192000, frame=48000, vfos=[dataclasses.replace(topo.vfos[i], parent=-1) for i in kids])
    onodes, _ = ob.build_tree("port", sub)
    want = {}
    for f, iq in enumerate(frames):
        if f == K:
            main.retune(f_new)
        z = main.process(iq.view(np.complex64))
        for o in onodes:
            o.process(z.view(np.float32))
        want[f] = (z, [o.usb() for o in onodes])
    rx = Receiver.from_topology(topo, keep_streams=True)

    def apply(f):
        if f == K and not getattr(apply, "done", False):
            rx.set_mixer_freqs([1], [f_new])
            apply.done = True

    def check(f):
        z, pays = want[f]
        assert np.array_equal(_bits(rx.stream(1)), _bits(z)), (mode, f, "main stream")
        for i, p in zip(kids, pays):
            assert np.array_equal(rx.output(i), p), (mode, f, i)

    Drive(rx, topo, frames, mode, [K]).run(apply, check)
    assert rx.descs[1].mixer_freq == f_new


@pytest.mark.parametrize("mode,opts", [("process", dict(fuse_demod=False)),
                                       ("device", dict(fuse_demod=True, tail_in_levels=True)),
                                       ("device", dict(fuse_demod=False, tail_in_levels=True))])
def test_gains_between_frames_equal_orc_set_gain(mode, opts):
    """k_usb_demod (process), k_levels_tail / the in-wave demodulation (device, frame pipeline), k_lpf_long (VFO25), late
    /5 leaves: set_gains between frames is orc_vfo_set_gain between orc_vfo_process calls.  A main's gain is stored, no effect."""
    from sdrreceiver_amd.receiver import Receiver
    for topo, changes in ((tree_1536(), {1: [(2, 0.5), (4, 0.11), (6, 0.07), (0, 3.0)], 3: [(4, 0.02), (6, 1.5)]}),
                          (tree_1920(), {2: [(1, 0.3), (2, 0.09)]})):
        if mode == "device" and topo.fs == 1920000:
            continue
        frames = _frames(topo, 5)
        nodes, roots = ob.build_tree("port", topo)
        want = {}
        for f, iq in enumerate(frames):
            for i, g in changes.get(f, []):
                if topo.vfos[i].demod_usb:
                    nodes[i].setGain(g)
            ob.process_roots(roots, iq)
            want[f] = {i: (nodes[i].usb() if topo.vfos[i].demod_usb else nodes[i].iq()) for i in _leaves(topo)}
        rx = Receiver.from_topology(topo, **opts)
        done = set()

        def apply(f):
            if f in changes and f not in done:
                ids, g = zip(*changes[f])
                rx.set_gains(list(ids), list(g))
                done.add(f)

        def check(f):
            for i, p in want[f].items():
                assert np.array_equal(rx.output(i), p), (mode, opts, topo.name, f, i)

        Drive(rx, topo, frames, mode, changes.keys()).run(apply, check)
        rx.close()


def test_group_equals_one_context():
    """3 members on device 0: replicated mains and subs in different shards, retuned and re-gained between frames; every
    payload byte-identical to one context given the same calls."""
    from sdrreceiver_amd.receiver import Group, Receiver
    topo = tp.profile_25e()
    topo.vfos = topo.vfos[:8] + topo.vfos[14:20]  # the mains, 6 subs of each
    frames = _frames(topo, 5)
    g = Group.from_topology(topo, [0, 0, 0])
    rx = Receiver.from_topology(topo)
    reps = set(g.locate(i)[0] for i in range(2, len(topo.vfos)))
    assert len(reps) == 3
    retunes = {2: ([1, 2, 5, 9, 13], [-497000.0, topo.vfos[2].mixer_freq + 700, topo.vfos[5].mixer_freq - 900,
                                      topo.vfos[9].mixer_freq + 50, topo.vfos[13].mixer_freq - 2000]),
               3: ([0, 7], [485500.0, topo.vfos[7].mixer_freq + 333])}
    gains = {2: ([3, 10, 12], [0.2, 0.07, 0.5]), 4: ([2], [0.9])}
    for f, iq in enumerate(frames):
        for obj in (g, rx):
            if f in retunes:
                obj.set_mixer_freqs(*retunes[f])
            if f in gains:
                obj.set_gains(*gains[f])
            obj.process(iq)
        for i in _leaves(topo):
            assert np.array_equal(g.output(i), rx.output(i)), (f, i)
        assert g.published == rx.published
    for i in (0, 1):  # every replica of a retuned main has the new table
        for k in range(3):
            ctx, _ = g.member_context(k)
            out = np.zeros(2 * 64, np.float32)
            assert rx.L.sdrx_get_nco(ctx, i, 0, 64, out.ctypes.data) == 0
            assert np.array_equal(out.view(np.complex64), rx.nco(i, 0, 64)), (i, k)
    g.close()
    rx.close()


def test_errors_change_nothing():
    from sdrreceiver_amd.receiver import Receiver, SdrxError
    topo = tree_1536()
    L = _lib.lib()
    rx = Receiver()
    for d in topo.vfos:
        rx.add_vfo(d)
    with pytest.raises(SdrxError) as e:
        rx.set_mixer_freqs([2], [1000.0])
    assert e.value.code == _lib.SDRX_ESTATE
    assert L.sdrx_set_gains(rx.h, None, None, 0) == _lib.SDRX_ESTATE  # before finalize
    rx.finalize()
    frames = _frames(topo, 3)
    nodes, roots = ob.build_tree("port", topo)
    before = {i: rx.nco(i, 0, 256) for i in range(len(topo.vfos))}
    ids = (C.c_int * 2)()
    vals = (C.c_double * 2)()
    gv = (C.c_float * 2)()
    bad = [([2, 99], [1.0, 2.0]), ([-1, 2], [1.0, 2.0]), ([3, 3], [1.0, 2.0]), ([2, 3], [float("nan"), 2.0]),
           ([2, 3], [1.0, float("inf")])]
    for b_ids, b_vals in bad:
        ids[:] = b_ids
        vals[:] = b_vals
        gv[:] = b_vals
        assert L.sdrx_set_mixer_freqs(rx.h, ids, vals, 2) == _lib.SDRX_EINVAL, (b_ids, b_vals)
        assert L.sdrx_set_gains(rx.h, ids, gv, 2) == _lib.SDRX_EINVAL, (b_ids, b_vals)
    assert L.sdrx_set_mixer_freqs(rx.h, ids, vals, -1) == _lib.SDRX_EINVAL
    assert L.sdrx_set_mixer_freqs(rx.h, None, None, 0) == 0
    assert L.sdrx_set_gains(rx.h, None, None, 0) == 0
    assert L.sdrx_set_mixer_freqs(None, ids, vals, 1) == _lib.SDRX_EINVAL
    for i, t in before.items():
        assert np.array_equal(rx.nco(i, 0, 256), t), i
    rx.submit(frames[0])
    ids[:] = [2, 3]
    vals[:] = [1000.0, 2000.0]
    gv[:] = [0.5, 0.25]
    assert L.sdrx_set_mixer_freqs(rx.h, ids, vals, 2) == _lib.SDRX_ESTATE  # in flight
    assert L.sdrx_set_gains(rx.h, ids, gv, 2) == _lib.SDRX_ESTATE
    rx.wait()
    rx.process(frames[1])
    for f in range(2):
        ob.process_roots(roots, frames[f])
    for i in _leaves(topo):  # nothing changed: still the oracle
        want = nodes[i].usb() if topo.vfos[i].demod_usb else nodes[i].iq()
        assert np.array_equal(rx.output(i), want), i
    rx.close()
    from sdrreceiver_amd.receiver import Group
    grp = Group.from_topology(topo, [0, 0])
    ids[:] = [2, 2]
    assert L.sdrx_group_set_mixer_freqs(grp.h, ids, vals, 2) == _lib.SDRX_EINVAL
    assert L.sdrx_group_set_gains(grp.h, None, None, 0) == 0
    grp.submit(frames[0])
    ids[:] = [2, 3]
    assert L.sdrx_group_set_mixer_freqs(grp.h, ids, vals, 2) == _lib.SDRX_ESTATE
    grp.wait()
    grp.close()


def test_config3_mix_offset_drift():
    """Config 3, all 1 024 subs retuned at frame K by mix_offset_retune.  Frame K equals the model (a sample of subs); from
    K + 1 on every sub equals a FRESH orc_vfo sub with the new mixer created at frame K and fed the unchanged main's stream
    from K on -- fresh oscillators agree, and the filters forget what came before K within one frame."""
    from sdrreceiver_amd.receiver import Receiver
    from test_retune_model import config3_ini
    text = config3_ini(1024)
    topo = tp.topology_from_ini(text)
    assert topo.vfos == tp.config3(1024).vfos
    ids, freqs = tp.mix_offset_retune(topo, text, 1500)
    assert len(ids) == 1024
    K, n = 1, 4
    frames = _frames(topo, n, seed=3)
    nodes, roots = ob.build_tree("port", topo)
    sample = ids[::97] + [ids[-1]]
    models = {i: rr.Node(topo.vfos[i]) for i in sample}
    new = dict(zip(ids, freqs))
    fresh_topo = Topology(fs=topo.fs, frame=topo.frame,
                          vfos=[dataclasses.replace(topo.vfos[i], parent=-1, mixer_freq=new[i]) for i in ids])
    fresh, _ = ob.build_tree("port", fresh_topo)
    rx = Receiver.from_topology(topo)
    for f, iq in enumerate(frames):
        if f == K:
            t0 = time.perf_counter()
            rx.set_mixer_freqs(ids, freqs)
            dt = time.perf_counter() - t0
            assert dt < 0.25, f"retune of 1024 subs took {dt * 1e3:.1f} ms"
            for i in sample:
                models[i].retune(new[i])
        rx.process(iq)
        ob.process_roots(roots, iq, threads=16)
        for i in sample:
            models[i].process(nodes[topo.vfos[i].parent].stream())
            p = models[i].payload()
            if f <= K:
                assert np.array_equal(rx.output(i), p), (f, i)
        if f < K:
            for i in ids:
                assert np.array_equal(rx.output(i), nodes[i].usb()), (f, i)
            continue
        for k, i in enumerate(ids):
            fresh[k].process(nodes[topo.vfos[i].parent].stream().view(np.float32))
            if f > K:
                assert np.array_equal(rx.output(i), fresh[k].usb()), (f, i)
    rx.close()
