"""Option "tail_in_levels" (include/sdrx.h): the USB demodulation of the frame that left the last tree level
rides in the next step's launch (k_levels_tail) instead of a k_usb_demod launch of its own.  Everything here holds the fused
form to the two-launch form (tail_in_levels = 0) bit for bit, checks where the planner must refuse the fusion (frame parity of
the leaf streams), and that the extra pipeline stage changes nothing a caller sees: fetch, sync, drain."""
import numpy as np
import pytest

from helpers import bits, golden_topology, random_topology
from oracle import binding as ob
from sdrreceiver_amd import synth, topology as tp

pytestmark = pytest.mark.gpu


def _frames(topo, n, seed=1, tones=None):
    lcg = synth.Lcg(seed)
    out = []
    for f in range(n):
        iq = synth.lcg_frame(topo.frame, lcg)
        if tones:
            iq = iq + synth.tone_frame(topo.frame, topo.fs, tones, f * topo.frame)
        out.append(iq)
    return out


def _leaves(topo):
    return [i for i in range(len(topo.vfos)) if not topo.children(i)]


def _check_oracle(rx, nodes, topo, ctx):
    for i, v in enumerate(topo.vfos):
        got = rx.stream(i, missing_ok=True)
        assert got is None or np.array_equal(bits(got), bits(nodes[i].stream())), (ctx, i, "stream")
        if not topo.children(i):
            want = nodes[i].usb() if v.demod_usb else nodes[i].iq()
            assert np.array_equal(rx.output(i), want), (ctx, i, "payload")


def _run_device(rx, topo, dev, fetch_at=None, sync_at=None):
    """queue `dev` back to back with sdrx_process_device; returns the payloads served by a fetch after frame `fetch_at` and at
    the end"""
    mid = None
    for f, d in enumerate(dev):
        rx.process_device(d.data_ptr(), topo.frame)
        if f == sync_at:
            rx.sync()
        if f == fetch_at:
            rx.fetch()
            mid = {i: rx.output(i).copy() for i in _leaves(topo)}
    rx.fetch()
    return mid, {i: rx.output(i).copy() for i in _leaves(topo)}


def _launches(rx):
    return {k: v["launches"] for k, v in rx.kernel_times().items()}


def _mix_launches(kt):
    return sum(kt.get(k, 0) for k in ("k_mix_levels", "k_mix_decimate(level0)", "k_mix_decimate(sub)"))


@pytest.mark.parametrize("key", ["config3-64", "profile_25e"])
def test_one_launch_per_steady_state_step(key):
    """config 3's tree: with the option every step is ONE launch (no k_usb_demod at all, one more launch to drain the extra
    stage); without it a k_usb_demod launch follows every frame's last level."""
    import torch
    from sdrreceiver_amd.receiver import Receiver
    topo = tp.config3(64) if key == "config3-64" else golden_topology(key)
    dev = [torch.from_numpy(iq).cuda() for iq in _frames(topo, 6, seed=5)]
    torch.cuda.synchronize()
    got = {}
    for tail in (True, False):
        rx = Receiver.from_topology(topo, exact=True, tail_in_levels=tail)
        rx.enable_kernel_timing(True)
        _, got[tail] = _run_device(rx, topo, dev)
        kt = _launches(rx)
        n_levels = rx.stats()["n_levels"]
        assert n_levels == 2, n_levels
        if tail:
            assert kt.get("k_usb_demod", 0) == 0, kt
            assert _mix_launches(kt) == len(dev) + n_levels, kt
        else:
            assert kt.get("k_usb_demod", 0) == len(dev), kt
            assert _mix_launches(kt) == len(dev) + n_levels - 1, kt
        rx.close()
    for i in got[True]:
        assert np.array_equal(got[True][i], got[False][i]), (key, i)


@pytest.mark.parametrize("key", ["profile_25e", "54w", "compress", "config1"])
def test_fetch_and_sync_serve_the_right_frame(key):
    """A fetch in the middle of a run serves the frame handed over last, an sdrx_sync drains the extra stage and the pipeline
    fills again: streams and payloads equal the oracle's after the mid-run fetch and at the end."""
    import torch
    from sdrreceiver_amd.receiver import Receiver
    topo = golden_topology(key)
    frames = _frames(topo, 7, seed=21, tones=[(topo.fs / 7.3, 20.0)])
    dev = [torch.from_numpy(iq).cuda() for iq in frames]
    torch.cuda.synchronize()
    nodes, roots = ob.build_tree("port", topo)
    rx = Receiver.from_topology(topo, exact=True, keep_streams=True, tail_in_levels=True)
    for f, d in enumerate(dev):
        rx.process_device(d.data_ptr(), topo.frame)
        ob.process_roots(roots, frames[f])
        if f == 1:
            rx.sync()
        if f == 3:
            rx.fetch()
            _check_oracle(rx, nodes, topo, (key, "mid-run fetch"))
    rx.fetch()
    _check_oracle(rx, nodes, topo, (key, "end"))
    # a synchronous frame after pipelined ones: the extra stage is flushed first, the frame runs on its own
    rx.process(frames[0])
    ob.process_roots(roots, frames[0])
    _check_oracle(rx, nodes, topo, (key, "sdrx_process after the pipeline"))
    rx.close()


def _vfo(parent, fs, n, d, usb=True, bw=0, topic="X", late=0):
    from sdrreceiver_amd.topology import VfoDesc, _g
    return VfoDesc(topic=topic, parent=parent, fs=fs, decimate_count=d, mixer_freq=float(fs // 9), demod_usb=usb, late_decimate=late,
                   filter_bw=bw, gain=_g(0.05), cstyle=1, samples_per_buffer=n)


def _parity_trees():
    """trees at the edge of the frame-parity rule: the fusion needs every demodulated leaf on the last level"""
    from sdrreceiver_amd.topology import Topology
    n, fs = 16 * 128 * 6, 16 * 128 * 6 * 2  # 12 288 samples at 24 576 S/s
    out = {}
    t = Topology(fs=fs, frame=n, name="depth1")  # one level: no k_mix_levels pipeline at all
    t.vfos += [_vfo(-1, fs, n, 2, topic="A"), _vfo(-1, fs, n, 3, bw=fs // 40, topic="B")]
    out["depth 1"] = (t, False, {})
    t = Topology(fs=fs, frame=n, name="two")  # the reference's shape: demodulated leaves on the last level
    t.vfos += [_vfo(-1, fs, n, 2, usb=False), _vfo(0, fs // 4, n // 4, 1, topic="A"), _vfo(0, fs // 4, n // 4, 2, bw=fs // 60, topic="B")]
    out["two levels"] = (t, True, {})
    t = Topology(fs=fs, frame=n, name="pless")  # a parent-less USB leaf beside a two-level tree: level n - 2
    t.vfos += [_vfo(-1, fs, n, 2, usb=False), _vfo(0, fs // 4, n // 4, 1, topic="A"), _vfo(-1, fs, n, 3, topic="P")]
    out["parent-less leaf"] = (t, False, {})
    t = Topology(fs=fs, frame=n, name="pless-iq")  # ... an IQ (compress) leaf there instead: its tail stays where it was
    t.vfos += [_vfo(-1, fs, n, 2, usb=False), _vfo(0, fs // 4, n // 4, 1, topic="A"), _vfo(-1, fs, n, 3, usb=False, topic="Q")]
    out["parent-less IQ leaf"] = (t, True, {})
    t = Topology(fs=fs, frame=n, name="three")  # three levels, demodulated leaves on levels 1 and 2
    t.vfos += [_vfo(-1, fs, n, 1, usb=False), _vfo(0, fs // 2, n // 2, 1, usb=False), _vfo(1, fs // 4, n // 4, 1, topic="A"),
               _vfo(0, fs // 2, n // 2, 2, topic="B")]
    out["three levels, a leaf on level 1"] = (t, False, {})
    f4 = 4 * fs
    t = Topology(fs=f4, frame=n, name="three-last")  # three levels, every demodulated leaf on the last; B's /6 late decimation
    t.vfos += [_vfo(-1, f4, n, 1, usb=False), _vfo(0, f4 // 2, n // 2, 1, usb=False),  # runs in k_late_decimate4 behind the launch
               _vfo(1, f4 // 4, n // 4, 1, topic="A"), _vfo(1, f4 // 4, n // 4, 1, bw=400, topic="B", late=6)]  # that finished the frame
    out["three levels, leaves on the last"] = (t, True, {})
    t = Topology(fs=fs, frame=n, name="three-late")  # a d = 0 leaf with the /6 low-pass in the mix wave: 9.6 KB of LDS per wave,
    t.vfos += [_vfo(-1, fs, n, 1, usb=False), _vfo(0, fs // 2, n // 2, 1, usb=False),  # four waves' worth would fit fewer waves on
               _vfo(1, fs // 4, n // 4, 1, topic="A"), _vfo(1, fs // 4, n // 4, 0, bw=200, topic="B", late=6)]  # a CU: two launches
    out["three levels, fused late decimation"] = (t, False, {})
    return out


@pytest.mark.parametrize("case", sorted(_parity_trees()))
def test_planner_fuses_only_where_frame_parity_allows(case):
    """Launch k writes frame k - l into the parity-(k - l) buffers of a level-l leaf and demodulates frame k - n_levels: only
    leaves of the last level leave that frame untouched until it is read.  Where the rule fails the two-launch form stays (a
    k_usb_demod launch per frame); either way every stream and payload equals the oracle's, and the two forms are bit-identical."""
    import torch
    from sdrreceiver_amd.receiver import Receiver
    topo, fused, opts = _parity_trees()[case]
    frames = _frames(topo, 7, seed=3, tones=[(topo.fs / 5.3, 30.0)])
    dev = [torch.from_numpy(iq).cuda() for iq in frames]
    torch.cuda.synchronize()
    nodes, roots = ob.build_tree("port", topo)
    for iq in frames:
        ob.process_roots(roots, iq)
    got = {}
    for tail in (True, False):
        rx = Receiver.from_topology(topo, exact=True, keep_streams=True, tail_in_levels=tail, **opts)
        rx.enable_kernel_timing(True)
        _, got[tail] = _run_device(rx, topo, dev, sync_at=2)
        kt = _launches(rx)
        demods = kt.get("k_usb_demod", 0)
        if tail and fused:
            assert demods == 0, (case, kt)
        elif any(v.demod_usb for v in topo.vfos):
            assert demods == len(dev), (case, tail, kt)
        _check_oracle(rx, nodes, topo, (case, tail))
        rx.close()
    for i in got[True]:
        assert np.array_equal(got[True][i], got[False][i]), (case, i)


N_SEEDS = 40


def test_random_trees_bit_identical_to_two_launches():
    """40 seeded random trees (1-3 levels, late decimation, long and short low-passes, IQ leaves), 6 frames back to back with a
    mid-run fetch and, for odd seeds, an sdrx_sync: tail_in_levels 1 and 0 serve bit-identical payloads at both points, and the
    last frame's equal the oracle's."""
    import torch
    from sdrreceiver_amd.receiver import Receiver, SdrxError
    ran = 0
    for seed in range(N_SEEDS):
        rng = np.random.default_rng(1000 + seed)
        topo = random_topology(rng)
        frames = _frames(topo, 6, seed=seed, tones=[(topo.fs / 7.3, 20.0)])
        got = {}
        try:
            for tail in (True, False):
                rx = Receiver.from_topology(topo, exact=True, segments=seed % 3, fuse_demod=seed % 4 == 3, tail_in_levels=tail)
                dev = [torch.from_numpy(iq).cuda() for iq in frames]
                torch.cuda.synchronize()
                got[tail] = _run_device(rx, topo, dev, fetch_at=3, sync_at=1 if seed % 2 else None)
                if tail:
                    nodes, roots = ob.build_tree("port", topo)
                    for iq in frames:
                        ob.process_roots(roots, iq)
                    _check_oracle(rx, nodes, topo, ("random", seed))
                rx.close()
        except SdrxError as e:
            assert "fs >= 1024" in str(e) or "last chunk shorter than 256" in str(e), (seed, str(e))
            continue
        for part in (0, 1):
            for i in got[True][part]:
                assert np.array_equal(got[True][part][i], got[False][part][i]), (seed, part, i)
        ran += 1
    assert ran >= N_SEEDS * 9 // 10, ran


# (workload, arithmetic) -> does the planner fuse on a 256-CU MI355X: up to 64 demodulation blocks per CU in the exact arithmetic,
# 16 in the others (sdrx_finalize.hip build_level_plan)
FUSES = {("config3", "exact"): True, ("config3", "tolerance"): False, ("config3", "robust"): False, ("10k", "exact"): False,
         ("config4", "exact"): True, ("config4", "tolerance"): True, ("config4", "robust"): True}


@pytest.mark.parametrize("key,arith", sorted(FUSES))
def test_every_sub_vfo_bit_identical_to_two_launches(key, arith):
    """config 3 (1 024 subs), 10 240 subs and config 4 (256 late-decimating subs): every leaf's payload after 5 frames queued
    back to back (and at a fetch after the third) is the same with tail_in_levels 1 as with 0, and the planner chose the form
    the measurement chose for that workload."""
    import torch
    from sdrreceiver_amd.receiver import Receiver
    topo = {"config3": lambda: tp.config3(1024), "10k": lambda: tp.config3(10240), "config4": lambda: tp.config4(256)}[key]()
    ex = {"exact": 1, "tolerance": 0, "robust": 2}[arith]
    dev = [torch.from_numpy(iq).cuda() for iq in _frames(topo, 5, seed=11, tones=[(topo.fs / 9.1, 25.0)])]
    torch.cuda.synchronize()
    got = {}
    for tail in (True, False):
        rx = Receiver.from_topology(topo, exact=ex, tail_in_levels=tail)
        rx.enable_kernel_timing(True)
        got[tail] = _run_device(rx, topo, dev, fetch_at=2)
        fused = _launches(rx).get("k_usb_demod", 0) == 0
        assert fused == (tail and FUSES[(key, arith)]), (key, arith, tail, _launches(rx))
        rx.close()
    for part in (0, 1):
        for i in got[True][part]:
            assert np.array_equal(got[True][part][i], got[False][part][i]), (key, arith, part, i)
