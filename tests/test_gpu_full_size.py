"""Parity at the sizes BASELINE.json's north_star and config 5 quote, on ONE GPU, through the C ABI:
10 240 sub VFOs (the north-star target) and config 5's whole 65 536-sub tree (sdrj.cpp:288-294
fanning out to vfo.cpp:253-264 at scale).

The oracle cannot run 65 538 VFOs inside the suite's budget, so each size is covered by
  (a) the oracle, bit for bit, on a seeded sample of >= 64 sub VFOs spread over both mains PLUS the
      first and the last sub VFO of every block of the 8-way partition topology.shard makes (the
      positions where an off-by-one of the work lists or of the shard would show first);
  (b) properties that hold for ALL VFOs: duplicates of sampled VFOs appended at the far end of the
      tree produce identical payloads; the time segmentation of the decimation kernel (forced to 2
      segments per VFO-frame instead of the library's own choice) does not change one byte of any
      of the 65 536 payloads; an all-zero frame gives all-zero audio everywhere.
"""
import hashlib

import numpy as np
import pytest

from helpers import bits
from oracle import binding as ob
from sdrreceiver_amd import synth, topology as tp

pytestmark = pytest.mark.gpu


def _sample(topo, n_random, seed, world=8):
    """Indices (into topo.vfos) of the sub VFOs to check against the oracle."""
    rng = np.random.default_rng(seed)
    picked = set()
    for r in topo.roots():
        ch = topo.children(r)
        for rank in range(world):
            lo, hi = (len(ch) * rank) // world, (len(ch) * (rank + 1)) // world
            if hi > lo:
                picked.update((ch[lo], ch[hi - 1]))
        picked.update(int(x) for x in rng.choice(ch, size=min(len(ch), n_random // 2), replace=False))
    return sorted(picked)


def _oracle_subset(topo, sample):
    """The mains + the sampled subs as a tree of their own (a VFO's output does not depend on its
    siblings: vfo.cpp:253-264 hands every child the same read-only buffer)."""
    roots = topo.roots()
    remap = {r: k for k, r in enumerate(roots)}
    vf = [topo.vfos[r] for r in roots]
    for i in sample:
        v = topo.vfos[i]
        vf.append(tp.VfoDesc(**{**v.__dict__, "parent": remap[v.parent]}))
    sub = tp.Topology(fs=topo.fs, frame=topo.frame, vfos=vf)
    nodes, oroots = ob.build_tree("port", sub)
    return nodes[len(roots):], oroots


def _payload_digest(rx):
    """One hash over every published payload of the last fetched frame, in publish order."""
    h = hashlib.sha256()
    for topic, rate, payload in rx.published:
        h.update(topic)
        h.update(payload)
    return h.hexdigest(), len(rx.published)


@pytest.mark.parametrize("n_subs", [10240, 65536])
def test_sampled_parity_and_all_vfo_properties(n_subs):
    from sdrreceiver_amd.receiver import Receiver
    topo = tp.config5(n_subs) if n_subs == 65536 else tp.config3(n_subs)
    sample = _sample(topo, 64, seed=n_subs)
    assert len(sample) >= 64 + 16
    dups = sample[:: max(1, len(sample) // 24)]
    for k, i in enumerate(dups):  # duplicates live behind every other node: other work items, other XCDs
        topo.vfos.append(tp.VfoDesc(**{**topo.vfos[i].__dict__, "topic": f"d{k:04d}"[:5]}))
    n_leaves = n_subs + len(dups)
    onodes, oroots = _oracle_subset(topo, sample)
    rx = Receiver.from_topology(topo)
    rx2 = Receiver.from_topology(topo, segments=2)
    frames = 2
    lcg = synth.Lcg(1)
    for f in range(frames):
        iq = synth.lcg_frame(topo.frame, lcg) + synth.tone_frame(topo.frame, topo.fs, [(-377000.0, 25.0), (251000.0, 11.0)], f * topo.frame)
        rx.process(iq)
        rx2.process(iq)
        ob.process_roots(oroots, iq, threads=8)
        for k, i in enumerate(sample):
            assert np.array_equal(rx.output(i), onodes[k].usb()), (n_subs, f, i, "payload")
            assert np.array_equal(bits(rx.stream(i)), bits(onodes[k].stream())), (n_subs, f, i, "stream")
        for k, i in enumerate(dups):
            assert np.array_equal(rx.output(i), rx.output(len(topo.vfos) - len(dups) + k)), (n_subs, f, i, "duplicate")
        d1, n1 = _payload_digest(rx)
        d2, n2 = _payload_digest(rx2)
        assert n1 == n2 == n_leaves and d1 == d2, (n_subs, f, "segmentation changed a payload")
    rx2.close()
    for r in oroots:
        r.free()
    # the zero-frame property needs the zero start-up state: a fresh receiver
    rx.close()
    rx = Receiver.from_topology(topo)
    rx.process(np.zeros(2 * topo.frame, np.float32))
    assert len(rx.published) == n_leaves
    assert all(p.count(0) == len(p) for _, _, p in rx.published)
    rx.close()


def _frames(topo, n, seed=1):
    lcg = synth.Lcg(seed)
    return [synth.lcg_frame(topo.frame, lcg) + synth.tone_frame(topo.frame, topo.fs, [(-377000.0, 25.0), (251000.0, 11.0)], f * topo.frame)
            for f in range(n)]


def _every_sub_vfo_against_the_oracle(topo, n_frames, queued=False, **options):
    """Payload (int16 audio as published) and final cf32 stream of EVERY sub VFO of `topo`, `n_frames` frames, against
    the plain-C oracle.  The oracle keeps a whole NCO table per VFO (oscillator.cpp:13-30: 1.5-3 MB each), so it runs
    the tree in batches of 1 024 sub VFOs on all host cores -- legal because a VFO's output does not depend on its
    siblings (vfo.cpp:253-264).  The GPU side is kept as one sha256 per VFO, frame and kind.

    `queued`: the launch sequence bench.py times -- every frame handed over with sdrx_process_device on a torch stream,
    back to back with no synchronisation in between (ONE k_mix_levels launch per call, level l on frame k - l, the leaf
    tail of the frame that left the last level behind it), ONE sdrx_fetch at the end: the LAST frame's payloads and
    streams are what can be read then, and they are compared (they carry every earlier frame in their NCO phase and
    filter histories)."""
    import os
    from sdrreceiver_amd.receiver import Receiver
    frames = _frames(topo, n_frames)
    rx = Receiver.from_topology(topo, **options)
    subs = [i for i in range(len(topo.vfos)) if topo.vfos[i].parent >= 0]

    def digests():
        out = {}
        for i in subs:
            z = rx.stream(i, missing_ok=True)  # (None: a fused late decimation keeps no decimate[0]; its payload is checked)
            out[i] = (hashlib.sha256(rx.output(i).tobytes()).digest(), None if z is None else hashlib.sha256(z.tobytes()).digest())
        return out

    got = {}
    if queued:
        import torch
        st = torch.cuda.Stream()
        rx.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            dev = [torch.from_numpy(iq).cuda(non_blocking=True) for iq in frames]
            for d in dev:
                rx.process_device(d.data_ptr(), topo.frame)
        rx.fetch()
        assert len(rx.published) == len(subs)
        got[n_frames - 1] = digests()
    else:
        for f, iq in enumerate(frames):
            rx.process(iq)
            assert len(rx.published) == len(subs)
            got[f] = digests()
    rx.close()
    threads = max(1, min(64, len(os.sched_getaffinity(0))))
    checked = 0
    for b in range(0, len(subs), 1024):
        batch = subs[b:b + 1024]
        onodes, oroots = _oracle_subset(topo, batch)
        for f, iq in enumerate(frames):
            ob.process_roots(oroots, iq, threads=threads)
            if f not in got:
                continue
            for k, i in enumerate(batch):
                assert hashlib.sha256(onodes[k].usb().tobytes()).digest() == got[f][i][0], (f, i, "payload")
                assert got[f][i][1] is None or hashlib.sha256(onodes[k].stream().tobytes()).digest() == got[f][i][1], (f, i, "stream")
                checked += 1
        for r in oroots:
            r.free()
    return checked


@pytest.mark.parametrize("workload", ["config3-1024", "north-star-10240", "config4-256"])
def test_every_sub_vfo_in_the_queued_form_bench_times(workload):
    """What bench.py's timed region launches, at the sizes it is quoted on, with the oracle on EVERY sub VFO: 8 frames queued
    with sdrx_process_device on a torch stream (k_mix_levels with the software pipeline over frames: level l works on
    frame k - l), one fetch, payloads and final cf32 streams of the last frame bit-identical to the plain-C oracle.
    BASELINE config 3 (1 024 sub VFOs), the north-star size (10 240) and config 4 (256 fused /5 leaves, whose payloads
    are compared: they keep no decimate[0]).  sdrj.cpp:288-294 -> vfo.cpp:235-296."""
    topo = {"config3-1024": lambda: tp.config3(1024), "north-star-10240": lambda: tp.config3(10240), "config4-256": lambda: tp.config4(256)}[workload]()
    n_subs = sum(1 for v in topo.vfos if v.parent >= 0)
    assert _every_sub_vfo_against_the_oracle(topo, 8, queued=True) == n_subs


REL_TOL = 1e-5  # BASELINE.json north_star: "within 1e-5 relative float tolerance" (of max|ref| per VFO-frame)


def _every_sub_vfo_within_tolerance(topo, n_frames, arith="tolerance"):
    """The TOLERANCE arithmetic (option exact = 0: the table NCO as rotations of its exact checkpoints, the mixer and the
    filters as FMAs) on EVERY sub VFO of `topo`, in the launch form bench.py times (frames queued with
    sdrx_process_device, one fetch): final cf32 stream and pre-quantisation float `usb * gain * 32768` within 1e-5 of
    max|ref|, int16 audio within +-1 LSB of the -O2 oracle's (SURVEY.md 8d's parity criterion).  Returns the worst
    relative errors seen (stream, pre-quantisation) and the share of int16 samples that differ at all."""
    import os
    import torch
    from sdrreceiver_amd.receiver import Receiver
    frames = _frames(topo, n_frames)
    rx = Receiver.from_topology(topo, exact=arith, keep_prequant=True)
    subs = [i for i in range(len(topo.vfos)) if topo.vfos[i].parent >= 0]
    st = torch.cuda.Stream()
    rx.set_stream(st.cuda_stream)
    with torch.cuda.stream(st):
        dev = [torch.from_numpy(iq).cuda(non_blocking=True) for iq in frames]
        for d in dev:
            rx.process_device(d.data_ptr(), topo.frame)
    rx.fetch()
    assert len(rx.published) == len(subs)
    got = {i: (rx.output(i), rx.stream(i, missing_ok=True), rx.prequant(i)) for i in subs}
    rx.close()
    threads = max(1, min(64, len(os.sched_getaffinity(0))))
    worst_s = worst_p = 0.0
    differing = total = 0
    for b in range(0, len(subs), 1024):
        batch = subs[b:b + 1024]
        onodes, oroots = _oracle_subset(topo, batch)
        for iq in frames:
            ob.process_roots(oroots, iq, threads=threads)
        for k, i in enumerate(batch):
            pay, z, pre = got[i]
            if z is not None:
                ref = onodes[k].stream()
                e = float(np.abs(z - ref).max()) / float(np.abs(ref).max())
                assert e <= REL_TOL, (i, "stream", e)
                worst_s = max(worst_s, e)
            pref = onodes[k].usb_prequant()
            e = float(np.abs(pre.astype(np.float64) - pref).max()) / float(np.abs(pref).max())
            assert e <= REL_TOL, (i, "pre-quantisation", e)
            worst_p = max(worst_p, e)
            d = np.abs(pay.astype(np.int32) - onodes[k].usb().astype(np.int32))
            assert d.max() <= 1, (i, "int16 beyond 1 LSB")
            differing += int(np.count_nonzero(d))
            total += d.size
        for r in oroots:
            r.free()
    return worst_s, worst_p, differing / total


@pytest.mark.parametrize("workload,arith", [("config3-1024", "tolerance"), ("north-star-10240", "tolerance"), ("config4-256", "tolerance"),
                                            ("config3-1024", "robust"), ("north-star-10240", "robust"), ("config4-256", "robust")])
def test_every_sub_vfo_in_the_tolerance_arithmetic(workload, arith):
    """north_star's bar ("audio output within 1e-5 of CPU reference") for the arithmetic that spends it: every sub VFO of
    BASELINE config 3, of the 10 240-sub north-star workload and of config 4, 8 queued frames (two wraps of the 384 k
    NCO tables, four of the 192 k ones, one of the 240 k ones with its replayed start-up entries), against the plain-C
    oracle.  oscillator.cpp:4-50, vfo.cpp:237-245."""
    topo = {"config3-1024": lambda: tp.config3(1024), "north-star-10240": lambda: tp.config3(10240), "config4-256": lambda: tp.config4(256)}[workload]()
    ws, wp, frac = _every_sub_vfo_within_tolerance(topo, 8, arith)
    print(f"{workload}, {arith}: worst stream error {ws:.3g}, worst pre-quantisation error {wp:.3g} (of max|ref|); {frac:.3%} of the int16 samples differ by 1 LSB")
    assert ws < REL_TOL and wp < REL_TOL


def test_all_10240_vfos_of_the_north_star_workload_bit_exact():
    """BASELINE.json's north-star size with the oracle on EVERY sub VFO, not a sample: 10 240 sub VFOs under the two
    sdr_25E mains, 2 frames; payloads and final cf32 streams bit-identical to the plain-C oracle."""
    assert _every_sub_vfo_against_the_oracle(tp.config3(10240), 2) == 2 * 10240


def test_all_65536_vfos_of_config5_bit_exact():
    """The same for config 5's whole tree: every one of its 65 536 sub VFOs against the oracle, 2 frames, payloads
    and final cf32 streams (64 oracle batches of 1 024 sub VFOs: 90-113 s on the 64-core host of the MI355X boxes).  Logs of
    earlier exhaustive runs: profiles/r03/exhaustive_config5.txt, profiles/r06/exhaustive_config5.txt."""
    assert _every_sub_vfo_against_the_oracle(tp.config5(65536), 2) == 2 * 65536


def test_config5_in_its_sharded_form_eight_members_of_8192():
    """BASELINE config 5 as `bench.py --gpus 8` and sdrx_group over 8 devices build it: the 65 536-sub
    tree cut into EIGHT shards of 8 192 sub VFOs (mains replicated), here as eight members of one group on
    the one GPU of the test box (sdrj.cpp:288-294 -> vfo.cpp:253-264, fanned out over devices).  One
    synchronous frame + two pipelined ones; the sampled VFOs (incl. the first and last sub of every shard
    block) against the oracle bit for bit, and ONE sha256 over all 65 536 payloads in the reference's
    publish order equal to the single-context run's -- so no shard loses, repeats or reorders a leaf."""
    from sdrreceiver_amd.receiver import Group, Receiver
    topo = tp.config5(65536)
    sample = _sample(topo, 64, seed=5)
    onodes, oroots = _oracle_subset(topo, sample)
    frames = _frames(topo, 3, seed=9)
    want = []
    rx = Receiver.from_topology(topo)
    for iq in frames:
        rx.process(iq)
        want.append(_payload_digest(rx))
    rx.close()
    g = Group.from_topology(topo, [0] * 8)
    st = g.member_stats()
    assert [s["n_leaves"] for s in st] == [8192] * 8 and all(s["n_vfos"] == 8192 + 2 for s in st)
    assert g.peer_access()
    got = []

    def check(f):
        got.append(_payload_digest(g))
        for k, i in enumerate(sample):
            assert np.array_equal(g.output(i), onodes[k].usb()), (f, i, "payload")

    g.process(frames[0])
    ob.process_roots(oroots, frames[0], threads=8)
    check(0)
    g.submit(frames[1])
    g.submit(frames[2])
    for f in (1, 2):
        g.wait()
        ob.process_roots(oroots, frames[f], threads=8)
        check(f)
    for k, i in enumerate(sample):  # the last frame's final cf32 streams, from whichever member holds the VFO
        assert np.array_equal(bits(g.stream(i)), bits(onodes[k].stream())), (i, "stream")
    assert got == want and all(n == 65536 for _, n in got)
    g.close()
    for r in oroots:
        r.free()
