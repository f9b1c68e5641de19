"""Frames that are already in device memory: sdrx_submit_device, sdrx_group_submit_device and the `producer_stream` of the
group's device calls, and sdrx_process_device / sdrx_submit_device on a caller's stream (sdrx_set_stream) -- against the live
oracle for the frame each payload belongs to.

Bars: the exact arithmetic bit for bit; exact = 0 and exact = 2 within _check_tolerance of test_gpu_parity.py; and whatever
the arithmetic, a frame handed over with sdrx_submit_device delivers exactly what the same frame through sdrx_submit does.
The stream-ordering tests hand the library a buffer that still holds a decoy frame while the true one is being copied in
behind a sleep on the producer's stream: they fail if anything reads the frame before the producer has written it."""
import ctypes as C
import functools

import numpy as np
import pytest

import spectrum_ref as sr
from helpers import bits, golden_topology, random_topology, tree_1536, tree_mixed
from oracle import binding as ob
from sdrreceiver_amd import _lib, synth, topology as tp

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5  # test_gpu_parity.py's _check_tolerance
N_FRAMES = 6
# How long the producer's stream sleeps before it writes the true frame.  Not measured: what a missing wait would need is a
# window far longer than the library takes to queue a frame (well under a millisecond of host time), and tens of
# milliseconds are that.  _sleep_cycles converts it with torch.cuda._sleep's rate measured on the device: on an MI355X about
# 1.06e8 cycles, which one run timed at 44 ms.
PRODUCER_SLEEP_MS = 50.0

TREES = {"profile_25e": lambda: golden_topology("profile_25e"), "54w": lambda: golden_topology("54w"),
         "compress": lambda: golden_topology("compress"), "config3-64": lambda: tp.config3(64), "1536": tree_1536,
         "mixed": tree_mixed}
OPTIONS = {"default": {}, "tail_in_levels=0": dict(tail_in_levels=False), "fuse_demod=1": dict(fuse_demod=True),
           "fuse_late=0": dict(fuse_late=False), "pipeline=1": dict(pipeline=True), "fuse=0": dict(fuse=False)}
# every tree with every option in the exact arithmetic; the other two arithmetics with the options that change the launches an
# egress frame runs through
STEADY_CASES = ([(k, o, 1) for k in TREES for o in OPTIONS]
                + [(k, o, a) for k in TREES for o in ("default", "fuse_demod=1", "pipeline=1") for a in (0, 2)])


def _lcg_frames(topo, n, seed):
    lcg = synth.Lcg(seed)
    return [synth.lcg_frame(topo.frame, lcg) for _ in range(n)]


def _to_device(frames):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(x, np.float32).reshape(-1)).cuda() for x in frames]
    torch.cuda.synchronize()
    return out


def _publishers(topo):
    """the leaves that publish, in the reference's order (an IQ leaf only with a topic)"""
    return [i for i in topo.leaves_in_publish_order() if topo.vfos[i].demod_usb or topo.vfos[i].topic]


def _published(nodes, topo):
    """what the publish callback gets for the frame the oracle processed last: (topic, rate, payload) per publisher"""
    return [(topo.vfos[i].topic.encode()[:5].ljust(5, b"\0"), topo.vfos[i].output_rate,
             (nodes[i].usb() if topo.vfos[i].demod_usb else nodes[i].iq()).tobytes()) for i in _publishers(topo)]


class Oracle:
    """The oracle tree fed frame by frame in the order the library gets them; feed() returns that frame's messages."""

    def __init__(self, topo):
        self.topo = topo
        self.nodes, self.roots = ob.build_tree("port", topo)
        self.dc_state = np.zeros(2, np.float32)

    def feed(self, iq):
        ob.process_roots(self.roots, iq)
        return _published(self.nodes, self.topo)

    def feed_u8(self, b, correct_dc):
        iq = ob.u8_to_float(b)
        if correct_dc:
            ob.dc_correct(iq, self.dc_state)
        return self.feed(iq)


@functools.lru_cache(maxsize=None)
def _oracle_run(key):
    """(topology, frames, messages of every frame, oracle nodes after the last frame) of the steady-state tests"""
    topo = TREES[key]()
    frames = [iq + synth.tone_frame(topo.frame, topo.fs, [(topo.fs / 7.3, 20.0)], f * topo.frame)
              for f, iq in enumerate(_lcg_frames(topo, N_FRAMES, seed=41))]
    o = Oracle(topo)
    want = [o.feed(iq) for iq in frames]
    return topo, frames, want, o.nodes


def _check_exact(rx, nodes, topo, ctx):
    for i, v in enumerate(topo.vfos):
        got = rx.stream(i, missing_ok=True)
        assert got is None or np.array_equal(bits(got), bits(nodes[i].stream())), (ctx, i, "stream")
        if not topo.children(i):
            want = nodes[i].usb() if v.demod_usb else nodes[i].iq()
            assert np.array_equal(rx.output(i), want), (ctx, i, "payload")


def _check_tolerance(rx, nodes, topo, ctx):
    for i, v in enumerate(topo.vfos):
        ref = nodes[i].stream()
        got = rx.stream(i, missing_ok=True)
        scale = float(np.abs(ref).max())
        assert got is None or np.abs(got - ref).max() <= REL_TOL * scale, (ctx, i, "stream", np.abs(got - ref).max() / scale)
        if not topo.children(i) and v.demod_usb:
            pre_ref = nodes[i].usb_prequant()
            pre = rx.prequant(i).astype(np.float64)
            s = float(np.abs(pre_ref).max())
            assert np.abs(pre - pre_ref).max() <= REL_TOL * s, (ctx, i, "prequant", np.abs(pre - pre_ref).max() / s)
            assert np.abs(rx.output(i).astype(np.int32) - nodes[i].usb().astype(np.int32)).max() <= 1, (ctx, i)


def _check_messages_close(got, want, topo, ctx):
    """one frame's messages in the tolerance arithmetics: same topics, rates and lengths, int16 audio within +-1 LSB (an IQ
    payload is held through its stream by _check_tolerance)"""
    pubs = _publishers(topo)
    assert len(got) == len(want) == len(pubs), ctx
    for (t, r, p), (t2, r2, p2), i in zip(got, want, pubs):
        assert (t, r, len(p)) == (t2, r2, len(p2)), (ctx, i)
        if topo.vfos[i].demod_usb:
            d = np.frombuffer(p, np.int16).astype(np.int32) - np.frombuffer(p2, np.int16).astype(np.int32)
            assert np.abs(d).max() <= 1, (ctx, i)


def _steady_state(rx, submit, n):
    """submit(f+1); wait() -> f over n frames, in_flight() checked at every step; the messages of every delivered frame"""
    out = []
    submit(0)
    assert rx.in_flight() == 1
    for f in range(1, n):
        submit(f)
        assert rx.in_flight() == 2, f
        rx.wait()
        assert rx.in_flight() == 1, f
        out.append(list(rx.published))
    rx.wait()
    assert rx.in_flight() == 0
    out.append(list(rx.published))
    return out


def _code(call):
    from sdrreceiver_amd.receiver import SdrxError
    with pytest.raises(SdrxError) as e:
        call()
    return e.value.code


# ---------------------------------------------------------------------------------------------------------- 1. steady state
@pytest.mark.parametrize("key,opt,arith", STEADY_CASES)
def test_submit_device_steady_state(key, opt, arith):
    """submit_device(f+1); wait() -> f with every frame in a device tensor of its own: every delivered frame's messages in the
    reference's order equal the oracle's for THAT frame (exact: bit for bit; else +-1 LSB and the streams within 1e-5) and are
    bit-identical to the same frames through sdrx_submit with the same options."""
    from sdrreceiver_amd.receiver import Receiver
    topo, frames, want, nodes = _oracle_run(key)
    kw = dict(exact=arith, keep_prequant=arith != 1, **OPTIONS[opt])
    dev = _to_device(frames)
    rx = Receiver.from_topology(topo, **kw)
    got = _steady_state(rx, lambda f: rx.submit_device(dev[f].data_ptr(), topo.frame), len(frames))
    host = Receiver.from_topology(topo, **kw)
    ref = _steady_state(host, lambda f: host.submit(frames[f]), len(frames))
    ctx = (key, opt, arith)
    for f in range(len(frames)):
        assert got[f] == ref[f], (ctx, f, "sdrx_submit_device differs from sdrx_submit")
        if arith == 1:
            assert got[f] == want[f], (ctx, f)
        else:
            _check_messages_close(got[f], want[f], topo, (ctx, f))
    (_check_exact if arith == 1 else _check_tolerance)(rx, nodes, topo, ctx)
    for i in range(len(topo.vfos)):
        a, b = rx.stream(i, missing_ok=True), host.stream(i, missing_ok=True)
        assert (a is None) == (b is None) and (a is None or np.array_equal(bits(a), bits(b))), (ctx, i, "stream")
    rx.close()
    host.close()


# ------------------------------------------------------------------------------------------- 2. transitions between paths
TRANSITION_SEEDS = [11, 12, 13, 14]
TRANSITION_FRAMES = 40


def _transition_topology(seed):
    if seed % 4 == 0:
        return golden_topology("profile_25e")
    if seed % 4 == 1:
        return golden_topology("54w")
    if seed % 4 == 2:
        return tree_mixed()
    rng = np.random.default_rng(3000 + seed)
    while True:  # the first draw the library takes (sdrx_check_vfo on the host, and finalize's frame-shape rules)
        topo = random_topology(rng)
        if all(_lib.lib().sdrx_check_vfo(C.byref(_lib.desc_to_c(v)), None, 0) == 0
               and not (0 < v.samples_per_buffer % 1024 < 256) for v in topo.vfos):
            return topo


@pytest.mark.parametrize("seed", TRANSITION_SEEDS)
def test_random_transitions_through_submit_device(seed):
    """One receiver, a seeded random interleaving of process, process_u8 and submit_u8 (with and without the DC-bias
    removal), submit, submit_device, wait, and process_device queued 1-4 deep followed by fetch, sync or nothing at all (the
    next call drains the software pipeline).  Every frame that comes out equals the oracle's for the frame it belongs to."""
    import torch
    from sdrreceiver_amd.receiver import Receiver
    rng = np.random.default_rng(500 + seed)
    topo = _transition_topology(seed)
    rx = Receiver.from_topology(topo, exact=True)
    o = Oracle(topo)
    frames = _lcg_frames(topo, TRANSITION_FRAMES, seed=seed)  # integer valued: also dongle bytes
    order = _publishers(topo)
    want = {}
    pending, keep = [], []
    f, checked, ops = 0, 0, set()

    def as_bytes(iq):
        return (iq + 127).astype(np.uint8)

    def delivered(idx):
        nonlocal checked
        assert rx.published == want[idx], (seed, idx)
        checked += 1

    def device(iq):
        d = torch.from_numpy(np.ascontiguousarray(iq, np.float32)).cuda()
        torch.cuda.synchronize()
        keep.append(d)
        return d

    while f < TRANSITION_FRAMES:
        op = int(rng.integers(0, 7))
        if op in (0, 1) and not pending:
            dc = op == 1 and bool(rng.integers(0, 2))
            want[f] = o.feed_u8(as_bytes(frames[f]), dc) if op == 1 else o.feed(frames[f])
            rx.process_u8(as_bytes(frames[f]), correct_dc=dc) if op == 1 else rx.process(frames[f])
            delivered(f)
            f += 1
        elif op in (2, 3, 4):
            if len(pending) == 2:
                rx.wait()
                delivered(pending.pop(0))
            if op == 2:
                want[f] = o.feed(frames[f])
                rx.submit(frames[f])
            elif op == 3:
                dc = bool(rng.integers(0, 2))
                want[f] = o.feed_u8(as_bytes(frames[f]), dc)
                rx.submit_u8(as_bytes(frames[f]), correct_dc=dc)
            else:
                want[f] = o.feed(frames[f])
                rx.submit_device(device(frames[f]).data_ptr(), topo.frame)
            pending.append(f)
            f += 1
        elif op == 5 and pending:
            rx.wait()
            delivered(pending.pop(0))
        elif op == 6 and not pending:
            for _ in range(min(int(rng.integers(1, 5)), TRANSITION_FRAMES - f)):
                want[f] = o.feed(frames[f])
                rx.process_device(device(frames[f]).data_ptr(), topo.frame)
                f += 1
            what = int(rng.integers(0, 3))
            if what == 0:
                rx.fetch()
                delivered(f - 1)
            elif what == 1:
                rx.sync()
                assert rx.output(order[0]).tobytes() == want[f - 1][0][2], (seed, f - 1)
                checked += 1
        else:
            continue
        ops.add(op)
        assert rx.in_flight() == len(pending), seed
        keep = keep[-12:]  # (at most 2 submitted + 4 queued frames are still the library's to read)
    while pending:
        rx.wait()
        delivered(pending.pop(0))
    rx.close()
    assert checked >= 15 and {2, 3, 4, 6} <= ops, (checked, ops)


def _launches(rx):
    return {k: v["launches"] for k, v in rx.kernel_times().items()}


def _mix_launches(kt):
    return sum(kt.get(k, 0) for k in ("k_mix_levels", "k_mix_decimate(level0)", "k_mix_decimate(sub)"))


def test_submit_device_behind_queued_device_frames_with_the_tail_in_levels():
    """3 x process_device (their demodulation rides in k_levels_tail), then submit_device with no fetch or sync in between: the
    submit drains the software pipeline -- the last frame's demodulation included -- before its own launches, and the frame it
    delivers equals the oracle's.  The launch counts show the fused form was in use: against tail_in_levels = 0, three
    k_usb_demod launches fewer and one k_mix_levels launch more (the drain of the extra stage)."""
    from sdrreceiver_amd.receiver import Receiver
    topo = golden_topology("profile_25e")
    frames = _lcg_frames(topo, 5, seed=77)
    dev = _to_device(frames)
    o = Oracle(topo)
    want = [o.feed(iq) for iq in frames]
    kts = {}
    for tail in (True, False):
        rx = Receiver.from_topology(topo, exact=True, tail_in_levels=tail)
        rx.enable_kernel_timing(True)
        for f in range(3):
            rx.process_device(dev[f].data_ptr(), topo.frame)
        rx.submit_device(dev[3].data_ptr(), topo.frame)
        assert rx.in_flight() == 1
        rx.wait()
        assert rx.published == want[3], tail
        rx.process_device(dev[4].data_ptr(), topo.frame)  # and back onto the device queue
        rx.fetch()
        assert rx.published == want[4], tail
        kts[tail] = _launches(rx)
        assert rx.stats()["n_levels"] == 2
        rx.close()
    assert kts[True].get("k_usb_demod", 0) == kts[False].get("k_usb_demod", 0) - 4, kts
    assert _mix_launches(kts[True]) == _mix_launches(kts[False]) + 2, kts


@pytest.mark.parametrize("pipeline", [False, True])
def test_dc_frames_and_device_frames_in_flight_together(pipeline):
    """A submit_u8(correct_dc=1) frame owes its payload copy to sdrx_wait, a submit_device frame has it queued at once: both
    orders with two frames in flight, an sdrx_sync between submit and wait, then a steady alternation.  Every frame delivers in
    order with its own payloads; the DC-bias state is carried by the correct_dc frames only."""
    from sdrreceiver_amd.receiver import Receiver
    topo = tp.config2()
    rx = Receiver.from_topology(topo, pipeline=pipeline)
    o = Oracle(topo)
    rng = np.random.default_rng(23)
    kinds = ["dc", "dev", "dev", "dc", "dc", "dev", "dc", "dev", "dc"]
    data, want, dev = [], [], {}
    for f, k in enumerate(kinds):
        b = rng.integers(0, 256, 2 * topo.frame, dtype=np.uint8)
        b[0::2] = np.clip(b[0::2].astype(int) // 8 + 100, 0, 255)
        if k == "dc":
            data.append(b)
            want.append(o.feed_u8(b, True))
        else:
            iq = ob.u8_to_float(b)
            data.append(iq)
            want.append(o.feed(iq))
            dev[f] = _to_device([iq])[0]

    def submit(f):
        if kinds[f] == "dc":
            rx.submit_u8(data[f], correct_dc=True)
        else:
            rx.submit_device(dev[f].data_ptr(), topo.frame)

    def wait(f):
        rx.wait()
        assert rx.published == want[f], (pipeline, f, kinds[f])

    submit(0)
    submit(1)  # dc, then device
    rx.sync()  # everything queued has run; frame 0's copy is still owed
    wait(0)
    wait(1)
    submit(2)
    submit(3)  # device, then dc
    wait(2)
    rx.sync()
    wait(3)
    submit(4)
    for f in range(5, len(kinds)):
        submit(f)
        assert rx.in_flight() == 2
        wait(f - 1)
    wait(len(kinds) - 1)
    assert rx.in_flight() == 0
    rx.close()


# ------------------------------------------------------------------------------------------------------- 3. stream ordering
@functools.lru_cache(maxsize=None)
def _sleep_cycles(ms):
    """torch.cuda._sleep cycles that last about `ms` milliseconds on this device (its counter's rate, measured here)"""
    import torch
    cal = 20_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(cal)
    b.record()
    b.synchronize()
    return max(1, int(cal * ms / max(a.elapsed_time(b), 1e-3)))


class LateProducer:
    """Device buffers that hold a decoy frame until a producer stream, after a sleep, copies the true frame in."""

    def __init__(self, topo, n_buffers=2):
        import torch
        self.topo = topo
        self.stream = torch.cuda.Stream()
        self.cycles = _sleep_cycles(PRODUCER_SLEEP_MS)
        self.bufs = [torch.empty(2 * topo.frame, dtype=torch.float32, device="cuda") for _ in range(n_buffers)]

    def write(self, k, true_dev, decoy_dev):
        """buffer k: the decoy now (complete), the true frame once the producer's sleep has ended; returns its pointer"""
        import torch
        buf = self.bufs[k]
        buf.copy_(decoy_dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(self.cycles)
            buf.copy_(true_dev)
        return buf.data_ptr()

    def still_running(self):
        return not self.stream.query()


def _true_and_decoy(topo, n):
    frames = _lcg_frames(topo, n, seed=61)
    decoys = [iq[::-1].copy() * 3.0 for iq in _lcg_frames(topo, n, seed=62)]
    for a, b in zip(frames, decoys):
        assert not np.array_equal(a, b)
    return frames, _to_device(frames), _to_device(decoys)


@pytest.mark.parametrize("members", [2, 3])
def test_group_waits_for_the_producer_stream(members):
    """sdrx_group_submit_device and sdrx_group_process_device with the frame still being written on `producer_stream`: member
    0 reads the caller's buffer directly, the others copy it -- all of them only after the producer's copy, so every payload is
    the true frame's, never the decoy's."""
    from sdrreceiver_amd.receiver import Group
    topo = golden_topology("profile_25e")
    n = 6
    frames, true_dev, decoy_dev = _true_and_decoy(topo, n)
    o = Oracle(topo)
    want = [o.feed(iq) for iq in frames]
    g = Group.from_topology(topo, [0] * members)
    p = LateProducer(topo)
    s = p.stream.cuda_stream
    g.submit_device(p.write(0, true_dev[0], decoy_dev[0]), topo.frame, producer_stream=s)
    assert p.still_running(), "the producer finished before the frame was handed over: the sleep is too short to test anything"
    for f in range(1, 4):
        g.submit_device(p.write(f % 2, true_dev[f], decoy_dev[f]), topo.frame, producer_stream=s)
        assert p.still_running()
        g.wait()
        assert g.published == want[f - 1], (members, f - 1)
    g.wait()
    assert g.published == want[3], members
    for f in (4, 5):
        g.process_device(p.write(f % 2, true_dev[f], decoy_dev[f]), topo.frame, producer_stream=s)
        assert p.still_running()
    g.sync()
    for i in topo.leaves_in_publish_order():
        assert np.array_equal(g.output(i), o.nodes[i].usb() if topo.vfos[i].demod_usb else o.nodes[i].iq()), (members, i)
    g.close()


@pytest.mark.parametrize("pipeline", [False, True])
def test_context_on_the_producer_stream(pipeline):
    """sdrx_set_stream(the producer's stream), then sdrx_submit_device / sdrx_process_device while the frame is still being
    written on it: the frame is consumed in that stream's order (with option pipeline the tail runs on the library's own
    stream behind it), so every payload is the true frame's."""
    from sdrreceiver_amd.receiver import Receiver
    topo = golden_topology("profile_25e")
    n = 7
    frames, true_dev, decoy_dev = _true_and_decoy(topo, n)
    o = Oracle(topo)
    want = [o.feed(iq) for iq in frames]
    rx = Receiver.from_topology(topo, exact=True, pipeline=pipeline)
    p = LateProducer(topo)
    rx.set_stream(p.stream.cuda_stream)
    rx.submit_device(p.write(0, true_dev[0], decoy_dev[0]), topo.frame)
    assert p.still_running(), "the producer finished before the frame was handed over: the sleep is too short to test anything"
    for f in range(1, 4):
        rx.submit_device(p.write(f % 2, true_dev[f], decoy_dev[f]), topo.frame)
        assert p.still_running()
        rx.wait()
        assert rx.published == want[f - 1], (pipeline, f - 1)
    rx.wait()
    assert rx.published == want[3], pipeline
    for f in (4, 5):
        rx.process_device(p.write(f % 2, true_dev[f], decoy_dev[f]), topo.frame)
        assert p.still_running()
    rx.fetch()
    assert rx.published == want[5], pipeline
    rx.process_device(p.write(0, true_dev[6], decoy_dev[6]), topo.frame)
    rx.sync()
    assert rx.output(_publishers(topo)[0]).tobytes() == want[6][0][2], pipeline
    rx.set_stream(None)
    rx.close()


# ------------------------------------------------------------------------------------------------------------- 4. lifetime
def _outputs(rx, topo):
    return [rx.output(i).tobytes() for i in _publishers(topo)]


def test_caller_buffer_is_free_after_delivery():
    """Once sdrx_wait (submit_device) or sdrx_sync / sdrx_fetch (process_device) has returned, the caller may overwrite its
    buffer: the delivered payloads stay what they were, and the following frames still equal the oracle's."""
    import torch
    from sdrreceiver_amd.receiver import Receiver
    topo = golden_topology("profile_25e")
    frames = _lcg_frames(topo, 11, seed=88)
    dev = _to_device(frames)
    decoy = _to_device([frames[0][::-1].copy() * 5.0])[0]
    o = Oracle(topo)
    want = [o.feed(iq) for iq in frames]
    msgs = lambda w: [p for _, _, p in w]  # noqa: E731
    rx = Receiver.from_topology(topo, exact=True)

    def clobber(*ks):
        for k in ks:
            dev[k].copy_(decoy)
        torch.cuda.synchronize()

    rx.submit_device(dev[0].data_ptr(), topo.frame)
    for f in range(1, 5):
        rx.submit_device(dev[f].data_ptr(), topo.frame)
        rx.wait()
        assert rx.published == want[f - 1], f - 1
        clobber(f - 1)
        assert _outputs(rx, topo) == msgs(want[f - 1]), ("after overwriting", f - 1)
    rx.wait()
    clobber(4)
    assert _outputs(rx, topo) == msgs(want[4])
    for f in (5, 6, 7):  # the device queue: sync, overwrite, then the payloads are fetched
        rx.process_device(dev[f].data_ptr(), topo.frame)
    rx.sync()
    clobber(5, 6, 7)
    assert _outputs(rx, topo) == msgs(want[7])
    for f in (8, 9):  # fetch, overwrite
        rx.process_device(dev[f].data_ptr(), topo.frame)
    rx.fetch()
    assert rx.published == want[9]
    clobber(8, 9)
    assert _outputs(rx, topo) == msgs(want[9])
    rx.submit_device(dev[10].data_ptr(), topo.frame)
    rx.wait()
    assert rx.published == want[10]
    rx.close()


def _member_raw(g, k, n):
    ctx, _ = g.member_context(k)
    out = np.zeros(2 * n, np.float32)
    got = C.c_int()
    rc = g.L.sdrx_get_raw(ctx, out.ctypes.data, n, C.byref(got))
    return rc, out[: 2 * got.value]


def test_get_raw_refuses_caller_owned_frames():
    """sdrx_get_raw after a device frame is SDRX_ESTATE (caller-owned device memory), on a context and on every member of a
    group; after a later host frame it serves that frame again (the DC-corrected one on the group's members)."""
    from sdrreceiver_amd.receiver import Group, Receiver
    topo = tp.config2()
    frames = _lcg_frames(topo, 4, seed=90)
    dev = _to_device(frames)
    o = Oracle(topo)
    rx = Receiver.from_topology(topo, exact=True)
    rx.submit_device(dev[0].data_ptr(), topo.frame)
    rx.wait()
    assert _code(rx.raw) == _lib.SDRX_ESTATE
    rx.process(frames[1])
    assert np.array_equal(bits(rx.raw()), bits(np.ascontiguousarray(frames[1], np.float32).view(np.complex64)))
    rx.submit_device(dev[2].data_ptr(), topo.frame)
    rx.wait()
    assert _code(rx.raw) == _lib.SDRX_ESTATE
    rx.process_u8((frames[3] + 127).astype(np.uint8))
    assert np.array_equal(bits(rx.raw()), bits(np.ascontiguousarray(frames[3], np.float32).view(np.complex64)))
    rx.close()

    g = Group.from_topology(topo, [0, 0])
    g.submit_device(dev[0].data_ptr(), topo.frame)
    g.wait()
    assert g.published == o.feed(frames[0])
    for k in (0, 1):
        assert _member_raw(g, k, topo.frame)[0] == _lib.SDRX_ESTATE, k
    b = (frames[1] * 4 + 131).astype(np.uint8)
    g.process_u8(b, correct_dc=True)
    assert g.published == o.feed_u8(b, True)
    iq = ob.u8_to_float(b)
    ob.dc_correct(iq, np.zeros(2, np.float32))
    for k in (0, 1):
        rc, raw = _member_raw(g, k, topo.frame)
        assert rc == 0 and np.array_equal(bits(raw), bits(iq)), k
    g.process_device(dev[2].data_ptr(), topo.frame)
    g.sync()
    o.feed(frames[2])
    for k in (0, 1):
        assert _member_raw(g, k, topo.frame)[0] == _lib.SDRX_ESTATE, k
    for i in topo.leaves_in_publish_order():
        assert np.array_equal(g.output(i), o.nodes[i].usb()), i
    g.close()


# ------------------------------------------------------------------------------------------- 5. what travels with the frame
def test_meters_and_spectra_travel_with_device_frames():
    """meter = 1 and spectra on a tapped leaf (a /5 late decimation fused into the mix wave), a main and the raw frame (every
    4th frame): the same frames through sdrx_submit and sdrx_submit_device, two in flight, give the same payloads, meter
    records (frame index included) and spectra bit for bit; the payloads equal the oracle's and the raw spectrum is
    fftHandlerSlot's of the frames handed over."""
    from sdrreceiver_amd.receiver import SPECTRUM_RAW, Receiver
    topo = golden_topology("54w")
    leaf, main = len(topo.vfos) - 1, 0
    assert topo.vfos[leaf].late_decimate == 5 and topo.children(main)
    n = 10
    frames = [iq + synth.tone_frame(topo.frame, topo.fs, [(topo.fs / 5.7, 30.0)], f * topo.frame)
              for f, iq in enumerate(_lcg_frames(topo, n, seed=95))]
    dev = _to_device(frames)
    o = Oracle(topo)
    want = [o.feed(iq) for iq in frames]
    leaves = [i for i in range(len(topo.vfos)) if not topo.children(i)]
    rxs = {}
    for kind in ("host", "device"):
        rx = Receiver.from_topology(topo, exact=True, meter=True)
        rx.set_tap(leaf)
        for v in (leaf, main, SPECTRUM_RAW):
            rx.set_spectrum(v)
        rxs[kind] = rx
    submit = {"host": lambda f: rxs["host"].submit(frames[f]),
              "device": lambda f: rxs["device"].submit_device(dev[f].data_ptr(), topo.frame)}
    raw_disp = sr.Display()
    raw_calls = sr.raw_update_calls(n)

    def deliver(f):
        got = {}
        for kind, rx in rxs.items():
            rx.wait()
            assert rx.published == want[f], (kind, f)
            got[kind] = rx.meters(leaves)
        for key in got["host"]:
            assert np.asarray(got["host"][key]).tobytes() == np.asarray(got["device"][key]).tobytes(), (f, key)
        assert (got["device"]["frame"] == f).all(), f
        if f + 1 in raw_calls:
            raw_disp.update(np.ascontiguousarray(frames[f], np.float32).view(np.complex64))

    def spectra(f):
        for v in (leaf, main, SPECTRUM_RAW):
            a, b = rxs["host"].spectrum(v), rxs["device"].spectrum(v)
            assert a["updates"] == b["updates"] and np.array_equal(bits(a["bins"]), bits(b["bins"])), (f, v)
            assert np.array_equal(bits(a["pwr"]), bits(b["pwr"])), (f, v)
        d = rxs["device"].spectrum(SPECTRUM_RAW)
        assert d["updates"] == raw_disp.updates and np.array_equal(bits(d["bins"]), bits(raw_disp.bins)), f
        if raw_disp.updates:
            assert np.abs(d["pwr"] - raw_disp.pwr).max() <= 1e-9, f

    for f in range(0, n, 2):  # two in flight, then both delivered: the spectra are read with nothing in flight
        for kind in rxs:
            submit[kind](f)
            submit[kind](f + 1)
        deliver(f)
        deliver(f + 1)
        spectra(f + 1)
    assert raw_disp.updates == 2
    for rx in rxs.values():
        rx.close()


# -------------------------------------------------------------------------------------- 6. refusals leave the state alone
def test_refused_device_frames_queue_nothing():
    """submit_device with two frames in flight (SDRX_ESTATE), a wrong n_complex or a null pointer (SDRX_EINVAL), and fetch,
    get_stream, get_raw or process_device while device frames are in flight (SDRX_ESTATE): each queues nothing, and the
    frames before and after still equal the oracle's."""
    from sdrreceiver_amd.receiver import Receiver
    topo = golden_topology("profile_25e")
    frames = _lcg_frames(topo, 6, seed=99)
    dev = _to_device(frames)
    o = Oracle(topo)
    want = [o.feed(iq) for iq in frames]
    rx = Receiver.from_topology(topo, exact=True)
    ptr = dev[0].data_ptr()

    def refused(call, code, in_flight):
        frames_before = rx.stats()["frames"]
        assert _code(call) == code
        assert rx.in_flight() == in_flight and rx.stats()["frames"] == frames_before

    refused(lambda: rx.submit_device(ptr, topo.frame - 16), _lib.SDRX_EINVAL, 0)
    refused(lambda: rx.submit_device(0, topo.frame), _lib.SDRX_EINVAL, 0)
    rx.submit_device(dev[0].data_ptr(), topo.frame)
    refused(lambda: rx.submit_device(ptr, topo.frame + 16), _lib.SDRX_EINVAL, 1)
    rx.submit_device(dev[1].data_ptr(), topo.frame)
    for call, code in ((lambda: rx.submit_device(dev[2].data_ptr(), topo.frame), _lib.SDRX_ESTATE),
                       (lambda: rx.submit_device(0, topo.frame), _lib.SDRX_EINVAL),
                       (lambda: rx.submit_device(ptr, 1), _lib.SDRX_EINVAL),
                       (rx.fetch, _lib.SDRX_ESTATE), (lambda: rx.stream(0), _lib.SDRX_ESTATE), (rx.raw, _lib.SDRX_ESTATE),
                       (lambda: rx.process_device(ptr, topo.frame), _lib.SDRX_ESTATE)):
        refused(call, code, 2)
    rx.wait()
    assert rx.published == want[0]
    rx.submit_device(dev[2].data_ptr(), topo.frame)
    rx.wait()
    assert rx.published == want[1]
    rx.wait()
    assert rx.published == want[2]
    for f in (3, 4):
        rx.process_device(dev[f].data_ptr(), topo.frame)
    rx.fetch()
    assert rx.published == want[4]
    rx.submit_device(dev[5].data_ptr(), topo.frame)
    rx.wait()
    assert rx.published == want[5]
    rx.close()


def test_refused_group_device_frames_queue_nothing():
    """The same refusals on a group: nothing queued on any member, the group not marked broken, every later frame the
    oracle's."""
    from sdrreceiver_amd.receiver import Group
    topo = golden_topology("profile_25e")
    frames = _lcg_frames(topo, 5, seed=98)
    dev = _to_device(frames)
    o = Oracle(topo)
    want = [o.feed(iq) for iq in frames]
    g = Group.from_topology(topo, [0, 0, 0])
    ptr = dev[0].data_ptr()

    def member_frames():
        return [s["frames"] for s in g.member_stats() if s]

    def refused(call, code, in_flight):
        before = member_frames()
        assert _code(call) == code
        assert g.in_flight() == in_flight and member_frames() == before

    refused(lambda: g.submit_device(ptr, topo.frame - 16), _lib.SDRX_EINVAL, 0)
    refused(lambda: g.submit_device(0, topo.frame), _lib.SDRX_EINVAL, 0)
    refused(lambda: g.process_device(0, topo.frame), _lib.SDRX_EINVAL, 0)
    g.submit_device(dev[0].data_ptr(), topo.frame)
    g.submit_device(dev[1].data_ptr(), topo.frame)
    for call, code in ((lambda: g.submit_device(dev[2].data_ptr(), topo.frame), _lib.SDRX_ESTATE),
                       (lambda: g.submit_device(0, topo.frame), _lib.SDRX_EINVAL),
                       (lambda: g.submit_device(ptr, 1), _lib.SDRX_EINVAL),
                       (lambda: g.process_device(ptr, topo.frame), _lib.SDRX_ESTATE),
                       (lambda: g.stream(_publishers(topo)[0]), _lib.SDRX_ESTATE)):
        refused(call, code, 2)
    for k in range(3):
        assert _member_raw(g, k, topo.frame)[0] == _lib.SDRX_ESTATE, k
    g.wait()
    assert g.published == want[0]
    g.submit_device(dev[2].data_ptr(), topo.frame)
    g.wait()
    assert g.published == want[1]
    g.wait()
    assert g.published == want[2]
    g.process_device(dev[3].data_ptr(), topo.frame)
    g.sync()
    g.submit_device(dev[4].data_ptr(), topo.frame)
    g.wait()
    assert g.published == want[4]
    g.close()
