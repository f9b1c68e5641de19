"""Parking and unparking leaves on a running tree (option "park", sdrx_set_active and its group form).

A parked leaf does nothing and is delivered as a closed one; a leaf unparked before frame K is, from K on, the reference's
`new vfo` with the descriptor as it stands: a fresh retune_ref.Node (pinned to the oracle by test_park_model.py) fed the oracle
parent's decimate[d] from K on.  Leaves that are never parked equal the oracle tree that ran every frame."""
import dataclasses
import functools

import numpy as np
import pytest

import retune_ref as rr
from oracle import binding as ob
from sdrreceiver_amd import _lib, squelch as sq, synth
from sdrreceiver_amd.receiver import SdrxError
from sdrreceiver_amd.topology import Topology, VfoDesc
from helpers import tree_1536
from test_park_model import NONE, gate_with_parking

pytestmark = pytest.mark.gpu

N_FRAMES = 8


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def tree_1920() -> Topology:
    """sdr_54W: one main to 240 k, three /5 leaves (48 k, two with the 10 kHz low-pass)."""
    t = Topology(fs=1920000, frame=480000, bufsplit=4, center_frequency=1545939000, name="park-1920")
    t.vfos.append(VfoDesc(parent=-1, fs=1920000, decimate_count=3, mixer_freq=819000.0, demod_usb=False, cstyle=1,
                          samples_per_buffer=480000))
    c = dict(parent=0, fs=240000, decimate_count=0, late_decimate=5, gain=float(np.float32(0.04)), cstyle=1,
             samples_per_buffer=60000)
    t.vfos.append(VfoDesc(topic="VFO41", mixer_freq=12000.0, filter_bw=10000, **c))
    t.vfos.append(VfoDesc(topic="VFO42", mixer_freq=-30000.0, **c))
    t.vfos.append(VfoDesc(topic="VFO43", mixer_freq=50000.0, filter_bw=10000, **c))
    return t


TREES = {"1536": tree_1536, "1920": tree_1920}
# frame -> the calls before it, in order: ("park" | "unpark", ids), ("freq" | "gain", id, value).
# 1536: A = 4 (d = 2, the 10 kHz low-pass; fuse_demod's shape), B = 2 (d = 5), C = 6 (the 463-tap low-pass: k_lpf_long), D = 3;
#       5 is never parked.  1920: A = 1, B = 2 (and restarted before frame 6: D), C = 3 -- every leaf of that tree is parked once.
SCHED = {
    "1536": {2: [("park", [4])], 3: [("park", [2, 6]), ("freq", 4, -40000.0), ("gain", 4, float(np.float32(0.05)))],
             4: [("unpark", [2]), ("park", [3]), ("unpark", [3])], 5: [("unpark", [4, 6])]},
    "1920": {2: [("park", [1])], 3: [("park", [2, 3]), ("freq", 1, 15000.0), ("gain", 1, float(np.float32(0.03)))],
             4: [("unpark", [2])], 5: [("unpark", [1, 3])], 6: [("park", [2]), ("unpark", [2])]},
}


def _leaves(topo):
    return [i for i in range(len(topo.vfos)) if not topo.children(i)]


@functools.lru_cache(maxsize=None)
def _frames(key, n=N_FRAMES, seed=11):
    lcg = synth.Lcg(seed)
    return [synth.lcg_frame(TREES[key]().frame, lcg) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def reference(key):
    """want[f][leaf] = (stream, payload), or None for a frame the leaf is parked in; and the descriptors after the schedule.
    Computed once per tree and shared (nobody writes into it)."""
    topo = TREES[key]()
    sched = SCHED[key]
    nodes, roots = ob.build_tree("port", topo)
    descs = {i: topo.vfos[i] for i in _leaves(topo)}
    fresh = {}    # leaf -> the model node it is since its last unpark
    parked = set()
    want = []
    for f, iq in enumerate(_frames(key)):
        for op in sched.get(f, []):
            if op[0] == "park":
                parked |= set(op[1])
            elif op[0] == "unpark":
                for i in op[1]:
                    if i in parked:
                        parked.discard(i)
                        fresh[i] = rr.Node(descs[i])
            elif op[0] == "freq":
                descs[op[1]] = dataclasses.replace(descs[op[1]], mixer_freq=op[2])
                assert op[1] in parked  # (the schedules retune parked leaves only: the model node is built afterwards)
            else:
                descs[op[1]] = dataclasses.replace(descs[op[1]], gain=op[2])
                assert op[1] in parked
        ob.process_roots(roots, iq)
        w = {}
        for i in _leaves(topo):
            if i in parked:
                w[i] = None
            elif i in fresh:
                z = fresh[i].process(nodes[topo.vfos[i].parent].stream().view(np.complex64))
                w[i] = (z, fresh[i].payload())
            else:
                v = nodes[i]
                w[i] = (v.stream().view(np.complex64), v.usb() if topo.vfos[i].demod_usb else v.iq())
        want.append(w)
    return want, descs


class Drive:
    """Feeds frames to a Receiver in one of three ways.  "process": sdrx_process; "submit": sdrx_submit with a frame in flight
    wherever no change follows; "device": sdrx_process_device under the frame pipeline, the two frames before a change left
    inside the pipeline (the change drains them)."""

    def __init__(self, rx, topo, frames, mode, changes_at):
        self.rx, self.topo, self.frames, self.mode, self.changes_at = rx, topo, frames, mode, set(changes_at)
        if mode == "device":
            import torch
            self.dev = [torch.from_numpy(iq).cuda() for iq in frames]
            torch.cuda.synchronize()

    def run(self, apply, check):
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


def _apply_ops(rx, ops):
    for op in ops:
        if op[0] == "park":
            rx.set_active(op[1], [0] * len(op[1]))
        elif op[0] == "unpark":
            rx.set_active(op[1], [1] * len(op[1]))
        elif op[0] == "freq":
            rx.set_mixer_freqs([op[1]], [op[2]])
        else:
            rx.set_gains([op[1]], [op[2]])


def _run(key, mode, exact=True, rx=None, **opts):
    from sdrreceiver_amd.receiver import Receiver
    topo = TREES[key]()
    sched = SCHED[key]
    want, descs = reference(key)
    meter = bool(opts.get("meter"))
    if rx is None:
        rx = Receiver.from_topology(topo, exact=exact, keep_streams=True, park=True, **opts)
    applied, seen = set(), []

    def apply(f):
        if f in sched and f not in applied:
            _apply_ops(rx, sched[f])
            applied.add(f)

    def check(f):
        topics = [t for t, _, _ in rx.published]
        for i, w in want[f].items():
            got_pay = rx.output(i)
            name = topo.vfos[i].topic.encode().ljust(5, b"\0")[:5]
            if w is None:  # the delivery rules of a parked leaf
                assert got_pay.size == 0, (key, mode, opts, f, i, "a parked leaf has a payload")
                assert name not in topics, (key, mode, opts, f, i, "a parked leaf was published")
                if rx.in_flight() == 0:
                    assert rx.stream(i, missing_ok=True) is None, (key, mode, opts, f, i, "a parked leaf has a stream")
                if meter:
                    m = rx.meters([i])
                    assert (int(m["frame"][0]), int(m["n_values"][0]), int(m["sum_sq"][0]), int(m["clipped"][0]),
                            float(m["peak"][0])) == (f, 0, 0, 0, 0.0), (key, mode, f, i, m)
                continue
            z, pay = w
            assert name in topics, (key, mode, opts, f, i, "an active leaf was not published")
            got_z = rx.stream(i) if rx.in_flight() == 0 else None  # (device read-backs wait for the frames in flight)
            if exact is True:
                assert np.array_equal(_bits(got_pay), _bits(pay)), (key, mode, opts, f, i, "payload")
                assert got_z is None or np.array_equal(_bits(got_z), _bits(z)), (key, mode, opts, f, i, "stream")
            else:
                tol = 1e-5 * float(np.abs(z).max())
                assert got_z is not None and float(np.abs(got_z - z).max()) <= tol, (key, mode, exact, f, i, "stream")
                assert int(np.abs(got_pay.astype(np.int32) - pay.astype(np.int32)).max()) <= 1, (key, mode, exact, f, i)
            if meter and exact is True:
                assert int(rx.meters([i])["sum_sq"][0]) == int((pay.astype(np.int64) ** 2).sum()), (key, mode, f, i, "meter")
        # the order of the other leaves' callbacks is the publish order of the active ones
        order = [topo.vfos[i].topic.encode().ljust(5, b"\0")[:5] for i in _publish_order(topo) if want[f][i] is not None]
        assert topics == order, (key, mode, opts, f, topics, order)
        seen.append(f)

    Drive(rx, topo, _frames(key), mode, sched.keys()).run(apply, check)
    assert set(range(2, N_FRAMES)) <= set(seen), seen  # every frame from the first change on ("device" leaves 0 and 1 queued)
    a = 4 if key == "1536" else 1  # leaf A: retuned while parked -- the new oscillator's table
    L = topo.vfos[a].fs
    tab = rr.table(L, descs[a].mixer_freq)
    assert np.array_equal(_bits(rx.nco(a, L - 64, 64)), _bits(tab[L - 64:]))
    st = rx.active(_leaves(topo))
    assert list(st["active"]) == [1] * len(_leaves(topo))
    assert int(st["since_frame"][_leaves(topo).index(a)]) == 5
    rx.close()


def _publish_order(topo):
    out = []
    for m in range(len(topo.vfos)):
        if topo.vfos[m].parent < 0:
            kids = topo.children(m)
            out += kids if kids else [m]
    return out


CASES_EXACT = [
    ("1536", "process", dict()),
    ("1536", "process", dict(meter=True)),
    ("1536", "submit", dict(fuse_demod=True, tail_in_levels=False)),
    ("1536", "device", dict(fuse_demod=True, tail_in_levels=True)),
    ("1536", "device", dict(fuse_demod=False, tail_in_levels=True)),
    ("1536", "device", dict(fuse_demod=False, tail_in_levels=False)),
    ("1536", "submit", dict(pipeline=True)),
    ("1536", "device", dict(fuse_demod=True, tail_in_levels=False, meter=True)),
    ("1920", "process", dict(fuse_late=True)),
    ("1920", "submit", dict(fuse_late=False)),
    ("1920", "device", dict(fuse_late=True)),
    ("1920", "device", dict(fuse_late=False)),
]


@pytest.mark.parametrize("key,mode,opts", CASES_EXACT, ids=[f"{k}-{m}-{'-'.join(f'{a}{int(b)}' for a, b in o.items())}"
                                                            for k, m, o in CASES_EXACT])
def test_park_unpark_exact(key, mode, opts):
    """Every launch form: the 1.536 MS/s tree carries the d = 5 and d = 2 leaves, fuse_demod's leaves and the leaf with the
    463-tap low-pass (k_lpf_long) in every case; the 1.92 MS/s tree the late decimation, fused and in its own kernel."""
    _run(key, mode, **opts)


@pytest.mark.parametrize("exact", [False, 2])
def test_park_tolerance_arithmetics(exact):
    """exact = 0 and exact = 2: within 1e-5 of max|stream| and 1 LSB of the same references."""
    _run("1536", "process", exact=exact)


def _collect(rx, topo, frames, meter):
    out = []
    for iq in frames:
        rx.process(iq)
        rec = dict(pub=list(rx.published), pay=[rx.output(i) for i in _leaves(topo)],
                   z=[rx.stream(i) for i in range(len(topo.vfos))])
        if meter:
            m = rx.meters(_leaves(topo))
            rec["meter"] = [m[k].tolist() for k in ("frame", "n_values", "sum_sq", "clipped", "peak")]
        out.append(rec)
    return out


@pytest.mark.parametrize("opts", [dict(meter=True), dict(fuse_demod=True, squelch=True, preroll=True)], ids=["meter", "gate"])
def test_nothing_parked_equals_option_off(opts):
    from sdrreceiver_amd.receiver import Receiver
    topo = tree_1536()
    frames = _frames("1536")[:4]
    res, dev_bytes = {}, {}
    for park in (False, True):
        rx = Receiver.from_topology(topo, keep_streams=True, park=park, **opts)
        res[park] = _collect(rx, topo, frames, True)
        dev_bytes[park] = rx.stats()["device_bytes"]
        if not park:
            with pytest.raises(SdrxError) as e:
                rx.set_active([2], [0])
            assert e.value.code == _lib.SDRX_ESTATE
            plain = Receiver.from_topology(topo, keep_streams=True, **opts)  # the figure of a context that was never asked
            plain.process(frames[0])
            assert plain.stats()["device_bytes"] == dev_bytes[False]
            plain.close()
        rx.close()
    for f, (a, b) in enumerate(zip(res[False], res[True])):
        assert a["pub"] == b["pub"], f
        assert a["meter"] == b["meter"], f
        for x, y in zip(a["pay"] + a["z"], b["pay"] + b["z"]):
            assert np.array_equal(_bits(x), _bits(y)), f
    assert dev_bytes[True] >= dev_bytes[False]


def test_park_with_squelch_preroll_auto():
    """Directory, open, pre, hang_left, floor state, n_open and egress bytes against the Python model, with thresholds read off
    the reference payloads' own sum_sq so that: leaf 4 is parked while its hang time runs; leaf 2 is unparked into a frame that
    would have pre-rolled; leaf 6 is auto-squelched and parked (its floor must not become 0); leaf 3 has threshold 0 and is
    parked (still closed)."""
    from sdrreceiver_amd.receiver import Receiver
    topo = tree_1536()
    want, _ = reference("1536")
    frames = _frames("1536")
    leaves = _leaves(topo)
    events = {4: {2: "p", 5: "u"}, 2: {3: "p", 4: "u"}, 6: {3: "p", 5: "u"}, 3: {4: "pu"}, 5: {}}
    s = {i: [0 if want[f][i] is None else int((want[f][i][1].astype(np.int64) ** 2).sum()) for f in range(N_FRAMES)] for i in leaves}
    # leaf 4: opens in frame 0 only (thr = its sum_sq there, more than frame 1's or just hang): hang 5 keeps it open, parked in 2
    thr = {4: max(s[4][0], s[4][1]), 2: 0, 6: 0, 3: 0, 5: 0}
    hang = {4: 5, 2: 0, 6: 0, 3: 0, 5: 1}
    # leaf 2: closed in frame 2 (a threshold no frame reaches, set before it), open again in 4 where it is unparked (threshold 1
    # from there on): without the parking frame 4 would pre-roll
    big = 1 << 62
    thr[2] = [0, 0, big, big, 1, 1, 1, 1]
    # leaf 5 (never parked): closed in some frames, open in others
    thr[5] = sorted(s[5])[N_FRAMES // 2]
    ratio = {i: 0 for i in leaves}
    window = {i: 0 for i in leaves}
    ratio[6], window[6] = 128, 2  # half the floor: open whenever it has one
    rx = Receiver.from_topology(topo, keep_streams=True, park=True, squelch=True, preroll=True, squelch_auto=True)
    rx.set_squelch(leaves, [thr[i][0] if i == 2 else thr[i] for i in leaves], [hang[i] for i in leaves])
    rx.set_squelch_auto(leaves, [ratio[i] for i in leaves], [window[i] for i in leaves])
    model = {i: gate_with_parking(s[i], events[i], thr[i], hang[i], ratio[i], window[i]) for i in leaves}
    assert model[4][2]["hang_left"] > 0 and not model[4][2]["active"], "leaf 4 is parked while its hang time runs"
    assert model[2][4]["open"] and not model[2][2]["open"] and not model[2][4]["pre"], "leaf 2: unparked where it would pre-roll"
    assert model[6][3]["floor"] not in (0, NONE) and not model[6][3]["active"], "leaf 6: a parked frame with a floor"
    units = {i: sq.align64(2 * topo.vfos[i].samples_per_buffer // 2 ** topo.vfos[i].decimate_count) for i in leaves}
    sched = SCHED["1536"]
    for f, iq in enumerate(frames):
        _apply_ops(rx, sched.get(f, []))
        if f and thr[2][f] != thr[2][f - 1]:
            rx.set_squelch([2], [thr[2][f]], [0])
        rx.process(iq)
        st, au, eg = rx.squelch(leaves), rx.squelch_auto(leaves), rx.egress()
        n_open = bytes_ = 0
        for k, i in enumerate(leaves):
            m = model[i][f]
            assert int(st["open"][k]) == m["open"], (f, i, "open")
            assert int(st["hang_left"][k]) == m["hang_left"], (f, i, "hang_left")
            assert int(au["thr_eff_sum_sq"][k]) == m["thr_eff"], (f, i, "thr_eff")
            assert int(au["floor_valid"][k]) == int(m["floor"] != NONE), (f, i, "floor_valid")
            assert int(au["floor_sum_sq"][k]) == (0 if m["floor"] == NONE else m["floor"]), (f, i, "floor")
            assert rx.preroll(i).size == (want[f - 1][i][1].size if m["pre"] else 0), (f, i, "pre")
            pay = rx.output(i)
            if m["open"]:
                assert np.array_equal(pay, want[f][i][1]), (f, i, "payload")
                if m["pre"]:
                    assert np.array_equal(rx.preroll(i), want[f - 1][i][1]), (f, i, "pre-rolled payload")
            else:
                assert pay.size == 0, (f, i)
            n_open += m["open"]
            bytes_ += units[i] * (m["open"] + m["pre"])
        assert (eg["n_open"], eg["n_leaves"], eg["payload_bytes_copied"]) == (n_open, len(leaves), bytes_), (f, eg)
    # threshold 0 on a parked leaf: parked again, it stays closed
    rx.set_active([3], [0])
    rx.process(frames[0])
    assert int(rx.squelch([3])["open"][0]) == 0 and int(rx.squelch([3])["thr_sum_sq"][0]) == 0 and rx.output(3).size == 0
    rx.close()


def test_park_spectrum_and_tap():
    """An enabled spectrum's `updates` stands still while its leaf is parked and resumes afterwards with the display state it
    had; a tap selection on a fused leaf is kept and serves the leaf's stream again after the unpark."""
    from sdrreceiver_amd.receiver import Receiver
    topo = tree_1536()
    frames = _frames("1536")
    want, _ = reference("1536")
    rx = Receiver.from_topology(topo, fuse_demod=True, park=True)  # leaf 4 demodulates in its mix wave: a stream only as a tap
    rx.set_tap(4)
    rx.set_spectrum(4, True)
    rx.set_spectrum(2, True)  # (a leaf that is never parked here, and keeps its stream: updated every frame)
    ups, pwr = [], None
    for f, iq in enumerate(frames[:7]):
        _apply_ops(rx, [op for op in SCHED["1536"].get(f, []) if op[1] == 4 or (isinstance(op[1], list) and 4 in op[1])])
        rx.process(iq)
        ups.append([int(u) for u in rx.spectrum_levels([4, 2])["updates"]])
        if f == 1:
            pwr = rx.spectrum(4)["pwr"].copy()
        if f in (2, 3, 4):
            assert np.array_equal(rx.spectrum(4)["pwr"], pwr), f  # the display state is kept
            assert rx.stream(4, missing_ok=True) is None, f
        if f in (1, 5, 6):
            assert np.array_equal(_bits(rx.stream(4)), _bits(want[f][4][0])), (f, "the tap serves the stream")
    assert [u[0] for u in ups] == [1, 2, 2, 2, 2, 3, 4], ups
    assert [u[1] for u in ups] == [1, 2, 3, 4, 5, 6, 7], ups
    assert not np.array_equal(rx.spectrum(4)["pwr"], pwr)
    rx.close()


def test_group_equals_one_context():
    """Two shards on one GPU with the same schedule: the group's payloads are the references', its parked leaves are silent,
    since_frame counts the group's frames."""
    from sdrreceiver_amd.receiver import Group
    topo = tree_1536()
    want, _ = reference("1536")
    g = Group.from_topology(topo, [0, 0], park=1)
    for f, iq in enumerate(_frames("1536")):
        _apply_ops(g, SCHED["1536"].get(f, []))
        g.process(iq)
        topics = [t for t, _, _ in g.published]
        for i, w in want[f].items():
            name = topo.vfos[i].topic.encode().ljust(5, b"\0")[:5]
            pay = g.output(i)
            if w is None:
                assert pay.size == 0 and name not in topics, (f, i)
            else:
                assert np.array_equal(_bits(pay), _bits(w[1])) and name in topics, (f, i)
    st = g.active([4, 2, 5])
    assert list(st["active"]) == [1, 1, 1] and list(st["since_frame"]) == [5, 4, 0]
    with pytest.raises(SdrxError) as e:
        g.set_active([0], [0])
    assert e.value.code == _lib.SDRX_EINVAL
    g.close()


def test_errors_change_nothing():
    """Every refused call gives its code, and the next frame is bit-identical to an undisturbed run."""
    from sdrreceiver_amd.receiver import Receiver
    topo = tree_1536()
    frames = _frames("1536")[:4]
    want, _ = reference("1536")  # (frames 0 and 1 are undisturbed in the schedule: here nothing is ever parked -> the oracle)
    nodes, roots = ob.build_tree("port", topo)
    rx = Receiver(park=True, keep_streams=True)
    for d in topo.vfos:
        rx.add_vfo(d)
    ids = np.array([2], np.int32)
    one = np.array([0], np.int32)
    assert rx.L.sdrx_set_active(rx.h, ids.ctypes.data, one.ctypes.data, 1) == _lib.SDRX_ESTATE  # before finalize
    rx.finalize()
    bad = [([99], [0]), ([2, 2], [0, 0]), ([0], [0]), ([2], [2]), ([-1], [1])]
    for f, iq in enumerate(frames):
        for vids, act in bad:
            with pytest.raises(SdrxError) as e:
                rx.set_active(vids, act)
            assert e.value.code == _lib.SDRX_EINVAL, (vids, act)
        a = np.array([2, 3], np.int32)
        assert rx.L.sdrx_set_active(rx.h, a.ctypes.data, a.ctypes.data, -1) == _lib.SDRX_EINVAL
        assert rx.L.sdrx_set_active(rx.h, None, None, 0) == 0  # n == 0 does nothing
        with pytest.raises(SdrxError):  # a good entry beside a bad one: nothing changes
            rx.set_active([3, 99], [0, 0])
        rx.submit(iq)
        with pytest.raises(SdrxError) as e:  # a frame in flight
            rx.set_active([2], [0])
        assert e.value.code == _lib.SDRX_ESTATE
        rx.wait()
        ob.process_roots(roots, iq)
        for i in _leaves(topo):
            assert np.array_equal(_bits(rx.output(i)), _bits(nodes[i].usb())), (f, i)
            assert np.array_equal(_bits(rx.stream(i)), _bits(nodes[i].stream())), (f, i)
        assert list(rx.active(_leaves(topo))["active"]) == [1] * 5
        assert list(rx.active(_leaves(topo))["since_frame"]) == [0] * 5
    rx.close()
