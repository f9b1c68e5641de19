"""Unpark with catch-up (option "catchup"): the ABI, the model of tests/catchup_ref.py against the plain-C oracle (and the real
reference where it is built), and the delivery sequence against hand-worked cases.  No GPU."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import catchup_ref as cr
import live_ref
from oracle import binding as ob
from sdrreceiver_amd import _lib, squelch as sq
from sdrreceiver_amd.topology import Topology


def test_the_abi_carries_the_new_symbols_and_keeps_its_version():
    for name in ("sdrx_get_catchup", "sdrx_group_get_catchup"):
        assert name in _lib.SYMBOLS, name
    L = _lib.lib()  # binds every symbol: AttributeError if the library lacks one
    for name in ("sdrx_get_catchup", "sdrx_group_get_catchup"):
        assert getattr(L, name).argtypes is not None
    assert L.sdrx_abi_version() == 5
    assert C.sizeof(_lib.MeterC) == 32
    import inspect
    from sdrreceiver_amd.receiver import Group, Receiver
    assert "catchup" in inspect.signature(Receiver.__init__).parameters
    assert callable(Receiver.catchup) and callable(Group.catchup)


def _unparks(key):
    """(leaf, K, caught) for every unpark of the schedule that changes a leaf's state"""
    _, _, kinds, _ = cr.reference(key)
    out = []
    for i, ev in kinds.items():
        for f, s in ev.items():
            if s[-1] in "uc":
                out.append((i, f, s[-1] == "c"))
    return out


def test_the_trees_hold_every_kind_and_every_case():
    kinds_caught, cases = set(), set()
    for key in cr.TREES:
        topo = cr.TREES[key]()
        for i, K, caught in _unparks(key):
            if caught:
                kinds_caught |= live_ref.leaf_kinds(topo, i)
            elif topo.vfos[i].parent < 0:
                cases.add("parent-less")
            else:
                cases.add("restart")
    assert kinds_caught >= set(live_ref.KINDS) - {"childless_main"}, set(live_ref.KINDS) - kinds_caught
    assert cases == {"parent-less", "restart"}
    flat = cr.flat_tree()
    assert flat.vfos[2].decimate_count == 2 and 0 < cr.lattice.lpf_taps(flat.vfos[2]) <= 64   # fuse_demod's shape
    assert cr.lattice.lpf_taps(flat.vfos[cr.LONG_LPF_LEAF]) > 256                             # k_lpf_long
    assert flat.vfos[3].decimate_count == 5 and flat.vfos[3].samples_per_buffer % 1024 != 0   # a partial last chunk
    assert {(flat.vfos[i].decimate_count, flat.vfos[i].late_decimate) for i in (4, 5, 6, 7)} == {(0, 5), (0, 6), (1, 5), (3, 6)}


def test_gains_keep_every_payload_inside_int16():
    """(a wrapped sample would turn the 1 LSB bar of the tolerance arithmetics into 65 535)"""
    for key in cr.TREES:
        topo, want, _, _ = cr.reference(key)
        usb = [i for i in topo.leaves_in_publish_order() if topo.vfos[i].demod_usb]
        for w in want:
            assert all(w["meters"][i]["clipped"] == 0 for i in usb), key
            assert all(c["meter"]["clipped"] == 0 for i, c in w["caught"].items() if i in usb), key
            assert max([0] + [int(np.abs(w["payload"][i]).max()) for i in usb if w["payload"][i] is not None]) > 50 or not any(w["active"][i] for i in usb), key  # (and are not silent)


@pytest.mark.parametrize("kind", ["port"] + (["reference"] if ob.have_reference() else []))
@pytest.mark.parametrize("key", sorted(cr.TREES))
def test_a_caught_up_leaf_is_a_fresh_oracle_node_fed_the_parent_stream_from_the_frame_before(key, kind):
    """Frames K-1, K, K+1 of the model == an oracle node built at the unpark and fed the model parent's decimate[d] from K-1 on
    (from K on for a leaf that is not caught up), bit for bit: stream and payload.  Every kind of live_ref.leaf_kinds."""
    topo, want, _, _ = cr.reference(key)
    checked = 0
    for i, K, caught in _unparks(key):
        if K + 1 >= cr.N_FRAMES or want[K + 1]["since"][i] != K:
            continue  # (parked or restarted again before K + 1: that unpark has a line of its own)
        d = want[K]["descs"][i]
        if d.parent < 0:
            assert not caught
            feed = lambda f: cr.frames(key)[f]  # noqa: E731
        else:
            feed = lambda f: np.ascontiguousarray(want[f]["streams"][d.parent]).view(np.float32)  # noqa: E731
        one = Topology(fs=d.fs, frame=d.samples_per_buffer, vfos=[dataclasses.replace(d, parent=-1)])
        nodes, _ = ob.build_tree(kind, one)
        for f in range(K - 1 if caught else K, K + 2):
            nodes[0].process(feed(f))
            if f == K - 1:
                c = want[K]["caught"][i]
                assert c["frame"] == K - 1
                z, pay = c["stream"], c["payload"]
            else:
                z, pay = want[f]["streams"][i], want[f]["payload"][i]
            assert np.array_equal(z.view(np.uint64), nodes[0].stream().view(np.uint64)), (key, i, K, f, "stream")
            got = nodes[0].usb() if d.demod_usb else nodes[0].iq()
            assert np.array_equal(pay, got), (key, i, K, f, "payload")
        if not caught:
            assert i not in want[K]["caught"]
        checked += 1
    assert checked >= 4, checked


def test_the_reported_state_of_the_frame_before_stays_parked():
    topo, want, _, gates = cr.reference("flat")
    # leaf 2 is caught up before frame 3: frame 2 itself still says parked, frame 3 says active since 3
    assert want[2]["payload"][2] is None and want[2]["meters"][2]["n_values"] == 0 and not gates[2][2]["open"]
    assert want[3]["since"][2] == 3 and want[3]["active"][2] == 1 and want[3]["caught"][2]["frame"] == 2
    assert want[6]["caught"][2]["frame"] == 2  # (as long as that active state lasts)


# ---- the delivery sequence, hand-worked -------------------------------------------------------------------------------------
S = [10, 10, 99, 10, 10, 10]  # one leaf's sum_sq per frame; frame 2 (parked) is never looked at


def test_threshold_zero_prerolls_the_caught_up_frame():
    g = cr.gate(S, {1: "p", 3: "c"}, 0, 0)
    assert [r["open"] for r in g] == [1, 0, 0, 1, 1, 1]
    assert [r["pre"] for r in g] == [0, 0, 0, 1, 0, 0]    # pre(K) = open(K): delivered twice in frame 3, once afterwards


def test_threshold_above_the_level_of_k_drops_the_caught_up_payload():
    g = cr.gate(S, {1: "p", 3: "c"}, [0, 0, 0, 50, 5, 5], 0)
    assert [r["open"] for r in g] == [1, 0, 0, 0, 1, 1]
    assert [r["pre"] for r in g] == [0, 0, 0, 0, 1, 0]    # frame 4 pre-rolls frame 3 (the ordinary rule), never frame 2
    g = cr.gate(S, {1: "p", 3: "c"}, [0, 0, 0, 50, 5, 5], 3)
    assert [r["open"] for r in g] == [1, 0, 0, 0, 1, 1]   # hang_frames does not help: no gate has run on frame 2


def test_parked_again_before_k_discards_and_a_restart_is_not_caught_up():
    g = cr.gate(S, {1: "p", 3: "cp"}, 0, 0)
    assert [r["open"] for r in g] == [1, 0, 0, 0, 0, 0] and sum(r["pre"] for r in g) == 0
    g = cr.gate(S, {3: "pu"}, 0, 0)                        # active in frame 2 and delivered then: the restart
    assert [r["open"] for r in g] == [1] * 6 and sum(r["pre"] for r in g) == 0
    g = cr.gate(S, {0: "pu"}, 0, 0)                        # K = 0
    assert sum(r["pre"] for r in g) == 0


def test_the_model_tree_decides_who_is_caught_up():
    """On the schedules: K >= 1 with a parent and parked in K-1 -> 'c'; parent-less, restart, K = 0 -> 'u'."""
    _, _, kinds, _ = cr.reference("flat")
    assert kinds[2] == {1: "p", 3: "c"} and kinds[4] == {1: "p", 4: "cpc"} and kinds[3] == {1: "p", 3: "c", 5: "pu"}
    _, _, kinds, _ = cr.reference("deep")
    assert kinds[5] == {1: "p", 3: "u"} and kinds[2] == {1: "p", 3: "c"}
    m = cr.CatchupTree(cr.deep_tree())
    m.park([2])
    m.unpark([2])  # K = 0
    assert m.kinds[2] == {0: "pu"} and not m.caught


def test_delivery_counts_and_bytes_on_the_flat_tree():
    topo, want, _, gates = cr.reference("flat")
    leaves = topo.leaves_in_publish_order()
    for f in range(cr.N_FRAMES):
        pub, n_open, n_pre, nbytes = cr.delivery(topo, want, gates, f)
        act = [i for i in leaves if want[f]["active"][i]]
        pre = [i for i in leaves if gates[i][f]["pre"]]
        assert n_open == len(act) and n_pre == len(pre) and len(pub) == n_open + n_pre
        assert nbytes == sum(sq.align64(want[f]["payload"][i].nbytes) for i in act + pre)
        # a pre-rolled leaf: two consecutive entries of one topic, the caught-up payload first
        for i in pre:
            t = live_ref.topic5(topo.vfos[i])
            k = [n for n, p in enumerate(pub) if p[0] == t]
            assert len(k) == 2 and k[1] == k[0] + 1
            assert pub[k[0]][2] == want[f]["caught"][i]["payload"].tobytes() and pub[k[1]][2] == want[f]["payload"][i].tobytes()
    assert {f: [i for i in leaves if gates[i][f]["pre"]] for f in (3, 4, 5)} == {3: [2, 3, 9], 4: [4, 5, 8], 5: [6, 7, 10]}
