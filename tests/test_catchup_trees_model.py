"""Catch-up on the random trees and on the lattice: what tests/test_gpu_catchup_trees.py compares the device with (CPU only).

* The schedules reach what they claim: every row of catchup_ref.REQUIRED over the 60 seeds, and on the lattice every cell of
  lattice.required_cells() that a leaf with a parent occupies, held by a caught-up leaf.
* The model is the oracle: frames K-1, K, K+1 of a caught-up leaf equal a fresh plain-C oracle node fed the parent's model
  stream from K-1 on (the method of tests/test_catchup_model.py), on every third seed and on every lattice tree.
* The GPU tests have teeth: at frame K a caught-up leaf's payload differs from live_ref.ModelTree's under the same schedule
  on at least 95 % of the caught-up leaves, so a library that ignored the option, or ran K-1 wrongly, cannot match.
* The gate settings drawn from the model's meters open and close every leaf that has a threshold."""
import dataclasses
import os

import numpy as np
import pytest

import catchup_ref as cr
import lattice as lt
import live_ref as lr
from oracle import binding as ob
from sdrreceiver_amd.topology import Topology
from test_park_model import NONE, gate_with_parking

N_SEEDS = int(os.environ.get("SDRX_TEST_SEEDS", "60"))
LATTICE = sorted(lt.trees())


def _delivered_catchups(want):
    """(leaf, K, record) of every catch-up whose leaf then ran frame K"""
    out = []
    for f, w in enumerate(want):
        for i, c in w["caught"].items():
            if c["frame"] == f - 1 and w["since"][i] == f:
                out.append((i, f, c))
    return out


def test_the_event_c_is_an_unpark_that_leaves_prev_open_zero():
    s = [10, 10, 99, 10, 50, 3, 60]
    for ratio, window in ((0, 0), (512, 2)):
        u = gate_with_parking(s, {1: "p", 3: "u"}, 8, 1, ratio, window)
        c = gate_with_parking(s, {1: "p", 3: "c"}, 8, 1, ratio, window)
        assert [r["pre"] for r in u][3] == 0 and [r["pre"] for r in c][3] == 1
        for a, b in zip(u, c):  # nothing else differs: the floor, the hang time and the threshold restart as for 'u'
            assert {k: v for k, v in a.items() if k != "pre"} == {k: v for k, v in b.items() if k != "pre"}
        assert c[3]["floor"] == NONE and c[3]["hang_left"] == 1 and c[3]["prev_open"] == 1
    # 'c' on an active leaf is ignored, as 'u' is; closed in K: nothing is pre-rolled and K + 1 pre-rolls K
    assert gate_with_parking(s, {3: "c"}, 8, 0) == gate_with_parking(s, {}, 8, 0)
    c = gate_with_parking(s, {1: "p", 3: "c"}, [0, 0, 0, 50, 5, 5, 5], 0)
    assert [r["open"] for r in c] == [1, 0, 0, 0, 1, 0, 1]  # (3 < 5 closes frame 5)
    assert [r["pre"] for r in c] == [0, 0, 0, 0, 1, 0, 1]   # frame 4 pre-rolls frame 3, never the caught-up frame 2
    assert cr.gate(s, {1: "p", 3: "c"}, 8, 1, 512, 2) == gate_with_parking(s, {1: "p", 3: "c"}, 8, 1, 512, 2)


def test_the_schedules_catch_up_every_kind_and_every_case():
    """A condition on the generators, not a measurement."""
    total = {}
    for seed in range(max(N_SEEDS, 60)):
        topo, _, sched, want, _, _, kinds = cr.reference_random(seed)
        for k, v in cr.coverage(topo, sched, want, kinds).items():
            total[k] = total.get(k, 0) + v
    table = "\n".join(f"{k:45s} {total.get(k, 0)}" for k in sorted(set(total) | set(cr.REQUIRED)) if not k.startswith("cell:"))
    print(table)
    missing = [k for k in cr.REQUIRED if not total.get(k)]
    assert not missing, f"missing: {missing}\n{table}"


def test_the_lattice_schedule_catches_up_every_cell_a_leaf_with_a_parent_holds():
    total = {}
    for name in LATTICE:
        topo, _, sched, want, _, kinds = cr.reference_lattice(name)
        below = [i for i in topo.leaves_in_publish_order() if topo.vfos[i].parent >= 0]
        assert below, name
        c = cr.coverage(topo, sched, want, kinds)
        assert c.get("parity:1") and c.get("pu_restart") == 1 and c.get("freq_then_unpark_caught", 0) <= 1, (name, c)
        assert len(below) < 2 or c.get("parity:0"), (name, c)
        assert {i for i, _, _ in _delivered_catchups(want)} == set(below), name  # every leaf with a parent, once
        assert sum(1 for ops in sched for op in ops if op[0] == "gain") == (1 if any(topo.vfos[i].demod_usb for i in below[1::2]) else 0), name
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    need = cr.required_lattice_cells()
    assert len(need) >= 60, len(need)  # (the rest: the inner-node cells and the parent-less late leaves)
    assert {c for c in lt.required_cells() - need if c[0] not in ("root", "inner0", "inner1")} == set()
    missing = sorted(str(c) for c in need if not total.get(f"cell:{c}"))
    assert not missing, missing
    for k in ("caught_after_parked_retune", "freq_then_unpark_caught", "one_call_two_levels", "caught_on_level_2"):
        assert total.get(k), k
    assert all(total.get("caught:" + k) for k in lr.KINDS if k != "childless_main")


def _pin_to_the_oracle(tag, topo, want, n_frames):
    """Frames K-1 (the catch-up record), K and K+1 of every caught-up leaf against a fresh oracle node fed the model parent's
    stream from K-1.  The oracle's oscillator is built once, so a leaf retuned or re-gained in K or K+1 (or parked again) is
    left to the leaves that are not.  Returns (checked, left out)."""
    checked = left = 0
    for i, K, c in _delivered_catchups(want):
        d = c["desc"]
        last = min(K + 1, n_frames - 1)
        if any(want[f]["descs"][i] != d or want[f]["since"][i] != K for f in range(K, last + 1)):
            left += 1
            continue
        one = Topology(fs=d.fs, frame=d.samples_per_buffer, vfos=[dataclasses.replace(d, parent=-1)])
        nodes, _ = ob.build_tree("port", one)
        for f in range(K - 1, last + 1):
            nodes[0].process(np.ascontiguousarray(want[f]["streams"][d.parent]).view(np.float32))
            z, pay = (c["stream"], c["payload"]) if f == K - 1 else (want[f]["streams"][i], want[f]["payload"][i])
            assert np.array_equal(z.view(np.uint64), nodes[0].stream().view(np.uint64)), (tag, i, K, f, "stream")
            assert np.array_equal(pay, nodes[0].usb() if d.demod_usb else nodes[0].iq()), (tag, i, K, f, "payload")
        checked += 1
    return checked, left


def test_caught_up_leaves_of_the_random_trees_are_fresh_oracle_nodes_fed_from_the_frame_before():
    checked = left = 0
    for seed in range(0, N_SEEDS, 3):
        topo, frames, _, want, _, _, _ = cr.reference_random(seed)
        a, b = _pin_to_the_oracle(seed, topo, want, len(frames))
        checked, left = checked + a, left + b
    assert checked >= 2 * left and checked >= N_SEEDS // 3, (checked, left)


@pytest.mark.parametrize("name", LATTICE)
def test_caught_up_leaves_of_the_lattice_are_fresh_oracle_nodes_fed_from_the_frame_before(name):
    topo, frames, _, want, _, _ = cr.reference_lattice(name)
    checked, left = _pin_to_the_oracle(name, topo, want, len(frames))
    assert left <= 1 and checked >= 1, (name, checked, left)  # (the restart before frame 4 takes one K + 1 away)


def _model_without_the_option(topo, frames, sched):
    model = lr.ModelTree(topo)
    out = []
    for f, iq in enumerate(frames):
        model.apply(sched[f])
        out.append(model.process(iq))
    return out


def test_a_library_that_ignored_the_option_could_not_pass():
    """Per caught-up leaf: the payload of frame K with the catch-up against the payload of K without it (live_ref.ModelTree:
    the new vfo starts at K).  Identical ones -- a leaf with no state whose oscillator table wraps with the frame -- are
    counted: at most 5 % on the random trees and on the lattice each.  And the caught-up payload itself is not silence."""
    for what, runs in (("random", [cr.reference_random(s)[:4] + (lr.reference(s)[3],) for s in range(N_SEEDS)]),
                       ("lattice", [cr.reference_lattice(n)[:4] for n in LATTICE])):
        n = same = silent = 0
        for run in runs:
            topo, frames, sched, want = run[:4]
            base = run[4] if len(run) > 4 else _model_without_the_option(topo, frames, sched)
            for i, K, c in _delivered_catchups(want):
                n += 1
                assert base[K]["payload"][i] is not None and base[K - 1]["payload"][i] is None, (what, i, K)
                same += bool(np.array_equal(want[K]["payload"][i], base[K]["payload"][i]))
                silent += not np.any(c["payload"])
        print(f"{what}: {n} caught-up leaves, {same} with the payload of K unchanged, {silent} silent catch-ups")
        assert n >= (100 if N_SEEDS >= 60 or what == "lattice" else 1), (what, n)
        assert same * 20 <= n, (what, same, n)
        assert silent * 20 <= n, (what, silent, n)


def test_every_gated_leaf_opens_and_closes_in_the_model_and_none_is_exempt():
    """live_ref.gate_settings on the CatchupTree's own meters and events: no leaf ends in `exempt` (share 0 -- the figure the
    GPU test relies on), every leaf with a threshold has an open and a closed active frame, and some caught-up leaf is open in
    K (pre-rolls the catch-up) and some is closed in K (drops it)."""
    gated = exempt = leaves = pre_k = closed_k = auto_k = 0
    for seed in range(N_SEEDS):
        topo, _, _, want, gate, _, kinds = cr.reference_random(seed)
        exempt += len(gate["exempt"])
        leaves += len(topo.leaves_in_publish_order())
        for i in topo.leaves_in_publish_order():
            g = gate["gate"][i]
            for j, K, _ in _delivered_catchups(want):
                if j == i:
                    assert g[K]["pre"] == g[K]["open"] and g[K]["floor"] == NONE, (seed, i, K)
                    pre_k += g[K]["open"]
                    closed_k += not g[K]["open"]
                    auto_k += gate["ratio"][i] > 0
            if gate["thr"][i] == 0:
                continue
            act = [r for r in g if r["active"]]
            assert any(r["open"] for r in act) and any(not r["open"] for r in act), (seed, i, gate["thr"][i])
            gated += 1
    assert exempt == 0, (exempt, leaves)
    assert gated >= N_SEEDS
    assert N_SEEDS < 60 or (pre_k >= 20 and closed_k >= 20 and auto_k >= 10), (pre_k, closed_k, auto_k)
