"""tests/live_ref.py is a valid oracle and its generator covers what it claims (CPU only).

* With an empty schedule ModelTree IS the plain-C oracle on every random tree of the seed range: every stream of every node and
  every payload of every leaf, bit for bit -- retune_ref.Node chained parent to child, on trees with IQ leaves of both compress
  styles, childless mains, d = 0 leaves, the /5 and /6 late decimation and three levels.
* A leaf unparked before frame K is a fresh oracle node fed the oracle parent's stream from K on: one leaf of every kind, taken
  from the random trees.
* The schedules of the default seeds park and later deliver every kind of leaf, retune inner nodes above inner nodes, childless
  mains and parked leaves, and restart leaves between two frames.
* The gate settings drawn from the model's meters open and close every leaf that has a threshold."""
import dataclasses
import os

import numpy as np

import live_ref as lr
import retune_ref as rr
from helpers import bits
from oracle import binding as ob
from sdrreceiver_amd import synth
from sdrreceiver_amd.topology import Topology

N_SEEDS = int(os.environ.get("SDRX_TEST_SEEDS", "60"))


def _tone_frames(topo, n, seed):
    """The frames of test_gpu_parity.py::test_random_trees_against_the_oracle."""
    lcg = synth.Lcg(seed)
    tones = [(topo.fs / 7.3, 20.0), (-topo.fs / 3.1, 9.0)]
    return [synth.lcg_frame(topo.frame, lcg) + synth.tone_frame(topo.frame, topo.fs, tones, f * topo.frame) for f in range(n)]


def _payload(node, desc):
    return node.usb() if desc.demod_usb else node.iq()


def test_the_model_tree_is_the_oracle_on_every_random_tree():
    compared = 0
    for seed in range(N_SEEDS):
        topo = lr.topology_of(seed)
        nodes, roots = ob.build_tree("port", topo)
        model = lr.ModelTree(topo)
        for f, iq in enumerate(_tone_frames(topo, 3, seed)):
            ob.process_roots(roots, iq)
            got = model.process(iq)
            for i, d in enumerate(topo.vfos):
                assert np.array_equal(bits(got["streams"][i]), bits(nodes[i].stream())), (seed, f, i, "stream")
                compared += 1
                if not topo.children(i):
                    want = _payload(nodes[i], d)
                    assert want.size > 0 and np.array_equal(got["payload"][i], want), (seed, f, i, "payload")
            assert [p[0] for p in got["published"]] == [lr.topic5(topo.vfos[i]) for i in topo.leaves_in_publish_order()]
    assert compared >= 3 * 2 * N_SEEDS  # (no tree has fewer than one main: nothing was skipped)


def _one_leaf_of_every_kind():
    found = {}
    for seed in range(60):
        topo = lr.topology_of(seed)
        for i in topo.leaves_in_publish_order():
            for k in lr.leaf_kinds(topo, i):
                found.setdefault(k, (seed, i))
    return found


def test_a_fresh_model_node_equals_a_fresh_oracle_node_for_every_kind_of_leaf():
    """test_park_model.py's pin on the random trees: the oracle tree runs n frames; a retune_ref.Node and an oracle node, both
    created before frame K, are fed the oracle parent's decimate[d] (the raw frame for a childless main) from K on."""
    K, n = 2, 4
    found = _one_leaf_of_every_kind()
    assert set(found) == set(lr.KINDS), sorted(set(lr.KINDS) - set(found))
    for kind, (seed, i) in sorted(found.items()):
        topo = lr.topology_of(seed)
        d = topo.vfos[i]
        nodes, roots = ob.build_tree("port", topo)
        alone = dataclasses.replace(d, parent=-1)
        fresh, _ = ob.build_tree("port", Topology(fs=d.fs, frame=d.samples_per_buffer, vfos=[alone]))
        model = rr.Node(d)
        for f, iq in enumerate(lr.frames_of(topo, seed, n)):
            ob.process_roots(roots, iq)
            if f < K:
                continue
            x = iq.view(np.complex64) if d.parent < 0 else nodes[d.parent].stream()
            z = model.process(x)
            fresh[0].process(np.ascontiguousarray(x).view(np.float32))
            assert np.array_equal(bits(z), bits(fresh[0].stream())), (kind, seed, i, f, "stream")
            pay = model.payload()  # (once per frame: it advances the filter histories)
            assert np.array_equal(pay, _payload(fresh[0], d)), (kind, seed, i, f, "payload")
            # and it is NOT the node that ran from frame 0 on, wherever the leaf has any state to differ in
            if f == K and (d.decimate_count > 0 or d.demod_usb):
                assert not np.array_equal(pay, _payload(nodes[i], d)), (kind, seed, i, "a fresh node that differs in nothing")


def test_the_schedules_are_well_formed():
    for seed in range(N_SEEDS):
        topo = lr.topology_of(seed)
        sched = lr.random_schedule(topo, np.random.default_rng(20000 + seed), lr.N_FRAMES)
        assert len(sched) == lr.N_FRAMES and sched[0] == [] and sched[1] == [], seed
        assert any(not ops for ops in sched[2:]), (seed, "no frame without a call")
        leaves = set(topo.leaves_in_publish_order())
        for ops in sched:
            for op in ops:
                if op[0] in ("park", "unpark"):
                    assert op[1] and set(op[1]) <= leaves and len(set(op[1])) == len(op[1]), (seed, op)
                elif op[0] == "freq":
                    fs = topo.vfos[op[1]].fs
                    assert -fs / 2 < op[2] < fs / 2 and np.isfinite(rr.table(fs, op[2])).all(), (seed, op)
                else:
                    assert op[0] == "gain" and op[1] in leaves and op[2] == float(np.float32(op[2])), (seed, op)


def test_the_schedules_cover_every_kind():
    """A condition on the generator, not a measurement: over the default 60 seeds every row of REQUIRED is met at least once."""
    total = {}
    for seed in range(max(N_SEEDS, 60)):
        topo = lr.topology_of(seed)
        c = lr.coverage(topo, lr.random_schedule(topo, np.random.default_rng(20000 + seed), lr.N_FRAMES))
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    table = "\n".join(f"{k:45s} {total.get(k, 0)}" for k in sorted(set(total) | set(lr.REQUIRED)))
    print(table)
    missing = [k for k in lr.REQUIRED if not total.get(k)]
    assert not missing, f"missing: {missing}\n{table}"
    for k in ("freq_zero", "freq_non_integer", "freq_integer", "gain_usb", "gain_iq", "retune_with_unpark", "quiet_frame"):
        assert total.get(k), f"missing: {k}\n{table}"


def test_every_gated_leaf_opens_and_closes_in_the_model():
    gated = 0
    for seed in range(N_SEEDS):
        topo, _, _, _, gate, _ = lr.reference(seed)
        assert not gate["exempt"], (seed, gate["exempt"])
        for i in topo.leaves_in_publish_order():
            if gate["thr"][i] == 0:
                continue
            act = [r for r in gate["gate"][i] if r["active"]]
            assert any(r["open"] for r in act) and any(not r["open"] for r in act), (seed, i, gate["thr"][i])
            gated += 1
    assert gated >= N_SEEDS  # (four leaves in five get a threshold)
