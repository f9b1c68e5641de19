"""The lattice of tests/lattice.py covers what it claims, and the oracle and the whole-tree model are pinned on it (CPU only).

* The covered (position, depth, kind) cells are the required ones: nobody can thin the lattice without this file noticing.
* Every descriptor passes sdrx_check_vfo on the host.
* The inputs are fit for the tolerance bar: no int16 wraps, no deep leaf is quiet, and the reference's own -O2 and -Ofast
  builds differ by less than half the 1e-5 bar on every node (measured: at most 4.3e-7, int16 within 1 LSB; per tree in the
  provenance of tests/golden/lattice.npz).
* The plain-C oracle equals the real reference build on every lattice tree (every stage stream, payload, tap set and
  outputRate) where that build loads, and the digests of tests/golden/lattice.npz -- made from the real build -- everywhere.
* live_ref.ModelTree equals the oracle with no controls, and under lattice.schedule, where the oracle side is: orc_vfo_retune
  (a fresh oscillator, filters kept), orc_vfo_set_gain, nothing for a parked leaf and a fresh oracle node, fed the oracle
  parent's stream, from the unpark on."""
import ctypes as C
import dataclasses
import hashlib

import numpy as np
import pytest

import lattice as lt
import live_ref as lr
from helpers import bits, golden
from oracle import binding as ob
from sdrreceiver_amd.topology import Topology

TREES = sorted(lt.trees())
REL_TOL = 1e-5  # BASELINE north star


def test_the_lattice_covers_every_required_cell():
    covered = set()
    for name, topo in lt.trees().items():
        c = lt.cells(topo)
        assert c, name
        covered |= c
        assert len(topo.vfos) <= 40 and topo.frame <= 65536 and topo.fs == 4 * topo.frame, name
    required = lt.required_cells()
    # the list of the issue, counted: 9 + 4 + 4 + 8 + 6 + 24 + 8 + 8 + 6 + 2 + 5
    assert len(required) == 84
    assert ("sub", 8, "usb") in required and ("root", 8, "late6") in required and ("inner1", 6, "usb+iq children") in required
    assert ("sub", 5, "pair:3+768") in required and ("sub", 5, "pair:8+0") in required and ("any", None, "scalecomp:100") in required
    missing = required - covered
    assert not missing, sorted(map(str, missing))
    # ... and nothing else but the by-products lattice.incidental_cells names: the covered set is pinned from both sides
    incidental = lt.incidental_cells()
    assert not (required & incidental)
    assert covered == required | incidental, sorted(map(str, covered ^ (required | incidental)))
    # no cell ends as a documented refusal: sdrx_finalize takes every tree (tests/test_gpu_lattice.py creates each one)


def test_every_descriptor_obeys_the_documented_geometry():
    for name, topo in lt.trees().items():
        for i, d in enumerate(topo.vfos):
            n, fs = d.samples_per_buffer, d.fs
            assert fs % 16 == 0 and n % 16 == 0 and fs >= 1024 and n <= fs and n % (1 << d.decimate_count) == 0, (name, i)
            assert n % 1024 == 0 or n % 1024 >= 256, (name, i)
            if d.parent >= 0:
                p = topo.vfos[d.parent]
                assert d.parent < i and n == p.samples_per_buffer >> p.decimate_count and fs == p.fs >> p.decimate_count, (name, i)
            else:
                assert n == topo.frame and fs == topo.fs, (name, i)
            if d.demod_usb and d.late_decimate:
                assert (n >> d.decimate_count) % d.late_decimate == 0 and (fs >> d.decimate_count) % d.late_decimate == 0, (name, i)


def test_every_descriptor_passes_check_vfo():
    from sdrreceiver_amd import _lib
    try:
        L = _lib.lib()
    except OSError as e:
        pytest.skip(f"libsdrx does not load here: {e}")
    for name, topo in lt.trees().items():
        for i, d in enumerate(topo.vfos):
            msg = C.create_string_buffer(200)
            assert L.sdrx_check_vfo(C.byref(_lib.desc_to_c(d)), msg, 200) == 0, (name, i, msg.value)


def test_the_filter_lengths_of_the_helper_are_the_oracle_s():
    """lattice.lpf_taps restates the design rule in plain arithmetic (the "<= 64 taps" cell and the gains lean on it)."""
    seen = 0
    for name, topo in lt.trees().items():
        nodes, _ = ob.build_tree("port", topo)
        for i, d in enumerate(topo.vfos):
            if not topo.children(i) and d.demod_usb:
                assert lt.lpf_taps(d) == (nodes[i].taps("fir_usb").size if d.filter_bw > 0 else 0), (name, i)
                seen += d.filter_bw > 0
    assert seen >= 10


def _tone_amplitude(stream, late):
    """The amplitude of the leaf's own tone in one frame of its stream: lattice.tones puts it an eighth of the OUTPUT rate
    above the centre, that is 1 / (8 late) cycles per stream sample.  A correlation with that one exponential: noise
    and the siblings' tones average out, which a maximum over |stream| does not tell apart from the tone."""
    n = np.arange(stream.size)
    return abs(np.sum(stream.astype(np.complex128) * np.exp(-2j * np.pi * n / (8.0 * late)))) / stream.size


@pytest.mark.parametrize("name", TREES)
def test_the_inputs_are_loud_and_do_not_wrap(name):
    topo = lt.trees()[name]
    want = lt.oracle_frames(name)
    for i, d in enumerate(topo.vfos):
        if topo.children(i):
            continue
        if lt.is_deep(topo, i):  # its own tone, through half-bands of unit gain (measured: 17.6 of 20 at the least)
            late = d.late_decimate if d.demod_usb and d.late_decimate else 1
            assert max(_tone_amplitude(w[i].stream(), late) for w in want) >= 0.5 * lt.TONE_AMP, (name, i)
        if d.demod_usb:
            peak = max(float(np.abs(w[i].usb_prequant()).max()) for w in want)
            assert 1000.0 <= peak < 20000.0, (name, i, peak)


def _try_reference(kind="reference"):
    if not ob.have_reference() or (kind == "reference_ofast" and not ob.have_reference_ofast()):
        pytest.skip(f"the {kind} build is not in oracle/_ref")
    try:
        ob.load(kind)
    except OSError as e:  # e.g. the Qt runtime is absent on this box
        pytest.skip(f"reference build not loadable here: {e}")


@pytest.mark.parametrize("name", TREES)
def test_the_reference_builds_agree_within_half_the_bar(name):
    """What the GPU's tolerance arithmetics are held to 1e-5 on must not be an input on which the reference's own two builds
    already use up the bar."""
    _try_reference()
    _try_reference("reference_ofast")
    topo = lt.trees()[name]
    a_nodes, a_roots = ob.build_tree("reference", topo)
    b_nodes, b_roots = ob.build_tree("reference_ofast", topo)
    for f, iq in enumerate(lt.frames(name)):
        ob.process_roots(a_roots, iq)
        ob.process_roots(b_roots, iq)
        for i, d in enumerate(topo.vfos):
            a, b = a_nodes[i].stream(), b_nodes[i].stream()
            assert float(np.abs(a - b).max()) < 0.5 * REL_TOL * float(np.abs(a).max()), (name, f, i)
            if not topo.children(i) and d.demod_usb:
                assert int(np.abs(a_nodes[i].usb().astype(np.int32) - b_nodes[i].usb().astype(np.int32)).max()) <= 1, (name, f, i)


@pytest.mark.parametrize("name", TREES)
def test_the_oracle_is_the_reference_on_the_lattice(name):
    _try_reference()
    topo = lt.trees()[name]
    port, ref = ob.build_tree("port", topo), ob.build_tree("reference", topo)
    for f, iq in enumerate(lt.frames(name)[:4]):
        ob.process_roots(port[1], iq)
        ob.process_roots(ref[1], iq)
        for i, d in enumerate(topo.vfos):
            a, b = port[0][i], ref[0][i]
            for s in range(d.decimate_count + 1):
                assert np.array_equal(bits(a.stream(s)), bits(b.stream(s))), (name, f, i, s)
            if not topo.children(i):
                if d.demod_usb:
                    assert a.usb().size == d.n_out and np.array_equal(a.usb(), b.usb()), (name, f, i)
                else:
                    assert a.iq().size > 0 and np.array_equal(a.iq(), b.iq()), (name, f, i)
    for i, d in enumerate(topo.vfos):
        a, b = port[0][i], ref[0][i]
        assert a.outputRate == b.outputRate == d.output_rate, (name, i)
        for which in ("fir_usb", "fir_dec", "hilbert"):
            assert np.array_equal(bits(a.taps(which)), bits(b.taps(which))), (name, i, which)


def _digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()[:8], np.uint8)


@pytest.mark.parametrize("name", TREES)
def test_the_oracle_reproduces_the_reference_fixture(name):
    """tests/golden/lattice.npz holds what the real reference build gave (make_golden.py lattice): the pin that survives
    where that build is absent."""
    g = golden("lattice.npz")
    topo = lt.trees()[name]
    n = int(g["frames"])
    assert g[name].shape == (n, len(topo.vfos), 2, 8), "the lattice changed: regenerate the fixture from the reference build"
    want = lt.oracle_frames(name)
    for f in range(n):
        for i, d in enumerate(topo.vfos):
            assert np.array_equal(_digest(want[f][i].stream()), g[name][f, i, 0]), (name, f, i, "stream")
            if not topo.children(i):
                pay = want[f][i].usb() if d.demod_usb else want[f][i].iq()
                assert np.array_equal(_digest(pay), g[name][f, i, 1]), (name, f, i, "payload")
            else:
                assert not g[name][f, i, 1].any()


@pytest.mark.parametrize("name", TREES)
def test_the_model_tree_is_the_oracle_without_controls(name):
    topo = lt.trees()[name]
    model = lr.ModelTree(topo)
    want = lt.oracle_frames(name)
    for f, iq in enumerate(lt.frames(name)):
        got = model.process(iq)
        for i, d in enumerate(topo.vfos):
            assert np.array_equal(bits(got["streams"][i]), bits(want[f][i].stream())), (name, f, i, "stream")
            if not topo.children(i):
                pay = want[f][i].usb() if d.demod_usb else want[f][i].iq()
                assert pay.size > 0 and np.array_equal(got["payload"][i], pay), (name, f, i, "payload")


@pytest.mark.parametrize("name", TREES)
def test_the_model_tree_is_the_oracle_under_the_schedule(name):
    # (the reference has no retune: orc_vfo_retune is held to live_ref.ModelTree here, two independently written sides, and
    # not to the reference build -- unlike everything else the oracle does on these trees)
    topo = lt.trees()[name]
    sched = lt.schedule(topo)
    kinds = {op[0] for ops in sched for op in ops}
    assert {"park", "unpark", "freq", "gain"} <= kinds, (name, kinds)
    want, _ = lt.model_frames(name)
    descs = list(topo.vfos)
    nodes, roots = ob.build_tree("port", topo)
    fresh = {}       # leaf -> the oracle node that replaced it at its unpark
    parked = set()
    for f, iq in enumerate(lt.frames(name)):
        for op in sched[f]:
            if op[0] == "park":
                parked |= set(op[1])
            elif op[0] == "unpark":
                for i in op[1]:
                    parked.discard(i)
                    alone = dataclasses.replace(descs[i], parent=-1)
                    fresh[i] = ob.build_tree("port", Topology(fs=alone.fs, frame=alone.samples_per_buffer, vfos=[alone]))[0][0]
            elif op[0] == "freq":
                descs[op[1]] = dataclasses.replace(descs[op[1]], mixer_freq=float(op[2]))
                fresh.get(op[1], nodes[op[1]]).retune(op[2])
            else:
                descs[op[1]] = dataclasses.replace(descs[op[1]], gain=float(np.float32(op[2])))
                fresh.get(op[1], nodes[op[1]]).setGain(op[2])
        ob.process_roots(roots, iq)
        for i, node in fresh.items():
            p = descs[i].parent
            node.process(iq if p < 0 else nodes[p].stream().view(np.float32))
        for i, d in enumerate(descs):
            w = want[f]
            if i in parked:
                assert w["streams"][i] is None and w["payload"][i] is None, (name, f, i)
                continue
            o = fresh.get(i, nodes[i])
            assert np.array_equal(bits(w["streams"][i]), bits(o.stream())), (name, f, i, "stream")
            if not topo.children(i):
                assert np.array_equal(w["payload"][i], o.usb() if d.demod_usb else o.iq()), (name, f, i, "payload")
    # the schedule did something: a retuned node's stream is not the untouched oracle's
    plain = lt.oracle_frames(name)
    for op in sched[2]:
        if op[0] == "freq":
            assert not np.array_equal(bits(want[2]["streams"][op[1]]), bits(plain[2][op[1]].stream())), (name, op)
