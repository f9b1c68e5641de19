"""tests/spectrum_trees_ref.py alone, on the CPU: what the lattice and the random trees of seeds 0-19 cover as (layout, level,
size class) of the stream a spectrum reads, and that the expected displays can tell a wrong kernel from a right one -- a
wrong frame parity, a tile-layout stream read in natural order -- before tests/test_gpu_spectrum_trees.py compares the
device with them.  The model runs are the ones the GPU tests share (about 12 s for the lattice, 14 s for the seeds)."""
import numpy as np
import pytest

import lattice as lt
import live_ref as lr
import spectrum_ref as sr
import spectrum_trees_ref as st

TREES = lt.trees()
NAMES = sorted(TREES)
FLOOR_CAP = 0.15
FULL_SUB_TREES = ("sub-3840", "sub-8704")


def test_the_lattice_covers_exactly_these_cells():
    assert len(NAMES) == 19 and sum(len(t.vfos) for t in TREES.values()) == 153
    got = set().union(*(st.cells(t) for t in TREES.values()))
    assert got == st.LATTICE_CELLS, (sorted(got - st.LATTICE_CELLS), sorted(st.LATTICE_CELLS - got))


def test_the_random_trees_add_exactly_these_cells():
    """Beyond the lattice's: tiled level-1 streams shorter than a chunk, ending inside one and longer than the FFT, level-2
    leaves ending inside a chunk and longer than the FFT -- and one cell the list this test was written from had missed: a
    childless main of whole chunks (seed 9's node 2 with 5 120 samples, seed 14's node 0 with 4 096)."""
    topos = [lr.topology_of(s) for s in st.SEEDS]
    assert sum(len(t.vfos) for t in topos) == 154
    assert sum(1 for t in topos if max(lt.level(t, i) for i in range(len(t.vfos))) == 2) == 16, "three-level trees"
    got = set().union(*(st.cells(t) for t in topos)) - st.LATTICE_CELLS
    want = st.RANDOM_ADDS | {("natural", 0, "full")}
    assert got == want, (sorted(got - want), sorted(want - got))
    assert all(lv <= 2 for _, lv, _ in got | st.LATTICE_CELLS)


def _updates(states, i):
    """The distinct states of node i in frame order (a frame without an update repeats the object before it)."""
    out = []
    for per_frame in states:
        s = per_frame[i]
        if s.updates and (not out or s is not out[-1]):
            out.append(s)
    return out


def _sensitivity(runs):
    """(pairs of consecutive updates, pairs with identical bins, updates, updates at the floor) over `runs`"""
    pairs = same = ups = floor = 0
    for states in runs:
        for i in range(len(states[0])):
            u = _updates(states, i)
            assert [s.updates for s in u] == list(range(1, len(u) + 1))
            ups += len(u)
            floor += sum(st.at_floor(s.bins) for s in u)
            pairs += max(0, len(u) - 1)
            same += sum(np.array_equal(a.bins.view(np.uint32), b.bins.view(np.uint32)) for a, b in zip(u, u[1:]))
    return pairs, same, ups, floor


@pytest.mark.parametrize("family", ["lattice", "random"])
def test_the_reference_tells_frames_apart_and_is_mostly_above_the_floor(family):
    """No two consecutive updates of one node have the same bins: the stream of the other parity, or of another level's frame,
    cannot pass.  At most 15 % of the updates sit at the display's floor (every 100000 |bin| / 8192 <= 1, so that pwr stays 0
    and only the bins test anything): measured 87 of 717 on the lattice, 47 of 1 010 on seeds 0-19."""
    runs = [st.lattice_displays(n) for n in NAMES] if family == "lattice" else [st.random_displays(s) for s in st.SEEDS]
    pairs, same, ups, floor = _sensitivity(runs)
    print(f"{family}: {same} of {pairs} consecutive updates with identical bins; {floor} of {ups} updates at the floor "
          f"({100.0 * floor / ups:.1f} %)")
    assert pairs >= 500 and same == 0, (family, pairs, same)
    assert floor <= FLOOR_CAP * ups, (family, floor, ups)


def test_a_tiled_stream_read_in_natural_order_gives_other_bins():
    """For every inner node of the lattice: the first min(n, 8192) entries of its tile-layout buffer, taken as they lie, are
    not the stream, and their display is not the stream's -- for the nodes shorter than 8 192 samples and ending inside a chunk
    as well, where the last tile is partly empty."""
    n_tiled = 0
    for name in NAMES:
        topo = TREES[name]
        want, _ = lt.model_frames(name)
        for i in range(len(topo.vfos)):
            if not topo.children(i):
                continue
            z = want[0]["streams"][i]
            wrong = st.tiled(z)[:z.size]
            right, bad = sr.Display(), sr.Display()
            right.update(z)
            bad.update(wrong)
            assert np.array_equal(st.lattice_displays(name)[0][i].bins.view(np.uint32), right.bins.view(np.uint32)), (name, i)
            assert not np.array_equal(right.bins.view(np.uint32), bad.bins.view(np.uint32)), (name, i)
            n_tiled += 1
    assert n_tiled == 26, n_tiled


def test_the_untapped_leaves_are_the_ones_without_a_stream():
    """tap_plan against the rule of include/sdrx.h, spelled out once more from the descriptors: with the default options every
    late0 tree holds fused /5 or /6 leaves (d = 0 below the main), one of which stays untapped; the full sub trees hold two
    d = 2 leaves that demodulate in the wave once fuse_demod is set (it is off by default, and then they keep their streams);
    keep_streams leaves nothing without a stream; fuse_late = 0 gives the late leaves theirs back."""
    for name in NAMES:
        topo = TREES[name]
        for opts in (dict(), dict(fuse_demod=True), dict(fuse_late=False), dict(fuse_demod=True, keep_streams=True)):
            plan = st.tap_plan(topo, opts)
            assert len(plan["untapped"]) <= 1 and not set(plan["tapped"]) & set(plan["untapped"]), (name, opts)
            for i in plan["tapped"] + plan["untapped"]:
                d = topo.vfos[i]
                assert not topo.children(i) and d.demod_usb and d.parent >= 0 and not opts.get("keep_streams"), (name, opts, i)
                if d.late_decimate:
                    assert opts.get("fuse_late", True) and d.decimate_count == 0 and d.late_decimate in (5, 6), (name, opts, i)
                else:
                    assert opts.get("fuse_demod") and d.decimate_count == 2 and lt.lpf_taps(d) <= 64, (name, opts, i)
        if name.startswith("late0-"):
            plan = st.tap_plan(topo, dict())
            assert plan["untapped"] and plan["tapped"], name
            assert st.tap_plan(topo, dict(fuse_late=False)) == dict(tapped=[], untapped=[]), name
        if name in FULL_SUB_TREES:
            assert st.tap_plan(topo, dict()) == dict(tapped=[], untapped=[]), name
            plan = st.tap_plan(topo, dict(fuse_demod=True))
            assert plan["untapped"] and plan["tapped"], name
        assert st.tap_plan(topo, dict(fuse_demod=True, keep_streams=True)) == dict(tapped=[], untapped=[]), name
    assert len(st.tap_plan(TREES["late0-2400"], dict())["tapped"]) == 3
    lens = [st.stream_len(TREES["inner"], i) for i in st.tap_plan(TREES["inner"], dict(fuse_demod=True))["tapped"]]
    assert len(set(lens)) >= 3, ("tapped fused leaves of different lengths at once", lens)


def test_the_raw_display_follows_sdrjs_counter():
    frames = lt.frames("late0-1920")
    states = st.raw_display(frames)
    assert [s.updates for s in states] == [0, 0, 0, 0, 1]
    assert TREES["late0-1920"].frame == 3840 and states[4].bins.any()
    d = sr.Display()
    d.update(np.asarray(frames[4]).view(np.complex64))
    assert np.array_equal(states[4].bins.view(np.uint32), d.bins.view(np.uint32)) and states[4].maxval == d.maxval
