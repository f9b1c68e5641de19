"""The impulse blanker's model (sdrreceiver_amd.blank, the definition the device is held to): worked by hand on one short frame,
told apart from twelve wrong devices by the crafted cases of tests/blank_ref.py, run over noise with pulses, and through the
oracle's tree.  No GPU."""
import numpy as np
import pytest

import blank_ref as br
from oracle import binding as ob
from sdrreceiver_amd import blank as bl, ingest


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def test_by_hand_on_one_short_frame():
    """Twelve samples, G = 1, ratio 4, the median.  Powers 1 except x[3] = 3 + 4j (25), x[4] = 2 (4.0: AT the threshold) and
    x[9] = 0.5 (0.25)."""
    x = np.ones(12, np.complex64)
    x[3], x[4], x[9] = 3 + 4j, 2, 0.5
    cfg = bl.Cfg(4.0, 0.0, 32768, 1)
    # frame 0: no reference yet -- thr = +inf, nothing is blanked; the histogram: bin 1000 (0.25) 1, bin 1016 (1.0) 9, bin 1032
    # (4.0) 1, bin 1052 (25 = 1.5625 * 16: 1048 + floor(8 * 0.5625)) 1; 65536 cum >= 32768 * 12 first holds in bin 1016 (cum = 10)
    assert list(bl.bin_of(bl.power(x))[[9, 0, 4, 3]]) == [1000, 1016, 1032, 1052]
    y, rec, st = bl.apply(x, cfg)
    assert np.array_equal(_bits(y), _bits(x))
    assert rec == {"frame": 0, "n_complex": 12, "measured": 1, "thr_bits": bl.INF_BITS, "ref_bin": -1, "next_ref_bin": 1016, "hits": 0, "blanked": 0,
                   "runs": 0, "carry_in": 0}
    assert st == bl.State(1016, bl.NO_HIT, False, 1)
    # frame 1: thr = 4 * edge(1016) = 4.0; only x[3] is above it (4.0 > 4.0 is false); samples 2, 3, 4 become zero
    y, rec, st = bl.apply(x, cfg, st)
    want = x.copy()
    want[2:5] = 0
    assert np.array_equal(_bits(y), _bits(want))
    assert rec == {"frame": 1, "n_complex": 12, "measured": 1, "thr_bits": 0x40800000, "ref_bin": 1016, "next_ref_bin": 1016, "hits": 1, "blanked": 3,
                   "runs": 1, "carry_in": 0}
    assert st == bl.State(1016, 8, False, 2)
    # a frame whose last sample is a hit, then one with none: tail_gap 0, so G - 0 = 1 sample is carried, and the run that began
    # in the frame before is not counted again
    z = np.ones(12, np.complex64)
    z[11] = 5
    y, rec, st = bl.apply(z, cfg, st)
    assert (rec["hits"], rec["blanked"], rec["runs"], rec["carry_in"]) == (1, 2, 1, 0) and st == bl.State(1016, 0, True, 3)
    y, rec, st = bl.apply(np.ones(12, np.complex64), cfg, st)
    assert (rec["hits"], rec["blanked"], rec["runs"], rec["carry_in"]) == (0, 1, 0, 1) and y[0] == 0 and y[1] == 1
    assert st == bl.State(1016, bl.NO_HIT, False, 4)


def test_bins_edges_and_the_threshold():
    assert bl.edge(1016) == 1.0 and bl.edge(1015) == np.float32(0.9375) and bl.edge(0) == 0.0 and bl.edge(bl.MAX_BIN) == np.inf
    p = np.array([0.0, 1.0, br.down(1.0), np.inf, -0.0, np.nan], np.float32)
    assert list(bl.bin_of(p)[:5]) == [0, 1016, 1015, 2040, 0] and bl.bin_of(p)[5] > bl.MAX_BIN
    assert bl.power(np.array([1e30 + 0j], np.complex64))[0] == np.inf
    assert bl.thr_bits(bl.threshold(-1, br.cfg(0))) == bl.INF_BITS
    assert bl.threshold(1016, br.cfg(0, ratio=4.0, floor=3.0)) == 4.0 and bl.threshold(1016, br.cfg(0, ratio=4.0, floor=8.0)) == 8.0
    assert bl.threshold(0, br.cfg(0)) == 0.0 and bl.threshold(bl.MAX_BIN, br.cfg(0)) == np.inf
    assert not (np.float32(np.nan) > bl.threshold(1016, br.cfg(0)))  # a NaN power is no hit
    for bad in (bl.Cfg(0.5, 0, 1, 0), bl.Cfg(np.inf, 0, 1, 0), bl.Cfg(np.nan, 0, 1, 0), bl.Cfg(2, -1.0, 1, 0), bl.Cfg(2, np.inf, 1, 0),
                bl.Cfg(2, 0, 0, 0), bl.Cfg(2, 0, 65537, 0), bl.Cfg(2, 0, 1, -1), bl.Cfg(2, 0, 1, 65)):
        assert bl.check_cfg(bad)
    assert bl.check_cfg(bl.Cfg(1.0, 0.0, 65536, 64)) is None and bl.check_cfg(bl.Cfg(1e30, br.F32_MAX, 1, 0)) is None


def test_the_rank_rule_at_equality():
    h = np.zeros(bl.BINS, np.int64)
    h[1000], h[1016] = 128, 128
    assert bl.rank_bin(h, 256, 32768) == 1000  # 65536 * 128 == 32768 * 256
    h[1000], h[1016] = 127, 129
    assert bl.rank_bin(h, 256, 32768) == 1016
    assert bl.rank_bin(h, 256, 1) == 1000 and bl.rank_bin(h, 256, 65536) == 1016
    h[:] = 0
    h[2047] = 256
    assert bl.rank_bin(h, 256, 32768) == bl.MAX_BIN


def test_the_second_writing_of_the_definition_is_the_model():
    for c in br.crafted():
        assert br.same_run(br.run_wrong(c.frames, c.cfgs, None), br.model_run(c)), c.name


@pytest.mark.parametrize("how", br.WRONG)
def test_every_wrong_device_shows_on_a_crafted_case(how):
    by_name = {c.name: c for c in br.crafted()}
    c = by_name[br.CAUGHT_BY[how]]
    assert not br.same_run(br.run_wrong(c.frames, c.cfgs, how), br.model_run(c)), (how, c.name)


def test_crafted_cases_hold_what_they_are_named_for():
    by_name = {c.name: c for c in br.crafted()}
    for n in br.LENGTHS:
        for G in br.GUARDS:
            recs = br.model_run(by_name[f"ends_n{n}_G{G}"])[1]
            assert recs[0]["hits"] == 0 and recs[0]["thr_bits"] == bl.INF_BITS
            assert (recs[1]["hits"], recs[1]["runs"], recs[1]["blanked"]) == (2, 2, 2 * (G + 1))
            assert (recs[2]["hits"], recs[2]["carry_in"], recs[2]["blanked"], recs[2]["runs"]) == (0, G, G, 0)  # the run went on: not counted twice
            recs = br.model_run(by_name[f"bounds_n{n}_G{G}"])[1]
            assert recs[1]["hits"] == recs[2]["hits"] == len(br.boundaries(n))
            assert recs[2]["carry_in"] == max(0, G - (n - 1 - br.boundaries(n)[-1]))  # (0 but where the frame ends 16 behind a boundary)
            recs = br.model_run(by_name[f"pairs_n{n}_G{G}"])[1]
            assert recs[2]["carry_in"] == G - G // 2
            if n > 1024 and G:
                assert (recs[1]["hits"], recs[1]["runs"]) == (5, 4)  # 2 G apart: one run; 2 G + 2 apart: two; and the one at the end
        recs = br.model_run(by_name[f"edges_n{n}"])[1]
        assert [r["next_ref_bin"] for r in recs] == [1000, 1015, 1016]
        assert bl.threshold(1000, br.cfg(1)) == 1.0 and recs[1]["hits"] == 2  # the unit background sits AT the threshold
        assert recs[2]["thr_bits"] == bl.thr_bits(np.float32(3.75)) and recs[2]["hits"] == 1
        ys, recs, _ = br.model_run(by_name[f"inf_n{n}"])
        assert recs[1]["hits"] == 3 and recs[1]["next_ref_bin"] == bl.MAX_BIN and recs[2]["thr_bits"] == bl.INF_BITS and recs[2]["hits"] == 0
        assert all(np.isfinite(y.view(np.float32)).all() for y in ys)  # the tree never sees the 1e30 samples
        recs = br.model_run(by_name[f"zero_then_live_n{n}"])[1]
        assert recs[0]["next_ref_bin"] == 0 and recs[1]["thr_bits"] == 0 and recs[1]["hits"] == n - 30
        assert br.model_run(by_name[f"rank1_n{n}"])[1][1]["ref_bin"] == 1000 and br.model_run(by_name[f"rank65536_n{n}"])[1][1]["ref_bin"] == 1064
        assert br.model_run(by_name[f"floor_above_n{n}"])[1][1]["hits"] == 2 and br.model_run(by_name[f"floor_below_n{n}"])[1][1]["hits"] == 3


def test_records_chain_from_frame_to_frame():
    """thr_bits of frame f + 1 is rule 3 on next_ref_bin of frame f; ref_bin of f + 1 is next_ref_bin of f"""
    for c in br.crafted():
        recs = br.model_run(c)[1]
        assert recs[0]["ref_bin"] == -1 and recs[0]["thr_bits"] == bl.INF_BITS
        for f in range(1, br.N_FRAMES):
            assert recs[f]["ref_bin"] == recs[f - 1]["next_ref_bin"], (c.name, f)
            assert recs[f]["thr_bits"] == bl.thr_bits(bl.threshold(recs[f - 1]["next_ref_bin"], c.cfgs[f])), (c.name, f)
            hist = np.bincount(bl.bin_of(bl.power(c.frames[f])), minlength=bl.BINS)
            assert recs[f]["next_ref_bin"] == bl.rank_bin(hist, c.n, c.cfgs[f].rank_q16), (c.name, f)


def test_noise_and_pulses_every_pulse_sample_and_no_noise_sample():
    """40 seeds x 3 frames of 4112 CS16 samples: Gaussian noise of sigma = 8 dongle LSB with five 4-sample pulses of +-25 000 codes
    a frame; ratio 32, the median, G = 8.  Frame 0 flags nothing; frames 1 and 2 flag the 20 pulse samples and nothing else.  (The
    per-sample false-hit probability is below exp(-32 ln 2 2^(-1/8)) = 1.5e-9; this is a condition on the inputs, no tolerance.)"""
    total = 0
    for seed in range(br.NP_SEEDS):
        _, dirty, masks = br.noise_and_pulses(seed)
        xs = [ingest.to_float(v).view(np.complex64) for v in dirty]
        ys, recs = bl.run(xs, br.NP_CFG)
        assert recs[0]["hits"] == 0 and np.array_equal(_bits(ys[0]), _bits(xs[0]))
        for f in (1, 2):
            thr = np.array([recs[f]["thr_bits"]], np.uint32).view(np.float32)[0]
            hit = bl.power(xs[f]) > thr
            assert np.array_equal(hit, masks[f]), (seed, f, int((hit & ~masks[f]).sum()), int((~hit & masks[f]).sum()))
            assert recs[f]["hits"] == br.NP_PULSES * br.NP_LEN and recs[f]["runs"] == br.NP_PULSES
            assert recs[f]["blanked"] == br.NP_PULSES * (br.NP_LEN + 2 * br.NP_CFG.guard)
            keep = ~bl.dilate(masks[f], br.NP_CFG.guard)
            assert not ys[f][~keep].any() and np.array_equal(_bits(ys[f][keep]), _bits(xs[f][keep]))
        total += sum(x.size for x in xs)
    assert total == 40 * 3 * 4112


def test_the_blanker_lowers_every_leafs_error_through_the_oracle():
    """The same input through the oracle's tree three times -- without pulses, with them, and with them behind the model: on
    frames 1 and 2 every leaf's payload is closer to the pulse-free one with the blanker than without.  A comparison, not a
    number (measured while writing: the squared error falls by a factor of 6.8 at the least, 12 to 30 in the median)."""
    topo = br.effect_tree(br.NP_N)
    leaves = [i for i in range(len(topo.vfos)) if not topo.children(i)]
    assert len(leaves) == 3

    def payload(nodes, i):
        return (nodes[i].usb() if topo.vfos[i].demod_usb else nodes[i].iq()).astype(np.float64)

    for seed in range(br.NP_SEEDS):
        clean, dirty, _ = br.noise_and_pulses(seed)
        xs = [ingest.to_float(v).view(np.complex64) for v in dirty]
        ys, _ = bl.run(xs, br.NP_CFG)
        trees = [ob.build_tree("port", topo) for _ in range(3)]
        for f in range(br.N_FRAMES):
            for (_, roots), x in zip(trees, (ingest.to_float(clean[f]), xs[f].view(np.float32), ys[f].view(np.float32))):
                ob.process_roots(roots, np.ascontiguousarray(x, dtype=np.float32))
            if f == 0:
                continue
            for i in leaves:
                want = payload(trees[0][0], i)
                e_pulses = float(((payload(trees[1][0], i) - want) ** 2).sum())
                e_blanked = float(((payload(trees[2][0], i) - want) ** 2).sum())
                assert e_blanked < e_pulses, (seed, f, i, e_blanked, e_pulses)
