"""The IQ balance correction's model (sdrreceiver_amd.iqbal, the definition the device is held to): worked by hand on one
16-sample frame, told apart from thirteen wrong devices by the crafted cases of tests/iq_ref.py, shown to converge as a Newton step
does, and through the oracle's tree.  No GPU."""
import math

import numpy as np
import pytest

import adc_ref as ar
import iq_ref as ir
from oracle import binding as ob
from sdrreceiver_amd import iqbal as iq, ingest, topology as tp


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def test_by_hand_on_one_frame_of_sixteen():
    """Twelve samples (+-1, -+1), four (+-1, +-1); mu = 1 from (0, 1).  q(+-1) = +-256, so S_i = S_q = 0, S_ii = S_qq = 16 * 65536,
    S_iq = (4 - 12) * 65536: A = B = 65536, C = -32768, ep = -1/2, eg = 0, g = 1 -- the step lands on c = 1/2 exactly, d stays."""
    x = ir.pattern(16, [(1, -1), (-1, 1), (1, -1), (-1, -1), (-1, 1), (1, -1), (-1, 1), (1, 1)])
    cfg = iq.Cfg(1.0, 0.0)
    y, rec, st = iq.apply(x, cfg)
    assert np.array_equal(_bits(y), _bits(x))  # (0, 1): Q' = Q
    assert rec == {"frame": 0, "n_complex": 16, "measured": 1, "adapted": 1, "rejected": 0, "c_bits": 0, "d_bits": 0x3F800000, "next_c_bits": 0x3F000000,
                   "next_d_bits": 0x3F800000, "sum_i": 0, "sum_q": 0, "sum_iq": -8 * 65536, "sum_ii": 16 * 65536, "sum_qq": 16 * 65536}
    assert st == iq.State(0.5, 1.0, 1)
    # the same frame under (1/2, 1): Q' = -+1/2 (twelve) and -+3/2 (four); q = -+128, -+384.  S_qq = 12 * 128^2 + 4 * 384^2 = 786432,
    # S_iq = 12 * (-32768) + 4 * 98304 = 0: decorrelated.  A = 65536, B = 49152, eg = 1/7, g = 8/7, c_next = 4/7 > 1/2: the step is
    # refused, the pair stays
    y, rec, st = iq.apply(x, cfg, st)
    assert list(y.imag[:4]) == [-0.5, 0.5, -0.5, -1.5] and list(y.real) == list(x.real)
    assert (rec["sum_q"], rec["sum_qq"], rec["sum_iq"], rec["sum_ii"]) == (0, 786432, 0, 16 * 65536)
    assert (rec["measured"], rec["adapted"], rec["rejected"]) == (1, 0, 1) and (rec["c_bits"], rec["next_c_bits"]) == (0x3F000000, 0x3F000000)
    assert st == iq.State(0.5, 1.0, 2)
    # mu = 1/4: g = 1 + 1/28, c_next = (float)(29/56): refused as well; d_next alone would have been fine -- the pair moves as one
    y, rec, st2 = iq.apply(x, iq.Cfg(0.25, 0.0), st)
    assert rec["rejected"] == 1 and st2 == iq.State(0.5, 1.0, 3)
    # min_power: (A + B) 2^-16 = 1.75 here
    assert iq.apply(x, iq.Cfg(0.25, 1.75), st)[1]["measured"] == 1 and iq.apply(x, iq.Cfg(0.25, float(ir.up(1.75))), st)[1]["measured"] == 0
    # mu = 0 holds: measured, never moved
    y, rec, st3 = iq.apply(x, iq.Cfg(0.0, 0.0), st)
    assert (rec["measured"], rec["adapted"], rec["rejected"]) == (1, 0, 0) and st3 == iq.State(0.5, 1.0, 3)


def test_the_quantiser_and_the_apply_at_their_edges():
    q = iq.quantise(np.array([0.5 / 256, 1.5 / 256, 2.5 / 256, -0.5 / 256, -1.5 / 256, ir.up(0.5 / 256), ir.down(1.5 / 256), 127.99, 128.0, -128.0, 1e30, -1e30,
                              np.inf, -np.inf, np.nan, 127.998046875, -0.0], np.float32))
    assert list(q) == [0, 2, 2, 0, -2, 1, 1, 32765, 32767, -32767, 32767, -32767, 32767, -32767, 0, 32767, 0]
    x = np.array([complex(3.0, -0.0), complex(-3.0, -0.0), complex(np.inf, 1.0), complex(np.nan, 1.0), complex(1.0, np.nan), complex(1e30, 2.0)], np.complex64)
    y = iq.correct(x, 0.0, 1.0).view(np.uint32)
    assert np.array_equal(y[0::2], x.view(np.uint32)[0::2])  # I' = I, bits kept -- a NaN's too
    # -0 in Q becomes +0 behind a non-negative I and stays behind a negative one; a non-finite I makes Q' the one NaN, at c = 0 too
    assert list(y[1::2]) == [0, 0x80000000, iq.NAN_BITS, iq.NAN_BITS, iq.NAN_BITS, 0x40000000]
    for bad in (iq.Cfg(-0.1, 0), iq.Cfg(1.1, 0), iq.Cfg(np.nan, 0), iq.Cfg(0.5, -1.0), iq.Cfg(0.5, np.inf), iq.Cfg(0.5, np.nan), iq.Cfg(0.5, 0, 0.51), iq.Cfg(0.5, 0, -0.51),
                iq.Cfg(0.5, 0, np.nan), iq.Cfg(0.5, 0, 0, 0.49), iq.Cfg(0.5, 0, 0, 2.01), iq.Cfg(0.5, 0, 0, np.nan), iq.Cfg(0.5, 0, 0, 1, 2), iq.Cfg(0.5, 1e39)):
        assert iq.check_cfg(bad), bad
    assert iq.check_cfg(iq.Cfg(0.0, 0.0, -0.5, 0.5)) is None and iq.check_cfg(iq.Cfg(1.0, 3e38, 0.5, 2.0, iq.IQ_LOAD)) is None


def test_the_second_writing_of_the_definition_is_the_model():
    for c in ir.crafted():
        assert ir.same_run(ir.run_wrong(c.frames, c.cfg, None), ir.model_run(c)[:2]), c.name


@pytest.mark.parametrize("how", ir.WRONG)
def test_every_wrong_device_shows_on_a_crafted_case(how):
    c = ir.by_name(ir.CAUGHT_BY[how])
    assert not ir.same_run(ir.run_wrong(c.frames, c.cfg, how), ir.model_run(c)[:2]), (how, c.name)


def test_crafted_cases_hold_what_they_are_named_for():
    assert len(ir.WRONG) == 13 and set(ir.CAUGHT_BY) == set(ir.WRONG)
    full = 32767 * 32767
    for n in ir.LENGTHS:
        recs = ir.model_run(ir.by_name(f"clamp_n{n}"))[1]
        assert (recs[0]["sum_ii"], recs[0]["sum_qq"], recs[0]["sum_iq"], recs[0]["sum_i"]) == (n * full, n * full, n * full, n * 32767) and recs[0]["measured"] == 0
        assert (recs[1]["sum_iq"], recs[1]["sum_q"]) == (-n * full, -n * 32767)
        recs = ir.model_run(ir.by_name(f"minpower_eq_n{n}"))[1]
        A, B, _ = iq.moments(recs[0], n)
        assert (A + B) * 2.0 ** -16 == 2.0 and [r["measured"] for r in recs] == [1, 0, 1, 1]
        recs = ir.model_run(ir.by_name(f"minpower_below_n{n}"))[1]
        A, B, _ = iq.moments(recs[0], n)
        assert 2.0 - 1.0 / (64 * n) < (A + B) * 2.0 ** -16 < 2.0 and [r["measured"] for r in recs] == [0, 1, 0, 1]
        assert [r["measured"] for r in ir.model_run(ir.by_name(f"zero_then_live_n{n}"))[1]] == [0, 1, 1, 0]
        recs = ir.model_run(ir.by_name(f"q_zero_n{n}"))[1]
        assert recs[0]["sum_qq"] == 0 and recs[0]["sum_ii"] > 0 and [r["measured"] for r in recs] == [0, 1, 1, 1]
        half, two = iq.bits(0.5), iq.bits(2.0)
        r = ir.model_run(ir.by_name(f"limit_c_on_n{n}"))[1][0]
        assert (r["adapted"], r["rejected"], r["next_c_bits"]) == (1, 0, half)
        r = ir.model_run(ir.by_name(f"limit_c_on_neg_n{n}"))[1][0]
        assert (r["adapted"], r["rejected"], r["next_c_bits"]) == (1, 0, iq.bits(-0.5))
        r = ir.model_run(ir.by_name(f"limit_c_beyond_n{n}"))[1][0]
        assert (r["adapted"], r["rejected"], r["next_c_bits"], r["c_bits"]) == (0, 1, iq.bits(2.0 ** -24), iq.bits(2.0 ** -24))
        s = iq.step(r, n, iq.Cfg(1.0, 0.0), 0.0, 1.0)  # (the same sums from c = 0 land on it; from 2^-24 on the next float)
        assert s["c"] == 0.5 and np.float32(np.float64(0.5) + np.float64(2.0 ** -24)) == ir.up(0.5)
        r = ir.model_run(ir.by_name(f"limit_d_on_n{n}"))[1][0]
        assert (r["adapted"], r["rejected"], r["next_d_bits"], r["next_c_bits"]) == (1, 0, two, 0)
        r = ir.model_run(ir.by_name(f"limit_d_beyond_n{n}"))[1][0]
        assert (r["adapted"], r["rejected"]) == (0, 1) and r["next_d_bits"] == r["d_bits"]
        assert np.float32(1.25 * np.float64(iq.from_bits(r["d_bits"]))) == ir.up(2.0)
        # the non-finite samples: counted as rule 2 says, and none reaches the tree
        ys, recs, zs, _ = ir.model_run(ir.by_name(f"extremes_n{n}"))
        assert all(not np.isfinite(y.view(np.float32)).all() for y in ys[1:]) and all(np.isfinite(z.view(np.float32)).all() for z in zs)
        assert np.isfinite(ys[0].view(np.float32)).all() and np.array_equal(_bits(ys[0]), _bits(zs[0]))
        # the fused quadruples: either contraction changes the sample
        c = ir.by_name(f"fused_n{n}")
        y = ir.model_run(c)[0][0].view(np.float32)[1::2]
        f0 = ir.fma_q(c.cfg.c0, c.cfg.d0, c.frames[0])
        assert f0[0] != y[0] or f0[15] != y[15]
    # every tie and its neighbours are in both arms
    c = ir.by_name("ties_n256")
    f = c.frames[0].view(np.float32)
    t = np.float32(2.5 / 256)
    for v in (t, ir.up(t), ir.down(t)):
        assert (f[0::2] == v).any() and (f[1::2] == v).any()


def test_records_chain_from_frame_to_frame():
    for c in ir.crafted():
        recs = ir.model_run(c)[1]
        assert (recs[0]["c_bits"], recs[0]["d_bits"]) == (iq.bits(c.cfg.c0), iq.bits(c.cfg.d0)), c.name
        for f in range(1, ir.N_FRAMES):
            assert (recs[f]["c_bits"], recs[f]["d_bits"]) == (recs[f - 1]["next_c_bits"], recs[f - 1]["next_d_bits"]), (c.name, f)
            assert recs[f]["adapted"] + recs[f]["rejected"] <= recs[f]["measured"], (c.name, f)


@pytest.mark.parametrize("n", ir.LENGTHS)
def test_convergence_is_a_newton_steps(n):
    """The tone of amplitude 40 with 37 + f whole cycles in frame f, offsets +0.7 / -0.3, Q arm 1.05 (q cos 3 deg + i sin 3 deg), no
    noise, mu = 1: the tone's bin over its mirror bin rises by at least 20 dB from frame 0 to frame 1 and is at least 80 dB on
    frame 2.  (Measured while writing, at every length: 28.9, 57.8 .. 57.9, then 110 to 129 dB: the error squares.)"""
    ys, recs = iq.run([ir.tone(n, f) for f in range(ir.N_FRAMES)], iq.Cfg(1.0, 0.0))
    db = [ir.image_ratio_db(y, f) for f, y in enumerate(ys)]
    print(n, [round(v, 1) for v in db])
    assert 28.0 < db[0] < 30.0  # (the 29 dB the header speaks of)
    assert db[1] >= db[0] + 20.0 and db[2] >= 80.0, db
    lv = iq.levels(recs[2])
    assert abs(lv["gain_imbalance"] - 1) < 1e-4 and abs(lv["phase_error"]) < 1e-4 and lv["image_rejection_db"] > 80.0
    lv = iq.levels(recs[0])  # (frame 0 ran at (0, 1): the front end's own figures, in ingest.adc_levels' terms)
    assert abs(lv["gain_imbalance"] - 1 / ir.GAIN) < 2e-3 and abs(lv["phase_error"] - math.radians(ir.PHASE_DEG)) < 2e-3
    assert 27.0 < lv["image_rejection_db"] < 31.0


@pytest.mark.parametrize("n", ir.LENGTHS)
def test_from_adc_levels_seeds_the_loop(n):
    """The pair that ingest.adc_levels' two figures imply, from the CS16 codes of frame 0, against the pair the loop converges to
    on the float frames.  The codes are the samples rounded to 1/256: an error of at most 1/512 a component, which moves a second
    moment of the tone (amplitude 40: variance 800) by at most 2 * 40 / 512 / 800 = 1.95e-4 of itself, and a ratio of two by
    twice that: 3.9e-4 is the tolerance.  (Measured while writing: 5e-7 to 1.3e-6 in c, 5e-7 to 9.2e-6 in d; the first step of the
    loop from (0, 1) is 1.3e-4 and 2.4e-3 away.)"""
    x0 = ir.tone(n, 0)
    codes = np.clip(np.rint(x0.view(np.float32).astype(np.float64) * 256), -32768, 32767).astype(np.int16)
    c0, d0 = iq.from_adc_levels(ingest.adc_levels(ar.model(codes, ingest.CS16)))
    assert iq.check_cfg(iq.Cfg(1.0, 0.0, c0, d0)) is None
    _, recs = iq.run([ir.tone(n, f) for f in range(ir.N_FRAMES)], iq.Cfg(1.0, 0.0))
    first = iq.from_bits(recs[0]["next_c_bits"]), iq.from_bits(recs[0]["next_d_bits"])
    conv = iq.from_bits(recs[3]["next_c_bits"]), iq.from_bits(recs[3]["next_d_bits"])
    print(n, (c0, d0), first, conv)
    tol = 2 * (2 * ir.AMP / 512) / (ir.AMP ** 2 / 2)
    assert abs(c0 - conv[0]) <= tol and abs(d0 - conv[1]) <= tol
    assert abs(c0 - conv[0]) < abs(first[0] - conv[0]) and abs(d0 - conv[1]) < abs(first[1] - conv[1])  # inside the first step's error
    # seeded with it, frame 0 is already where the unseeded loop is on frame 2
    y, _, _ = iq.apply(x0, iq.Cfg(1.0, 0.0, c0, d0))
    assert ir.image_ratio_db(y, 0) >= 80.0


MIRROR_N, MIRROR_K = 4096, 600


def mirror_tree() -> tp.Topology:
    """Two parent-less leaves of an eighth of the band at mirror frequencies, +-K cycles a frame; nibble payloads with scalecomp
    128, so that nothing saturates (blank_ref.effect_tree's scales)"""
    fs = 4 * MIRROR_N
    t = tp.Topology(fs=fs, frame=MIRROR_N, name="mirror")
    for name, sign in (("POS00", 1), ("NEG01", -1)):
        t.vfos.append(tp.VfoDesc(topic=name, parent=-1, fs=fs, decimate_count=3, mixer_freq=float(sign * 4 * MIRROR_K), demod_usb=False, cstyle=1,
                                 scalecomp=128, samples_per_buffer=MIRROR_N))
    return t


def mirror_frame(f: int) -> np.ndarray:
    """A carrier of amplitude 100 at +K cycles a frame, phase-continuous, in noise of sigma 1, through the tone's front end"""
    rng = np.random.default_rng(900 + f)
    j = np.arange(MIRROR_N) + f * MIRROR_N
    ph = 2 * np.pi * MIRROR_K * j / MIRROR_N
    i, q = 100.0 * np.cos(ph) + rng.standard_normal(MIRROR_N), 100.0 * np.sin(ph) + rng.standard_normal(MIRROR_N)
    a = np.deg2rad(ir.PHASE_DEG)
    x = np.empty(MIRROR_N, np.complex64)
    x.real = i + ir.OFF_I
    x.imag = ir.GAIN * (q * np.cos(a) + i * np.sin(a)) + ir.OFF_Q
    return x


def test_the_empty_mirror_leaf_goes_quiet_through_the_oracle():
    """The payoff: the carrier's leaf keeps its power, the leaf at the mirror frequency -- empty but for the image -- loses it.
    Measured while writing, payload power (mean square of the int8 payload) of the empty leaf without / with the stage: frame 1
    253.5 / 3.0, frame 2 252.0 / 1.9, frame 3 254.5 / 1.5 -- 19.2, 21.1 and 22.3 dB; the carrier's leaf 3481 either way.  Asserted
    on frames 2 and 3, 6 dB under the smaller of the two: 15.1 dB."""
    topo = mirror_tree()
    xs = [mirror_frame(f) for f in range(ir.N_FRAMES)]
    ys, recs = iq.run(xs, iq.Cfg(1.0, 0.0))
    trees = [ob.build_tree("port", topo) for _ in range(2)]
    for f in range(ir.N_FRAMES):
        p = []
        for (nodes, roots), x in zip(trees, (xs[f], ys[f])):
            ob.process_roots(roots, np.ascontiguousarray(x).view(np.float32))
            assert all(int(np.abs(nodes[i].iq().astype(np.int32)).max()) < 127 for i in range(2))  # nothing saturates
            p.append([float((nodes[i].iq().astype(np.float64) ** 2).mean()) for i in range(2)])
        print(f, p)
        (c_off, e_off), (c_on, e_on) = (sorted(v, reverse=True) for v in p)
        assert c_off > 10 * e_off  # one leaf holds the carrier, the other its image
        if f >= 2:
            assert 10 * math.log10(e_off / e_on) >= 15.1, (f, e_off, e_on)
            assert abs(10 * math.log10(c_on / c_off)) < 0.1
