"""The IQ balance correction's host arithmetic (sdrreceiver_amd/csrc/sdrx_iqbal.h: the argument check, the quantiser, the step)
against the model, through host/iq_check.cpp: built by host/Makefile with AddressSanitizer and UndefinedBehaviorSanitizer, run as
a stand-alone program in a child process -- no GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import iq_ref as ir
from sdrreceiver_amd import iqbal as iq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("iq_check") / "iq_check"
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), f"IQ_CHECK={out}", "IQ_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all",
                           str(out)], stdout=subprocess.DEVNULL)
    return str(out)


def _run(exe, text="", args=()):
    r = subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "runtime error" not in r.stdout and "Sanitizer" not in r.stdout
    return r.stdout.splitlines()


def _record(cfg, n, s, pair=None):
    lines = [f"cfg {cfg.mu!r} {cfg.min_power!r} {cfg.c0!r} {cfg.d0!r} {cfg.flags}"]
    if pair is not None:
        lines.append(f"pair {pair[0]:08x} {pair[1]:08x}")
    lines += [f"n {n}", "sums " + " ".join(str(s[k]) for k in iq.SUMS)]
    return "\n".join(lines + ["end"]) + "\n"


def _want(s, n, cfg, c, d):
    r = iq.step(s, n, cfg, c, d)
    return f"ok {r['measured']} {r['adapted']} {r['rejected']} {iq.bits(r['c']):08x} {iq.bits(r['d']):08x}"


def test_geometry_is_the_models(exe):
    assert _run(exe, args=["--geometry"]) == [f"geometry {iq.LANE} {iq.TILE} {iq.WORKGROUP} {iq.CLAMP}"]
    assert ir.LENGTHS[-1] == iq.WORKGROUP + 272 and iq.WORKGROUP == 4 * iq.TILE


def test_the_quantiser(exe):
    rng = np.random.default_rng(3)
    ks = rng.integers(-32770, 32770, 300)
    ties = ((ks + 0.5) / 256).astype(np.float32)
    vals = np.concatenate([ties, np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf)),
                           np.array([127.99, -127.99, 128, -128, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-30, 127.998046875], np.float32),
                           (rng.standard_normal(300) * 40).astype(np.float32)])
    text = "q " + " ".join(f"0x{int(b):08x}" for b in vals.view(np.uint32)) + "\n"
    assert _run(exe, text) == ["q " + " ".join(str(int(v)) for v in iq.quantise(vals))]
    assert _run(exe, "q 0.5 nan inf -inf -1e30\n") == ["q 128 0 32767 -32767 -32767"]


def test_crafted_sums_give_the_models_step(exe):
    """Every frame of every crafted case: its sums under its settings and the pair it ran with"""
    text, want = "", []
    for c in ir.crafted():
        for rec in ir.model_run(c)[1]:
            s = {k: rec[k] for k in iq.SUMS}
            text += _record(c.cfg, c.n, s, (rec["c_bits"], rec["d_bits"]))
            want.append(f"ok {rec['measured']} {rec['adapted']} {rec['rejected']} {rec['next_c_bits']:08x} {rec['next_d_bits']:08x}")
    got = _run(exe, text)
    assert got == want
    assert {w.split()[1:4] == ["1", "0", "1"] for w in want} == {True, False} and {w.split()[1] for w in want} == {"0", "1"}


def test_sums_near_two_to_the_61_and_min_power_on_either_side(exe):
    n = 2 ** 31 - 16
    full = 32767 * 32767
    assert n * full < 2 ** 61 and n * full > 2 ** 60
    text, want = "", []
    rng = np.random.default_rng(61)
    for k in range(40):
        # all but a few samples at the clamp in either arm, the rest spread: A, B of a few units from sums of 2^61
        s = {"sum_i": n * 32767 - int(rng.integers(0, 10 ** 9)), "sum_q": -n * 32767 + int(rng.integers(0, 10 ** 9)),
             "sum_iq": -n * full + int(rng.integers(0, 10 ** 14)), "sum_ii": n * full - int(rng.integers(0, 10 ** 3)), "sum_qq": n * full - int(rng.integers(0, 10 ** 3))}
        if k % 4 == 0:  # and uncentred, large variances
            s = {"sum_i": int(rng.integers(-10 ** 9, 10 ** 9)), "sum_q": int(rng.integers(-10 ** 9, 10 ** 9)), "sum_iq": int(rng.integers(-10 ** 17, 10 ** 17)),
                 "sum_ii": n * full - int(rng.integers(0, 10 ** 17)), "sum_qq": n * full - int(rng.integers(0, 10 ** 17))}
        for cfg in (iq.Cfg(1.0, 0.0), iq.Cfg(2.0 ** -8, 0.0, 0.25, 1.5), iq.Cfg(0.0, 0.0)):
            text += _record(cfg, n, s)
            want.append(_want(s, n, cfg, cfg.c0, cfg.d0))
        # min_power at (A + B) 2^-16 rounded to fp32, and the fp32 on either side: >= against a double holds or not as the model says
        A, B, _ = iq.moments(s, n)
        if A > 0 and B > 0:
            v = np.float32((A + B) * 2.0 ** -16)
            for mp in (v, ir.up(v), ir.down(v)):
                cfg = iq.Cfg(1.0, float(mp))
                text += _record(cfg, n, s)
                want.append(_want(s, n, cfg, 0.0, 1.0))
    # quotients that are not round: S_ii, S_qq about 2^60 over n = 2^31 - 16, a unit apart
    for d in (-1, 0, 1):
        s = {"sum_i": 0, "sum_q": 0, "sum_iq": d, "sum_ii": 2 ** 60 + d, "sum_qq": 2 ** 60 - d}
        A, B, _ = iq.moments(s, n)
        v = np.float32((A + B) * 2.0 ** -16)
        for mp in (v, ir.up(v), ir.down(v)):
            cfg = iq.Cfg(1.0, float(mp))
            text += _record(cfg, n, s)
            want.append(_want(s, n, cfg, 0.0, 1.0))
    got = _run(exe, text)
    assert got == want
    assert {w.split()[1] for w in want} == {"0", "1"} and any(w.split()[2] == "1" for w in want)


def test_bad_arguments_are_refused(exe):
    s = {"sum_i": 0, "sum_q": 0, "sum_iq": 0, "sum_ii": 256 * 65536, "sum_qq": 256 * 65536}
    bad = [iq.Cfg(-0.1, 0.0), iq.Cfg(1.1, 0.0), iq.Cfg(float("nan"), 0.0), iq.Cfg(0.5, -1.0), iq.Cfg(0.5, float("inf")), iq.Cfg(0.5, float("nan")),
           iq.Cfg(0.5, 0.0, 0.51), iq.Cfg(0.5, 0.0, -0.51), iq.Cfg(0.5, 0.0, float("nan")), iq.Cfg(0.5, 0.0, 0.0, 0.49), iq.Cfg(0.5, 0.0, 0.0, 2.01),
           iq.Cfg(0.5, 0.0, 0.0, float("nan")), iq.Cfg(0.5, 0.0, 0.0, 1.0, 2), iq.Cfg(0.5, 0.0, 0.0, 1.0, 3), iq.Cfg(0.5, 1e39), iq.Cfg(0.5, 0.0, 0.0, 1.0, 2 ** 32)]
    for c in bad[:-1]:
        assert iq.check_cfg(c), c
    out = _run(exe, "".join(_record(c, 256, s) for c in bad))
    assert len(out) == len(bad) and all(o.startswith("refused ") for o in out), out
    good = iq.Cfg(1.0, 3e38, -0.5, 2.0, iq.IQ_LOAD)
    over = dict(s, sum_ii=256 * 32767 * 32767 + 1)
    out = _run(exe, _record(good, 256, s) + _record(good, 0, s) + _record(good, 2 ** 31, s) + _record(good, 256, over) + _record(good, 256, dict(s, sum_i=256 * 32767 + 1))
               + _record(good, 256, s, (iq.bits(0.6), iq.bits(1.0))) + "n 4\nsums 0 0 0 4 4\nend\n" + "cfg 1 0 0 1 0\nn 4\nend\n")
    assert out[0] == f"ok 0 0 0 {iq.bits(-0.5):08x} {iq.bits(2.0):08x}" and [o.split()[0] for o in out[1:]] == ["refused"] * 7
