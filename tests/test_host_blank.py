"""The blanker's host arithmetic (sdrreceiver_amd/csrc/sdrx_blank.h: the argument check, the bins' edges, the rank rule, the
threshold, the carry) against the model, through host/blank_check.cpp: built by host/Makefile with AddressSanitizer and
UndefinedBehaviorSanitizer, run as a stand-alone program in a child process -- no GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import blank_ref as br
from sdrreceiver_amd import blank as bl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("blank_check") / "blank_check"
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), f"BLANK_CHECK={out}", "BLANK_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all",
                           str(out)], stdout=subprocess.DEVNULL)
    return str(out)


def _run(exe, text="", args=()):
    r = subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "runtime error" not in r.stdout and "Sanitizer" not in r.stdout
    return r.stdout.splitlines()


def _record(cfg, n, hist, carry=None):
    lines = [f"cfg {cfg.ratio!r} {cfg.floor!r} {cfg.rank_q16} {cfg.guard}", f"n {n}"]
    lines += [f"bin {b} {int(c)}" for b, c in enumerate(hist) if c]
    if carry is not None:
        lines.append(f"carry {carry}")
    return "\n".join(lines + ["end"]) + "\n"


def test_geometry_is_the_models(exe):
    assert _run(exe, args=["--geometry"]) == [f"geometry {bl.LANE} {bl.TILE} {bl.WORKGROUP} {bl.HALO} {bl.BINS} {bl.MAX_BIN} {bl.MAX_GUARD}"]
    assert br.LENGTHS[-1] == bl.WORKGROUP + 272 and bl.WORKGROUP == 4 * bl.TILE and bl.HALO > bl.MAX_GUARD


def test_crafted_histograms_give_the_models_bin_and_threshold(exe):
    """Every frame of every crafted case: its histogram under its settings and the carry it started with"""
    text, want = "", []
    for c in br.crafted():
        st = bl.State()
        for f, x in enumerate(c.frames):
            hist = np.bincount(bl.bin_of(bl.power(x)), minlength=bl.BINS)
            _, rec, nxt = bl.apply(x, c.cfgs[f], st)
            text += _record(c.cfgs[f], c.n, hist, st.tail_gap)
            thr = bl.threshold(rec["next_ref_bin"], c.cfgs[f])
            want.append(f"ok {rec['next_ref_bin']} {bl.thr_bits(thr):08x} {bl.thr_bits(bl.edge(rec['next_ref_bin'])):08x} {rec['carry_in']}")
            st = nxt
    assert _run(exe, text) == want


def test_the_rank_at_equality_and_one_sample_fewer_and_the_extremes(exe):
    text, want = "", []
    for n in br.LENGTHS + (384000, 2 ** 31 - 16):
        for rank in (1, 32768, 65535, 65536):
            for low in {max(0, -(-rank * n // 65536) - 1), min(n, -(-rank * n // 65536)), 0, n}:
                hist = np.zeros(bl.BINS, np.int64)
                hist[7], hist[2047] = low, n - low
                cfg = bl.Cfg(1.0, 0.0, rank, 0)
                text += _record(cfg, n, hist)
                b = bl.rank_bin(hist, n, rank)
                assert b == (7 if 65536 * low >= rank * n else bl.MAX_BIN)
                want.append(f"ok {b} {bl.thr_bits(bl.threshold(b, cfg)):08x} {bl.thr_bits(bl.edge(b)):08x} 0")
    assert _run(exe, text) == want and {w.split()[1] for w in want} == {"7", str(bl.MAX_BIN)}


def test_bad_arguments_are_refused(exe):
    hist = np.zeros(bl.BINS, np.int64)
    hist[1016] = 256
    bad = [bl.Cfg(0.5, 0.0, 1, 0), bl.Cfg(float("inf"), 0.0, 1, 0), bl.Cfg(float("nan"), 0.0, 1, 0), bl.Cfg(2.0, -1.0, 1, 0),
           bl.Cfg(2.0, float("inf"), 1, 0), bl.Cfg(2.0, float("nan"), 1, 0), bl.Cfg(2.0, 0.0, 0, 0), bl.Cfg(2.0, 0.0, 65537, 0),
           bl.Cfg(2.0, 0.0, 1, -1), bl.Cfg(2.0, 0.0, 1, 65), bl.Cfg(1e39, 0.0, 1, 0)]  # (1e39 is inf in fp32)
    for c in bad:
        assert bl.check_cfg(c), c
    out = _run(exe, "".join(_record(c, 256, hist) for c in bad))
    assert len(out) == len(bad) and all(o.startswith("refused ") for o in out), out
    good = bl.Cfg(1.0, br.F32_MAX, 65536, 64)
    out = _run(exe, _record(good, 256, hist) + _record(good, 255, hist) + "cfg 2 0 1 0\nn 4\nbin 2048 4\nend\n" + "n 4\nbin 0 4\nend\n")
    assert out[0] == f"ok 1016 {bl.thr_bits(br.F32_MAX):08x} 3f800000 0" and [o.split()[0] for o in out[1:]] == ["refused"] * 3
