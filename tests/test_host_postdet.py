"""The post-detection filter's host arithmetic (sdrreceiver_amd/csrc/sdrx_postdet.h: the argument check, the Kaiser design, the FIR
with its history) against the model, through host/postdet_check.cpp: built by host/Makefile with AddressSanitizer and
UndefinedBehaviorSanitizer, run as a stand-alone program in a child process -- no GPU, nothing loaded into Python.  And the INI
keys post_decim, post_taps, post_cutoff_hz, post_atten_db through sdrx_demo's parser (--dump needs no GPU either)."""
import json
import os
import subprocess

import numpy as np
import pytest

import postdet_ref as pr
from sdrreceiver_amd import detect as dt, postdet as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("postdet_check") / "postdet_check"
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), f"POSTDET_CHECK={out}",
                           "POSTDET_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all", str(out)], stdout=subprocess.DEVNULL)
    return str(out)


def _run(exe, text="", args=()):
    r = subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "runtime error" not in r.stdout and "Sanitizer" not in r.stdout
    return r.stdout.splitlines()


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_limits_and_the_argument_check(exe):
    assert _run(exe, args=["--limits"]) == [f"limits {pd.MAX_TAPS} {pd.MAX_DECIM}"]
    rows = [(1, 1, 0, 0), (16, 256, 0, 0), (0, 0, 0, 0), (99, 0, 0, 0), (0, 64, 0, 0), (17, 64, 0, 0), (2, 257, 0, 0), (2, -1, 0, 0), (2, 64, 1, 0),
            (2, 64, 0, -3), (0, 0, 0, 1)]
    out = _run(exe, "".join("cfg " + " ".join(str(v) for v in r) + "\n" for r in rows))
    assert [o.split()[0] for o in out] == ["ok"] * 4 + ["refused"] * 7
    for (R, T, _, _), o in zip(rows[:2] + rows[4:8], out[:2] + out[4:8]):
        assert (pd.refusal(T, R) is None) == (o == "ok"), (R, T, o)


def test_the_design_is_the_model_s(exe):
    rows = [(fs, cut, N, A) for fs, cut in ((48000.0, 3000.0), (30720.0, 1500.0), (12000.0, 2999.5)) for N in (2, 17, 64, 129, 255, 256) for A in (50.5, 60.0, 120.0)]
    rows += [(48000.0, 3000.0, 1, 80.0), (48000.0, 300.0, 64, 80.0), (48000.0, 23900.0, 64, 80.0), (48000.0, 3000.0, 0, 80.0), (48000.0, 3000.0, 257, 80.0),
             (48000.0, 3000.0, 64, 50.0), (48000.0, 3000.0, 64, float("nan")), (0.0, 3000.0, 64, 80.0), (48000.0, -1.0, 64, 80.0)]
    out = _run(exe, "".join(f"design {fs!r} {cut!r} {N} {A!r}\n" for fs, cut, N, A in rows))
    assert len(out) == len(rows)
    fine = 0
    for (fs, cut, N, A), line in zip(rows, out):
        w = line.split()
        try:
            taps, info = pd.design(fs, cut, N, A)
        except ValueError:
            assert w[0] == "design" and w[1] in ("1", "2") and len(w) == 4, line
            continue
        assert w[1] == "0" and float.fromhex(w[2]) == info["pass_hz"] and float.fromhex(w[3]) == info["stop_hz"], line[:80]
        assert " ".join(w[4:]) == _hex(_u32(taps)), (fs, cut, N, A)
        fine += 1
    assert fine >= 30


def test_every_crafted_frame_filters_as_the_model(exe):
    """Every frame of every crafted case through both detectors' floats: every output and the history handed on, bit for bit"""
    text, want = [], []
    for c in pr.crafted():
        h = np.asarray(c.taps, np.float32)
        for kind in (dt.AM, dt.FM):
            det, hist = dt.State(), np.zeros(h.size - 1, np.float32)
            for f, z in enumerate(c.frames):
                pre = pd.pre_of(kind, z, pr.gain_of(c, kind, f), det)
                y, new = pd.fir(pre, h, c.decim, hist)
                text.append(f"fir {h.size} {c.decim} {_hex(_u32(h))} {_hex(_u32(hist))} {pre.size} {_hex(_u32(pre))}")
                want.append(("fir " + _hex(_u32(y)) + " | " + _hex(_u32(new))).replace("  ", " ").rstrip())
                hist = new
    got = _run(exe, "\n".join(text) + "\n")
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.rstrip() == w, (k, text[k][:40], [i for i, (a, b) in enumerate(zip(g.split(), w.split())) if a != b][:5])


def test_edges_of_the_fir(exe):
    """T = 1 (no history), the identity, R = 16, a frame shorter than the history, signed zeros, an infinity and a NaN"""
    f = np.float32
    rng = np.random.default_rng(5)
    cases = [((1.0,), 1, rng.standard_normal(32).astype(f)), ((0.75,), 16, rng.standard_normal(32).astype(f)),
             (pr.taps_random(256, 7), 16, rng.standard_normal(48).astype(f)), (pr.taps_random(64, 8), 3, rng.standard_normal(6).astype(f)),
             ((1.0, -1.0), 1, np.array([0.0, -0.0, np.inf, 1.0, np.nan, 2.0, -0.0, -0.0], f))]
    text, want = [], []
    for taps, R, pre in cases:
        h = np.asarray(taps, f)
        hist = rng.standard_normal(h.size - 1).astype(f)
        y, new = pd.fir(pre, h, R, hist)
        text.append(f"fir {h.size} {R} {_hex(_u32(h))} {_hex(_u32(hist))} {pre.size} {_hex(_u32(pre))}")
        want.append((_hex(_u32(y)), _hex(_u32(new))))
    got = _run(exe, "\n".join(text) + "\n")
    for g, (y, new) in zip(got, want):
        a, _, b = g[4:].partition("|")
        assert a.strip() == y and b.strip() == new, g[:80]
    assert want[0][0] == _hex(_u32(cases[0][2])), "T = 1, h = 1, R = 1 is the identity"


def test_the_ini_keys_through_the_cpp_front_door(tmp_path):
    from test_postdet_model import postfilter_ini
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "sdrx_demo"], stdout=subprocess.DEVNULL)
    demo = os.path.join(ROOT, "host", "sdrx_demo")
    text, topo = postfilter_ini()
    p = tmp_path / "postdet.ini"
    p.write_text(text)
    rows = [json.loads(l) for l in subprocess.check_output([demo, str(p), "--dump"], text=True).splitlines()]
    subs = {r["topic"]: r for r in rows if "sub_of" in r}
    assert rows[0]["n"] == len(topo.vfos)
    for v in topo.vfos:
        if v.parent < 0:
            continue
        r = subs[v.topic]
        assert (r["detector"], r["post_decim"], len(r["post_taps"])) == (v.detector, v.post_decim, len(v.post_taps)), v.topic
        assert np.array_equal(np.asarray(r["post_taps"], np.float32), np.asarray(v.post_taps, np.float32)), (v.topic, "the taps, bit for bit")
    assert len(subs["AIR01"]["post_taps"]) == 64 and subs["AIR01"]["post_decim"] == 6 and subs["POC01"]["post_taps"] == []
    for bad, what in ((text.replace("post_decim=6\n", ""), "all four keys or none"), (text.replace("post_decim=6", "post_decim=17"), "decim must be 1 .. 16"),
                      (text.replace("post_decim=6", "post_decim=7"), "not a multiple of decim"), (text.replace("post_taps=64", "post_taps=300"), "ntaps must be"),
                      (text.replace("post_cutoff_hz=3000", "post_cutoff_hz=100"), "does not fit"), (text.replace("detector=am", "out_rate=48000"), "detector=am|fm")):
        assert bad != text
        p.write_text(bad)
        r = subprocess.run([demo, str(p), "--dump"], capture_output=True, text=True)
        assert r.returncode == 1 and what in r.stderr, (what, r.stderr)
