"""The detector leaves' host arithmetic (sdrreceiver_amd/csrc/sdrx_detect.h: the argument check, the envelope, the carrier sum, the
carrier, the AM and FM values in front of the int16 conversion, ANG) against the model, through host/detect_check.cpp: built by
host/Makefile with AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone program in a child process -- no GPU,
nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import detect_ref as dr
from sdrreceiver_amd import detect as dt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("detect_check") / "detect_check"
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), f"DETECT_CHECK={out}",
                           "DETECT_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all", str(out)], stdout=subprocess.DEVNULL)
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


def _f(x):
    return f"{int(_u32(np.float32(x).reshape(1))[0]):08x}"


def test_geometry_and_the_argument_check(exe):
    assert _run(exe, args=["--geometry"]) == [f"geometry {dr.BLOCK} 256"]
    rows = [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (3, 0, 0, 0), (-1, 0, 0, 0), (1, 1, 0, 0), (2, 0, 5, 0), (0, 0, 0, -7)]
    out = _run(exe, "".join("cfg " + " ".join(str(v) for v in r) + "\n" for r in rows))
    assert [o.split()[0] for o in out] == ["ok"] * 3 + ["refused"] * 5
    assert (dt.NONE, dt.AM, dt.FM) == (0, 1, 2)


def test_ang_on_its_axes_diagonals_and_a_grid(exe):
    rng = np.random.default_rng(21)
    v = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 3.0, -3.0, 1e-30, -1e-30, 1e-42, 3e38, -3e38, 2.0 ** -126]
    y, x = (np.array(a, np.float32).reshape(-1) for a in np.meshgrid(v, v))
    a = rng.uniform(-np.pi, np.pi, 4000)
    m = np.exp2(rng.uniform(-40, 40, 4000))
    y = np.concatenate([y, (m * np.sin(a)).astype(np.float32)])
    x = np.concatenate([x, (m * np.cos(a)).astype(np.float32)])
    got = _run(exe, "".join(f"ang {_f(p)} {_f(q)}\n" for p, q in zip(y, x)))
    want = dt.ang(y, x)
    assert got == [f"ang {_f(w)}" for w in want]
    assert dt.ang(0, 0) == 0 and dt.ang(0, -1) == 1 and dt.ang(1, 0) == 0.5 and dt.ang(-1, 0) == -0.5
    assert abs(float(dt.ang(1, 1)) - 0.25) < 1e-6 and dt.ang(-1, -1) == -(np.float32(1) - dt.ang(1, 1)) and dt.ang(np.float32(-0.0), -1) == 1
    assert np.all(np.abs(want) <= 1)


def test_every_crafted_frame_detects_as_the_model(exe):
    """Every frame of every crafted case through both detectors: S, the carrier and every value in front of the int16 conversion"""
    text, want = [], []
    for c in dr.crafted():
        zp = 0j
        for z in c.frames:
            words = _hex(_u32(z))
            e = dt.envelope(z)
            text.append(f"am {_f(c.gain_am)} {z.size} {words}")
            want.append(f"am {dt.carrier_sum(e)} {_f(dt.carrier(e))} " + _hex(_u32(dt.am_pre(z, c.gain_am))))
            text.append(f"fm {_f(c.gain_fm)} {_f(zp.real)} {_f(zp.imag)} {z.size} {words}")
            want.append("fm " + _hex(_u32(dt.fm_pre(z, c.gain_fm, zp))))
            zp = complex(z[-1])
    got = _run(exe, "\n".join(text) + "\n")
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, text[k][:40], [i for i, (a, b) in enumerate(zip(g.split(), w.split())) if a != b][:5])


def test_the_carrier_sum_at_its_cap_and_in_any_order(exe):
    """Envelopes at and above 2^15 count as 2^15 2^8; ties of e 2^8 go to the even integer; the sum does not depend on the order"""
    e = np.array([32768.0, 65536.0, 3e38, 0.001953125 * 1, 0.001953125 * 3, 0.001953125 * 5, 1.0 / 512 + 1.0 / 4096, 0.0], np.float32)
    z = e.astype(np.complex64)
    assert dt.carrier_sum(e) == 3 * 2 ** 23 + 0 + 2 + 2 + 1
    out = _run(exe, f"am {_f(1.0)} {z.size} {_hex(_u32(z))}\nam {_f(1.0)} {z.size} {_hex(_u32(z[::-1].copy()))}\n")
    assert out[0].split()[1] == out[1].split()[1] == str(dt.carrier_sum(e)) and out[0].split()[2] == _f(dt.carrier(e))
