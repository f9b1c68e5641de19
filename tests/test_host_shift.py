"""The frequency shift's host arithmetic (sdrreceiver_amd/csrc/sdrx_shift.h: the tables, the conversion pair, the argument check,
the index split, the rotation, the frame advance) against the model, through host/shift_check.cpp: built by host/Makefile with
AddressSanitizer and UndefinedBehaviorSanitizer, run as a stand-alone program in a child process -- no GPU, nothing loaded into
Python."""
import os
import subprocess

import numpy as np
import pytest

import shift_ref as sr
from sdrreceiver_amd import shift as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("shift_check") / "shift_check"
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), f"SHIFT_CHECK={out}",
                           "SHIFT_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all", str(out)], stdout=subprocess.DEVNULL)
    return str(out)


def _run(exe, text="", args=()):
    r = subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "runtime error" not in r.stdout and "Sanitizer" not in r.stdout
    return r.stdout.splitlines()


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_geometry_and_tables_are_the_models(exe):
    assert _run(exe, args=["--geometry"]) == [f"geometry {sh.LANE} {sh.TILE} {sh.WORKGROUP} {sh.TAB}"]
    assert sr.LENGTHS[-1] == sh.WORKGROUP + 272 and sh.WORKGROUP == 4 * sh.TILE
    want = "tables " + " ".join(f"{int(b):08x}" for b in _u32(np.concatenate(sh.tables())))
    assert _run(exe, args=["--tables"]) == [want]


def test_the_conversion_pair(exe):
    rng = np.random.default_rng(8)
    pairs = [(2048000.0, 0.4), (2048000.0, -250000.0), (1e6, 5e5), (1e6, -5e5), (2.0 ** 32, 0.5), (2.0 ** 32, 1.5), (2.0 ** 32, -2.5), (48000.0, 0.0)]
    pairs += [(float(fs), float(rng.uniform(-fs / 2, fs / 2))) for fs in rng.uniform(1e3, 1e8, 300)]
    bad = [(0.0, 0.0), (-1.0, 0.0), ("nan", 0.0), ("inf", 0.0), (1e6, "nan"), (1e6, "inf"), (1e6, "-inf"), (1e6, 500000.1), (1e6, -500000.1)]
    text = "".join(f"inc {fs!r} {hz!r}\n" for fs, hz in pairs) + "".join(f"inc {fs} {hz}\n" for fs, hz in bad)
    assert _run(exe, text) == [f"inc {sh.inc_of(fs, hz):08x}" for fs, hz in pairs] + ["refused"] * len(bad)
    incs = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1] + [int(v) for v in rng.integers(0, 2 ** 32, 200)]
    out = _run(exe, "".join(f"hz 2048000.0 {v:08x}\nhz 30720 {v:08x}\n" for v in incs))
    want = [w for v in incs for w in (sh.hz_of(2048000.0, v), sh.hz_of(30720.0, v))]
    assert [float(o.split()[1]) for o in out] == want


def test_the_argument_check(exe):
    rows = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0), (2, 0, 0, 0, 0, 0), (3, 0, 0, 0, 0, 0), (0x80000000, 0, 0, 0, 0, 0), (2 ** 32, 0, 0, 0, 0, 0),
            (0, 1, 0, 0, 0, 0), (1, 0, 0, 0, 0, 7), (0, 0, 0, 9, 0, 0)]
    out = _run(exe, "".join("cfg " + " ".join(str(v) for v in r) + "\n" for r in rows))
    assert [o.split()[0] for o in out] == ["ok", "ok"] + ["refused"] * 7
    assert sh.check_cfg(sh.Cfg(0, 0, 1)) is None and sh.check_cfg(sh.Cfg(0, 0, 2)) and sh.check_cfg(sh.Cfg(0, 0, 3))


def test_every_crafted_frame_splits_rotates_and_advances_as_the_model(exe):
    """Every frame of every crafted case: the phase behind it, and the indices and the rotation of samples on either side of every
    boundary, of the wrap, and of a few hundred more"""
    rng = np.random.default_rng(10)
    text, want = "", []
    for c in sr.crafted():
        for rec in sr.model_run(c)[2]:
            n, ph, inc = rec["n_complex"], rec["phase"], rec["inc"]
            p = sh.phases(ph, inc, n)
            wraps = np.flatnonzero(np.diff(p.astype(np.int64)) < 0)[:4]
            js = sorted({0, n - 1} | {j for j in (6, 7, 15, 16, 1023, 1024, 4095, 4096) if j < n} | {int(j) + d for j in wraps for d in (0, 1)}
                        | {int(j) for j in rng.integers(0, n, 8)})
            text += f"frame {ph:08x} {inc:08x} {n} " + " ".join(str(j) for j in js) + "\n"
            h, m, l = sh.split(p[js])
            rot = sh.rotation(p[js])
            w = f"frame {rec['next_phase']:08x}"
            for k in range(len(js)):
                w += f" {int(p[js[k]]):08x} {int(h[k])} {int(m[k])} {int(l[k])} {int(_u32(rot[k: k + 1])[0]):08x} {int(_u32(rot[k: k + 1])[1]):08x}"
            want.append(w)
    # frames as long as they get, and an advance that wraps 2^31 times
    for ph, inc, n in ((0xFFFFFFFF, 0xFFFFFFFF, 2 ** 31 - 1), (5, 2 ** 31, 2 ** 31 - 1), (0x89ABCDEF, 0x9E3779B1, 384000)):
        text += f"frame {ph:08x} {inc:08x} {n}\n"
        want.append(f"frame {(ph + n * inc) % 2 ** 32:08x}")
    got = _run(exe, text)
    assert got == want


def test_samples_mix_as_the_model(exe):
    """Finite, zero, signed-zero and non-finite samples at phases that use every table entry"""
    rng = np.random.default_rng(14)
    x = np.concatenate([sr.crafted_samples(rng, 3000), sr.by_name("nonfinite_n256").frames[1][:200], sr.by_name("zeros_n256").frames[0][:40]])
    p = rng.integers(0, 2 ** 32, x.size).astype(np.uint32)
    p[:768] = np.concatenate([np.arange(256) << 24, (np.arange(256) << 16) | 0xAB000000, (np.arange(256) << 8) | 0x00CD0000]).astype(np.uint32)
    p[768] = p[769] = 0
    y = sh.cmul(x, sh.rotation(p))
    u = y.view(np.uint32)
    u[np.isnan(y.view(np.float32))] = sh.NAN_BITS
    xb = _u32(x)
    got = _run(exe, "".join(f"mix {int(xb[2 * k]):08x} {int(xb[2 * k + 1]):08x} {int(p[k]):08x}\n" for k in range(x.size)))
    assert got == [f"mix {int(u[2 * k]):08x} {int(u[2 * k + 1]):08x}" for k in range(x.size)]
    h, m, l = sh.split(p)
    assert set(h) == set(m) == set(l) == set(range(256))
