"""The spur canceller's host arithmetic (sdrreceiver_amd/csrc/sdrx_notch.h: the geometry, the argument check with the spacing rule,
the restart rule, the order of the block correlation's sums, the step rule of a tone over a frame's blocks, the subtraction) against
the model, through host/notch_check.cpp: built by host/Makefile with AddressSanitizer and UndefinedBehaviorSanitizer, run as a
stand-alone program in a child process -- no GPU, nothing loaded into Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import notch_ref as nr
from sdrreceiver_amd import notch as nt, shift as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("notch_check") / "notch_check"
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), f"NOTCH_CHECK={out}",
                           "NOTCH_FLAGS=-fsanitize=address,undefined -fno-sanitize-recover=all", str(out)], stdout=subprocess.DEVNULL)
    return str(out)


def _run(exe, text="", args=()):
    r = subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "runtime error" not in r.stdout and "Sanitizer" not in r.stdout
    return r.stdout.splitlines()


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _f(v) -> str:
    return f"{int(_u32(np.array([v], np.float32))[0]):08x}"


def _d(v) -> str:
    return "nan" if v != v else f"{struct.unpack('<Q', struct.pack('<d', v))[0]:016x}"


def _cfg_line(inc0=(1 << 24,), flags=0, pull=100, r0=0, mu=0.25, afc=1.0, coh=0.5, r1=0, n=None, res=(0,) * 8):
    slots = list(inc0) + [0] * (8 - len(inc0))
    return f"cfg {len(inc0) if n is None else n} {flags} {pull} {r0} {_f(mu)} {_f(afc)} {_f(coh)} {r1} " + " ".join(str(v) for v in slots) + " " + \
        " ".join(str(v) for v in res) + "\n"


def test_geometry_is_the_models(exe):
    assert _run(exe, args=["--geometry"]) == [f"geometry {nt.LANE} {sh.TILE} {nt.L} {nt.MAX} {nt.SPACING} {nt.RAD_TO_INC!r}"]
    assert nt.L == 4096 and nt.SPACING == 8 * 2 ** 32 // nt.L and nt.RAD_TO_INC == 2.0 ** 20 / (2 * np.pi) == 2.0 ** 32 / (2 * np.pi * nt.L)


def test_the_argument_check_and_the_spacing_rule(exe):
    S = nt.SPACING
    nan = float("nan")
    ok = [dict(), dict(mu=1.0, afc=0.0, coh=1.0, pull=2 ** 32 - 1), dict(inc0=()), dict(inc0=(1000, 1000 + S)), dict(inc0=(2 ** 32 - 100, S - 100)),
          dict(inc0=tuple(k * S for k in range(8))), dict(flags=1), dict(mu=1e-30, coh=1e-30), dict(inc0=(0, 2 ** 31))]
    bad = [dict(mu=0.0), dict(mu=-0.5), dict(mu=1.0000001), dict(mu=nan), dict(afc=-1e-9), dict(afc=1.0000001), dict(afc=nan), dict(coh=0.0), dict(coh=1.5),
           dict(coh=nan), dict(flags=2), dict(flags=3), dict(n=9), dict(inc0=(5, 7), n=1), dict(r0=1), dict(r1=1), dict(res=(0,) * 7 + (1,)),
           dict(inc0=(1000, 1000 + S - 1)), dict(inc0=(5, 5)), dict(inc0=(2 ** 32 - 100, S - 101)), dict(inc0=(0, 2 ** 32 - S + 1)),
           dict(inc0=tuple(k * S for k in range(7)) + (3 * S + 1,))]
    out = _run(exe, "".join(_cfg_line(**k) for k in ok + bad))
    assert [o.split()[0] for o in out] == ["ok"] * len(ok) + ["refused"] * len(bad), out
    for k in ok + bad:  # the model's check says the same wherever a Cfg can express the settings
        if not set(k) & {"n", "r0", "r1", "res"}:
            c = nt.Cfg(tuple(k.get("inc0", (1 << 24,))), k.get("mu", 0.25), k.get("afc", 1.0), k.get("coh", 0.5), k.get("pull", 100), k.get("flags", 0))
            assert (nt.check_cfg(c) is None) == (k in ok), k
    # every crafted case's settings pass; the pair inside the spacing limit is refused by both
    cfgs = {c for case in nr.crafted() for c in case.cfgs}
    out = _run(exe, "".join(_cfg_line(inc0=c.inc0, flags=c.flags, pull=c.max_pull, mu=c.mu, afc=c.afc_gain, coh=c.min_coherence) for c in cfgs))
    assert out == ["ok"] * len(cfgs)
    pair = nt.Cfg((nr.BASE, nr.BASE + nr.hz(1000.0)), 0.25, 1.0, 0.5, 100)  # 1 kHz = 2.7 bins apart
    assert nt.check_cfg(pair) and _run(exe, _cfg_line(inc0=pair.inc0))[0].startswith("refused")


def test_the_restart_rule_of_a_live_change(exe):
    text, want = "", []
    for case in nr.crafted():
        for f in range(1, nr.N_FRAMES):
            a, b = case.cfgs[f - 1], case.cfgs[f]
            if a is b:
                continue
            text += "restart " + " ".join(f"{c.n_tones} {c.flags} " + " ".join(str(v) for v in list(c.inc0) + [0] * (8 - c.n_tones)) for c in (a, b)) + "\n"
            st = nt.load(nt.State(tuple(nt.Tone(7, v, v, np.float32(1)) for v in a.inc0), 0), a, b)
            want.append(f"restart {sum(1 << k for k, t in enumerate(st.tones) if t.phase == 0)}")
    assert len(want) >= 9 and len(set(want)) >= 3  # (keep one and replace others; restart all; nothing but mu changes)
    assert _run(exe, text) == want


def test_the_order_of_the_sums_on_given_lane_sums(exe):
    """256 lane sums whose total depends on the order: the tree's, not a sequential sum's"""
    rng = np.random.default_rng(3)
    text, want, seq = "", [], []
    for _ in range(40):
        v = (rng.standard_normal(256) * np.exp2(rng.integers(-12, 12, 256))).astype(np.float32)
        text += "lanes " + " ".join(_f(x) for x in v) + "\n"
        w = v.reshape(4, 64).copy()
        d = 1
        while d < 64:
            w[:, 0::2 * d] = w[:, 0::2 * d] + w[:, d::2 * d]
            d *= 2
        want.append("lanes " + _f((w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])))
        acc = np.float32(0)
        for x in v:
            acc = np.float32(acc + x)
        seq.append("lanes " + _f(acc))
    assert _run(exe, text) == want and sum(a != b for a, b in zip(want, seq)) >= 20


def test_block_correlations_are_the_models(exe):
    """The first, a middle and the last (short) block of some crafted frames, and blocks that end inside a lane's neighbourhood"""
    text, want = "", []
    for name in ("exact_n256", "eight_n1008", "wrap_n4352", "inc_half_n16640", "nonfinite_n4352"):
        case = nr.by_name(name)
        x = case.frames[1]
        for k, inc in enumerate(case.cfgs[0].inc0[:2]):
            phase = 0x12345678 * (k + 1) & nt.M32
            c = nt.correlate(x, phase, inc)
            for b in sorted({0, nt.blocks(case.n) // 2, nt.blocks(case.n) - 1}):
                blk = x[b * nt.L: (b + 1) * nt.L]
                p0 = (phase + b * nt.L * inc) & nt.M32
                text += f"corr {p0:08x} {inc:08x} {blk.size} " + " ".join(f"{int(u):08x}" for u in _u32(blk)) + "\n"
                want.append("corr " + " ".join(f"{int(u):08x}" for u in _u32(c[b: b + 1])))
    got = _run(exe, text)
    def nan32(w):
        return len(w) == 8 and int(w, 16) & 0x7FFFFFFF > 0x7F800000

    same = [all(u == v or (nan32(u) and nan32(v)) for u, v in zip(a.split(), b.split())) for a, b in zip(got, want)]  # (a NaN sum: any NaN)
    assert len(got) == len(want) and all(same), [(a, b) for a, b in zip(got, want) if a != b][:3]
    assert any(nan32(w) for b in want for w in b.split()[1:])


def test_the_step_rule_on_every_crafted_case(exe):
    """Every tone of every frame of every crafted case: the block correlations the model found go in; the amplitudes handed to the
    blocks, S, P, E, inc_next, the flags and the state behind the frame come out"""
    text, want = "", []
    for case in nr.crafted():
        cur = case.cfgs[0]
        state = nt.State.initial(cur)
        for f, x in enumerate(case.frames):
            if f and case.cfgs[f] is not case.cfgs[f - 1]:
                state, cur = nt.load(state, cur, case.cfgs[f]), case.cfgs[f]
            nxt = []
            for tone in state.tones:
                c = nt.correlate(x, tone.phase, tone.inc)
                used, rec, t2 = nt.step(c, case.n, tone, cur)
                text += (f"step {case.n} {_f(cur.mu)} {_f(cur.afc_gain)} {_f(cur.min_coherence)} {cur.max_pull} {tone.phase:08x} {tone.inc:08x} {tone.inc0:08x} "
                         f"{_f(tone.a_re)} {_f(tone.a_im)} " + " ".join(f"{int(u):08x}" for u in _u32(c)) + "\n")
                want.append((f"step {t2.phase:08x} {t2.inc:08x} {_f(t2.a_re)} {_f(t2.a_im)} {tone.phase:08x} {tone.inc:08x} | {rec['inc']:08x} {rec['inc_next']:08x} "
                             f"{rec['a_re_bits']:08x} {rec['a_im_bits']:08x} {rec['coherent']} {rec['adapted']} {rec['clamped']} {rec['rejected']} "
                             f"{_d(rec['s_re'])} {_d(rec['s_im'])} {_d(rec['p'])} {_d(rec['e'])} | " + " ".join(f"{int(u):08x}" for u in _u32(used))))
                nxt.append(t2)
            state = nt.State(tuple(nxt), state.frame + 1)
    got = _run(exe, text)
    assert len(got) == len(want) > 500
    for a, b in zip(got, want):
        if "nan" in b:  # (a NaN double: any NaN)
            wa, wb = a.split(), b.split()
            assert len(wa) == len(wb) and all(u == v or (v == "nan" and int(u, 16) & 0x7fffffffffffffff > 0x7ff0000000000000) for u, v in zip(wa, wb)), (a, b)
        else:
            assert a == b
    flags = np.array([[int(v) for v in w.split("|")[1].split()[4:8]] for w in want])
    assert flags[:, 0].any() and not flags[:, 0].all() and flags[:, 1].any() and flags[:, 2].any() and flags[:, 3].any()


def test_samples_subtract_as_the_model(exe):
    rng = np.random.default_rng(21)
    y = np.concatenate([nr.sr.crafted_samples(rng, 2000), np.array([complex(np.nan, 1), complex(1, -np.inf), complex(np.inf, np.inf), 0j, complex(-0.0, -0.0)], np.complex64)])
    u = nr.sr.crafted_samples(rng, y.size)
    u[:50] = 0
    p = rng.integers(0, 2 ** 32, y.size).astype(np.uint32)
    q = sh.cmul(u, sh.rotation(p))
    with np.errstate(all="ignore"):
        out = (y.view(np.float32) - q.view(np.float32)).view(np.complex64)
    ob = out.view(np.uint32)
    ob[np.isnan(out.view(np.float32))] = nt.NAN_BITS
    yb, ub = _u32(y), _u32(u)
    got = _run(exe, "".join(f"sub {int(yb[2 * k]):08x} {int(yb[2 * k + 1]):08x} {int(ub[2 * k]):08x} {int(ub[2 * k + 1]):08x} {int(p[k]):08x}\n" for k in range(y.size)))
    assert got == [f"sub {int(ob[2 * k]):08x} {int(ob[2 * k + 1]):08x}" for k in range(y.size)]
