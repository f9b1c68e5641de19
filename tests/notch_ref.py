"""What the spur canceller's tests share: the frame lengths, the crafted cases (four cf32 tree frames each, with their settings) and
the wrong devices as variants of a second writing of the model (sdrreceiver_amd.notch).

Frame lengths (`in_frame` = the tree's frame, no other stage): 255, 256, 1 023, 1 024, 4 095, 4 096, 4 097, 2 * 4 096 + 272, 3 * 4 096
and 4 * 4 096 + 16, each moved to the nearest length sdrx_finalize takes (tree_len: a multiple of 16 -- down for a length one short of
one, else up -- whose last chunk of 1 024 is empty or at least 256 samples).  They cover one lane short of a tile (1 008), one lane
short of a block (4 080), one block exactly, a short last block behind one, two and four full ones, fewer than two full blocks (no
frequency step) and enough blocks for one.

A frame is tones in complex Gaussian noise of unit power, generated in double with the phase running on across frames.  Hz are those
of a 1.536 MS/s tree: one Hz is 2^32 / 1 536 000 = 2 796.2 increment units, whatever rate the tiny test tree names."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import blank_ref as br
import shift_ref as sr
from sdrreceiver_amd import notch as nt, shift as sh

FS = 1536000.0
N_FRAMES = 4
M32 = nt.M32
L = nt.L
F32 = np.float32


def tree_len(n: int) -> int:
    """The nearest tree frame sdrx_finalize takes"""
    m = n - n % 16 if n % 16 == 15 else -(-n // 16) * 16
    if 0 < m % 1024 < 256:
        m += 256 - m % 1024
    return m


ASKED = (255, 256, 1023, 1024, 4095, 4096, 4097, 2 * L + 272, 3 * L, 4 * L + 16)
LENGTHS = tuple(dict.fromkeys(tree_len(n) for n in ASKED))
assert LENGTHS == (256, 1008, 1024, 4080, 4096, 4352, 8464, 12288, 16640)
SOME = (256, 4352, 16640)  # the lengths of the cases that do not turn on the frame's length: no full block, one, four and a short one

tree, integer_frames = br.tree, br.integer_frames


def hz(v: float) -> int:
    """Hz at 1.536 MS/s as a signed number of increment units"""
    return int(np.rint(v / FS * 4294967296.0))


@dataclasses.dataclass(frozen=True, eq=False)  # (hashed by identity: crafted() builds each once)
class Case:
    name: str
    n: int
    cfgs: tuple            # one nt.Cfg per frame; one that is another object than its predecessor is set in front of its frame
    frames: tuple          # N_FRAMES complex64 arrays of n samples (read-only)
    finite: bool = True    # False: NaN and Inf samples -- compared on the raw frame and the records only


def ro(x) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.complex64)
    x.setflags(write=False)
    return x


def signal(n: int, f: int, tones, seed: int, noise: float = 1.0) -> np.ndarray:
    """Frame f of n samples: tones [(amplitude, increment (any real number of units), phase in turns)] in noise of power noise^2"""
    rng = np.random.default_rng(52000 + 16 * seed + f)
    j = np.arange(f * n, (f + 1) * n, dtype=np.float64)
    x = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    for amp, inc, ph in tones:
        x = x + amp * np.exp(2j * np.pi * ((ph + j * (float(inc) / 4294967296.0)) % 1.0))
    return x.astype(np.complex64)


def frames_of(n, tones, seed, noise=1.0) -> list:
    return [signal(n, f, tones, seed, noise) for f in range(N_FRAMES)]


def cfg(inc0, mu=0.25, afc=1.0, coh=0.5, pull=hz(100.0), flags=0) -> nt.Cfg:
    return nt.Cfg(tuple(int(v) & M32 for v in inc0), mu, afc, coh, pull, flags)


BASE = hz(61234.5)                                   # where the single tone of most cases is given
EIGHT = tuple((hz(-200000.0) + k * nt.SPACING) & M32 for k in range(8))  # eight tones at the spacing limit
EIGHT_AMP = (30.0, 3.0, 12.0, 0.5, 20.0, 7.0, 1.0, 15.0)


@functools.lru_cache(maxsize=None)
def crafted() -> tuple:
    out = []

    def add(name, n, cfgs, frames, finite=True):
        cfgs = (cfgs,) * N_FRAMES if isinstance(cfgs, nt.Cfg) else tuple(cfgs)
        assert all(nt.check_cfg(c) is None for c in cfgs), name
        out.append(Case(f"{name}_n{n}", n, cfgs, tuple(ro(x) for x in frames), finite))

    for i, n in enumerate(LENGTHS):
        one = cfg([BASE])
        add("exact", n, one, frames_of(n, [(30.0, BASE, 0.1)], i))
        add("off20_afc1", n, one, frames_of(n, [(30.0, BASE + hz(20.0), 0.2)], 20 + i))
        add("off20_afc0", n, cfg([BASE], afc=0.0), frames_of(n, [(30.0, BASE + hz(20.0), 0.2)], 20 + i))
        tones = [(EIGHT_AMP[k], ((EIGHT[k] + 2 ** 31) % 2 ** 32 - 2 ** 31) + hz((-1) ** k * 3.0 * k), 0.11 * k) for k in range(8)]
        add("eight", n, cfg(EIGHT, pull=hz(50.0)), frames_of(n, tones, 40 + i))
    for i, n in enumerate(SOME):
        # a tone that is not there: the gate holds the increment
        add("absent", n, cfg([BASE], coh=0.9), frames_of(n, [], 60 + i))
        # 20 Hz off, but no more than 5 Hz may be pulled
        add("clamp", n, cfg([BASE], pull=hz(5.0)), frames_of(n, [(30.0, BASE + hz(20.0), 0.3)], 70 + i))
        add("clamp_down", n, cfg([BASE], pull=hz(5.0)), frames_of(n, [(30.0, BASE - hz(20.0), 0.3)], 70 + i))
        # a NaN and an Inf sample in frame 1: the tone's amplitude resets, rejected counts, the frames behind recover
        fr = frames_of(n, [(30.0, BASE, 0.4)], 80 + i)
        fr[1][n // 3] = complex(np.nan, 1.0)
        fr[1][n - 5] = complex(2.0, -np.inf)
        add("nonfinite", n, one, fr, finite=False)
        # a sample near the top of the fp32 range: a block sum overflows to Inf with no non-finite sample in the frame
        fr = frames_of(n, [(30.0, BASE, 0.4)], 80 + i)
        fr[2][7] = complex(3.0e38, 3.0e38)
        fr[2][9] = complex(3.0e38, 3.0e38)
        add("overflow", n, one, fr, finite=False)
        # a live change behind frame 1 keeps slot 0, replaces slot 1 and adds slot 2; behind frame 2 only mu changes
        t3 = [(30.0, BASE, 0.5), (10.0, hz(-300000.0), 0.6), (20.0, hz(250000.0), 0.7), (5.0, hz(5000.0), 0.8)]
        a = cfg([BASE, hz(-300000.0)])
        b = cfg([BASE, hz(250000.0), hz(5000.0)], afc=0.5)
        c = cfg([BASE, hz(250000.0), hz(5000.0)], mu=1.0, afc=0.5)
        add("change", n, (a, a, b, c), frames_of(n, t3, 90 + i))
        # SDRX_NOTCH_LOAD behind frame 1 with the same tones: every slot starts afresh
        ld = cfg([BASE, hz(-300000.0)], flags=nt.LOAD)
        add("load", n, (a, a, ld, ld), frames_of(n, t3[:2], 100 + i))
        # the phase passes 2^32 once inside every block (inc = 2^32 / 3000), resp. inside the frame of 256
        w = 2 ** 32 // (3000 if n > 256 else 100)
        add("wrap", n, cfg([w]), frames_of(n, [(30.0, w + hz(2.0), 0.9)], 110 + i))
        # inc0 = 0: a DC notch, the carrier 10 Hz above it; inc0 = 2^31: a tone at half the rate
        add("inc_zero", n, cfg([0]), frames_of(n, [(30.0, hz(10.0), 0.15)], 120 + i))
        add("inc_half", n, cfg([2 ** 31]), frames_of(n, [(30.0, 2 ** 31 - hz(10.0), 0.25)], 130 + i))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case_ids() -> list[str]:
    return [c.name for c in crafted()]


def by_name(name: str) -> Case:
    return next(c for c in crafted() if c.name == name)


@functools.lru_cache(maxsize=None)
def model_run(case: Case) -> tuple:
    """((the notched frames), (records)) of a crafted case under the model: computed once, read-only"""
    ys, recs = nt.run(case.frames, list(case.cfgs))
    for y in ys:
        y.setflags(write=False)
    return tuple(ys), tuple(recs)


# ---- wrong devices: each one thing a kernel or its launch code could get wrong ----------------------------------------------------
WRONG = ["fma_corr", "fma_subtract", "lanes_sequential", "waves_sequential", "used_after_update", "amplitude_not_carried", "phase_not_carried",
         "advance_padded", "advance_inc_next", "short_block_by_L", "short_block_in_S", "descending", "conj_dropped", "no_clamp", "no_gate",
         "step_in_frame", "no_reset"]
# the crafted case that catches each (tests/test_notch_model.py checks every one of these)
#   fma_corr: a fused product moves a term by an ulp of the term, which the ulp of a strong tone's block sum hides more often than
#   not -- the case with no tone, whose sums are small, shows it; waves_sequential needs a block with more than two waves
CAUGHT_BY = {"fma_corr": "absent_n4352", "fma_subtract": "exact_n4352", "lanes_sequential": "exact_n256", "waves_sequential": "exact_n4096",
             "used_after_update": "exact_n4352", "amplitude_not_carried": "exact_n256", "phase_not_carried": "exact_n256",
             "advance_padded": "exact_n1008", "advance_inc_next": "off20_afc1_n8464", "short_block_by_L": "exact_n4352",
             "short_block_in_S": "off20_afc1_n8464", "descending": "eight_n4352", "conj_dropped": "exact_n256", "no_clamp": "clamp_n16640",
             "no_gate": "absent_n16640", "step_in_frame": "off20_afc1_n8464", "no_reset": "nonfinite_n4352"}


def correlate_wrong(x, phase, inc, how) -> np.ndarray:
    """notch.correlate written out a second time, with one thing wrong"""
    n, nb = x.size, nt.blocks(x.size)
    rot = sh.rotation(sh.phases(phase, inc, n))
    t = np.zeros(nb * L, np.complex64)
    t[:n] = sr.cmul_wrong(x, rot if how == "conj_dropped" else np.conj(rot), "fma_re_first" if how == "fma_corr" else None)
    out = np.empty(nb, np.complex64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for part in ("real", "imag"):
            v = np.ascontiguousarray(getattr(t, part), dtype=F32).reshape(nb, 256, 16)
            lanes = np.zeros((nb, 256), F32)
            for j in range(16):
                lanes = lanes + v[:, :, j]
            waves = np.empty((nb, 4), F32)
            for w in range(4):
                u = [lanes[:, 64 * w + l] for l in range(64)]
                if how == "lanes_sequential":
                    acc = u[0]
                    for l in range(1, 64):
                        acc = acc + u[l]
                    waves[:, w] = acc
                else:
                    s = 1
                    while s < 64:
                        for l in range(0, 64, 2 * s):
                            u[l] = u[l] + u[l + s]
                        s *= 2
                    waves[:, w] = u[0]
            if how == "waves_sequential":
                setattr(out, part, ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3])
            else:
                setattr(out, part, (waves[:, 0] + waves[:, 1]) + (waves[:, 2] + waves[:, 3]))
    return out


def step_wrong(c, n, tone: nt.Tone, cfg: nt.Cfg, how) -> tuple:
    """notch.step written out a second time, with one thing wrong"""
    D = np.float64
    nb, nfull = nt.blocks(n), n // L
    mu, afc, coh = D(F32(cfg.mu)), D(F32(cfg.afc_gain)), D(F32(cfg.min_coherence))
    a = [F32(tone.a_re), F32(tone.a_im)]
    used = np.empty(nb, np.complex64)
    S = [D(0), D(0), D(0), D(0)]
    prev = [D(0), D(0)]
    rejected = 0
    last_in_s = nb if how == "short_block_in_S" else nfull
    with np.errstate(all="ignore"):
        for b in range(nb):
            lb = D(L if how == "short_block_by_L" else nt.block_len(n, b))
            m = [D(c[b].real) / lb, D(c[b].imag) / lb]
            new = [F32(D(a[i]) + mu * (m[i] - D(a[i]))) for i in range(2)]
            if not (np.isfinite(new[0]) and np.isfinite(new[1])) and how != "no_reset":
                new = [F32(0), F32(0)]
                rejected += 1
            hand = new if how == "used_after_update" else a
            used[b] = complex(hand[0], hand[1])
            if 1 <= b < last_in_s:
                S[0] = S[0] + (m[0] * prev[0] + m[1] * prev[1])
                S[1] = S[1] + (m[1] * prev[0] - m[0] * prev[1])
                S[2] = S[2] + (m[0] * m[0] + m[1] * m[1])
                d = [m[0] - D(hand[0]), m[1] - D(hand[1])]
                S[3] = S[3] + (d[0] * d[0] + d[1] * d[1])
            prev = m
            a = new
    inc = tone.inc
    inc_next, coherent, adapted, clamped = inc, 0, 0, 0
    if (nb if how == "short_block_in_S" else nfull) >= 2:
        coherent = int(bool(S[0] > 0 and S[0] >= coh * S[2]))
        if (coherent or how == "no_gate") and afc > 0:
            with np.errstate(all="ignore"):
                r = S[1] / S[0]
            r = D(1) if r > 1 else r
            r = r if r >= -1 else D(-1)
            inc_next, adapted = (inc + int(np.rint((afc * r) * D(nt.RAD_TO_INC)))) % 2 ** 32, 1
            off = (inc_next - tone.inc0 + 2 ** 31) % 2 ** 32 - 2 ** 31
            if abs(off) > cfg.max_pull and how != "no_clamp":
                inc_next, clamped = (tone.inc0 + (cfg.max_pull if off > 0 else -cfg.max_pull)) % 2 ** 32, 1
    bits = np.array(a, F32).view(np.uint32)
    rec = {"inc": inc, "inc_next": inc_next, "a_re_bits": int(bits[0]), "a_im_bits": int(bits[1]), "coherent": coherent, "adapted": adapted,
           "clamped": clamped, "rejected": rejected, "s_re": float(S[0]), "s_im": float(S[1]), "p": float(S[2]), "e": float(S[3])}
    steps = {"advance_padded": -(-n // sh.TILE) * sh.TILE}.get(how, n)
    nxt = (tone.phase + steps * (inc_next if how == "advance_inc_next" else inc)) % 2 ** 32
    return used, rec, nt.Tone(nxt, inc_next, tone.inc0, a[0], a[1])


def apply_wrong(x, cfg: nt.Cfg, state: nt.State, how) -> tuple:
    """notch.apply with one thing wrong; how = None is the definition itself (written out a second time)"""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    n = x.size
    y = x.copy()
    steps = []
    for tone in state.tones:
        if how == "amplitude_not_carried":
            tone = dataclasses.replace(tone, a_re=F32(0), a_im=F32(0))
        if how == "phase_not_carried":
            tone = dataclasses.replace(tone, phase=0)
        steps.append((tone,) + step_wrong(correlate_wrong(x, tone.phase, tone.inc, how), n, tone, cfg, how))
    for tone, used, rec, nxt in (reversed(steps) if how == "descending" else steps):
        q = sr.cmul_wrong(np.repeat(used, L)[:n], sh.rotation(sh.phases(tone.phase, nxt.inc if how == "step_in_frame" else tone.inc, n)),
                          "fma_im_second" if how == "fma_subtract" else None)
        with np.errstate(all="ignore"):
            y = (y.view(F32) - q.view(F32)).view(np.complex64)
    f = y.view(F32)
    f[np.isnan(f)] = np.array([nt.NAN_BITS], np.uint32).view(F32)[0]
    zero = dict.fromkeys(nt.TONE_FIELDS[:8], 0) | dict.fromkeys(nt.TONE_FIELDS[8:], 0.0)
    rec = {"frame": state.frame, "n_complex": n, "n_tones": cfg.n_tones, "blocks": nt.blocks(n),
           "tones": [s[2] for s in steps] + [dict(zero) for _ in range(nt.MAX - len(steps))]}
    return y, rec, nt.State(tuple(s[3] for s in steps), state.frame + 1)


def run_wrong(case: Case, how) -> tuple[list, list]:
    cur = case.cfgs[0]
    state, out, recs = nt.State.initial(cur), [], []
    for f, x in enumerate(case.frames):
        if f and case.cfgs[f] is not case.cfgs[f - 1]:
            state, cur = nt.load(state, cur, case.cfgs[f]), case.cfgs[f]
        y, rec, state = apply_wrong(x, cur, state, how)
        out.append(y)
        recs.append(rec)
    return out, recs


def same_run(a, b) -> bool:
    """Two (frames, records) runs with the same bits and the same figures"""
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[0], b[0])) and \
        [nt.record_key(r) for r in a[1]] == [nt.record_key(r) for r in b[1]]
