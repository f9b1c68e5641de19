"""What the IQ balance correction's tests share: the frame lengths, the crafted cases (four cf32 frames each, with their settings),
the imbalanced tone, the integer frames, and thirteen wrong devices as variants of the model (sdrreceiver_amd.iqbal).

Frame lengths: blank_ref's, the smallest that exercise k_iqbal's geometry -- 256 (less than a tile), 1296 (a tile plus 272), 4112
(four tiles plus the shortest last tile of 16; reached as blank_ref.rs_case reaches it, at the input rate of a 256/257 resampler)
and 4368, one workgroup plus 272.

The statistics are taken from the stage's output quantised to 1/256, so a crafted frame whose components lie on that grid has
sums one can write down; the pair after sdrx_finalize is (c0, d0) = (0, 1) unless the case says otherwise, and then Q' = Q."""
from __future__ import annotations

import dataclasses
import fractions
import functools

import numpy as np

import blank_ref as br
from sdrreceiver_amd import blank as bl, iqbal as iq

LENGTHS = br.LENGTHS
assert LENGTHS == (256, 1296, 4112, iq.WORKGROUP + 272)
N_FRAMES = 4
MU8 = 2.0 ** -8
NAN = np.float32(np.nan)
INF = np.float32(np.inf)

rs_case, tree, receiver_kw, behind = br.rs_case, br.tree, br.receiver_kw, br.behind


@dataclasses.dataclass(frozen=True, eq=False)  # (hashed by identity: crafted() builds each once)
class Case:
    name: str
    n: int
    cfg: iq.Cfg
    frames: tuple             # N_FRAMES complex64 arrays of n samples (read-only)
    blanker: object = None    # a bl.Cfg: the blanker behind the stage zeroes what the tree must not see (non-finite samples)


def ro(x) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.complex64)
    x.setflags(write=False)
    return x


def up(v) -> np.float32:
    return np.nextafter(np.float32(v), INF)


def down(v) -> np.float32:
    return np.nextafter(np.float32(v), -INF)


# ---- the imbalanced tone ----------------------------------------------------------------------------------------------------------
AMP, CYCLES, OFF_I, OFF_Q, GAIN, PHASE_DEG = 40.0, 37, 0.7, -0.3, 1.05, 3.0


def tone(n: int, f: int, noise: float = 0.0, seed: int = 0, dc: bool = True) -> np.ndarray:
    """A tone of amplitude 40 with 37 + f whole cycles in the frame through a front end with offsets +0.7 / -0.3 and the Q arm
    1.05 (q cos 3 deg + i sin 3 deg); `noise`: the sigma of Gaussian noise in front of the imbalance"""
    j = np.arange(n, dtype=np.float64)
    ph = 2 * np.pi * (CYCLES + f) * j / n
    i, q = AMP * np.cos(ph), AMP * np.sin(ph)
    if noise:
        rng = np.random.default_rng(5000 + 97 * seed + f)
        i, q = i + noise * rng.standard_normal(n), q + noise * rng.standard_normal(n)
    a = np.deg2rad(PHASE_DEG)
    x = np.empty(n, np.complex64)
    x.real = (i + (OFF_I if dc else 0.0)).astype(np.float32)
    x.imag = (GAIN * (q * np.cos(a) + i * np.sin(a)) + (OFF_Q if dc else 0.0)).astype(np.float32)
    return x


def on_grid(x) -> np.ndarray:
    """The frame with every component rounded to the statistics' grid of 1/256"""
    f = np.ascontiguousarray(x, dtype=np.complex64).view(np.float32)
    return (np.rint(f.astype(np.float64) * 256) / 256).astype(np.float32).view(np.complex64)


def image_ratio_db(y, f: int) -> float:
    """The tone's bin over its mirror bin, in dB"""
    s = np.fft.fft(np.asarray(y, dtype=np.complex128))
    k = CYCLES + f
    return float(20 * np.log10(abs(s[k]) / abs(s[-k])))


def boundaries(n) -> list[int]:
    """The last sample in front of every lane-row, tile and workgroup boundary the frame has (15 | 16, 1023 | 1024, 4095 | 4096)"""
    return [b - 1 for b in (iq.LANE, iq.TILE, iq.WORKGROUP) if b < n]


def pattern(n, kinds) -> np.ndarray:
    """Sample j is kinds[j % len(kinds)], an (I, Q) pair; len(kinds) divides 16, so it divides every frame"""
    assert 16 % len(kinds) == 0
    k = np.array(kinds, np.float32).view(np.complex64).reshape(-1)
    return np.tile(k, n // len(kinds))


@functools.lru_cache(maxsize=None)
def fused_differs(c, d, which: int) -> np.complex64:
    """A sample (I, Q) for which a fused product-sum differs from fl(fl(c I) + fl(d Q)): which = 0: fma(c, I, fl(d Q)); 1:
    fma(d, Q, fl(c I)).  Searched; the fused value is computed exactly (fractions) and the double it is rounded through is
    required to hold it exactly, so no second rounding hides in the search."""
    c, d = np.float32(c), np.float32(d)
    rng = np.random.default_rng(23 + which)
    F = fractions.Fraction
    for _ in range(200000):
        I, Q = np.float32(rng.uniform(-60, 60)), np.float32(rng.uniform(-60, 60))
        a, b = np.float32(c * I), np.float32(d * Q)
        plain = np.float32(a + b)
        exact = F(float(c)) * F(float(I)) + F(float(b)) if which == 0 else F(float(d)) * F(float(Q)) + F(float(a))
        if F(float(exact)) != exact:
            continue
        if np.float32(float(exact)) != plain:
            return np.complex64(complex(I, Q))
    raise AssertionError("no such sample")


def fma_q(c, d, x) -> np.ndarray:
    """Q' of a device that contracts: fma(c, I, fl(d Q)) through a double (exact for the samples fused_differs returns)"""
    f = np.ascontiguousarray(x, dtype=np.complex64).view(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        b = (np.float32(d) * f[1::2]).astype(np.float32)
        return (np.float64(np.float32(c)) * f[0::2].astype(np.float64) + b.astype(np.float64)).astype(np.float32)


def d0_landing(g: float, beyond: bool) -> float:
    """An fp32 d0 near 2 / g for which (float)(g (double)d0) is exactly 2 (beyond: the next float above 2)"""
    want = up(2.0) if beyond else np.float32(2.0)
    d = np.float32(2.0 / g)
    for _ in range(64):
        got = np.float32(np.float64(g) * np.float64(d))
        if got == want:
            return float(d)
        d = up(d) if got < want else down(d)
    raise AssertionError("no such d0")


BL_GUARD = bl.Cfg(4.0, 0.0, br.MEDIAN, 2)  # behind the stage in the cases with non-finite samples: each lies within 2 of a 1e30


@functools.lru_cache(maxsize=None)
def crafted() -> tuple:
    out = []
    for n in LENGTHS:
        tones = tuple(ro(tone(n, f)) for f in range(N_FRAMES))
        noisy = tuple(ro(tone(n, f, noise=6.0, seed=n)) for f in range(N_FRAMES))
        # mu = 0 (hold at a calibration), 2^-8, 1 (the Newton step) on the tone; with noise, so that every sample differs
        out.append(Case(f"tone_mu0_n{n}", n, iq.Cfg(0.0, 0.0, -0.05, 0.95), noisy))
        out.append(Case(f"tone_mu8_n{n}", n, iq.Cfg(MU8, 0.0), noisy))
        out.append(Case(f"tone_mu1_n{n}", n, iq.Cfg(1.0, 0.0), tones))
        # differing samples on either side of every boundary, and at 0 and n - 1: each its own large value, so a sample that is
        # skipped, read twice or taken from the neighbouring lane, tile or workgroup changes all five sums
        fr = []
        for f in range(N_FRAMES):
            x = tone(n, f, noise=1.0, seed=n + 1)
            at = sorted({0, n - 1} | set(boundaries(n)) | {b + 1 for b in boundaries(n)})
            for k, j in enumerate(at):
                x[j] = complex((-1) ** k * (90 + 3 * k + f), (-1) ** (k // 2) * (70 - 5 * k - f))
            fr.append(ro(x))
        out.append(Case(f"bounds_n{n}", n, iq.Cfg(MU8, 0.0), tuple(fr)))
        # components at q's ties (k + 1/2) / 256, and one float above and below: held at (0, 1), so Q' = Q and both arms show them
        ks = [0, 1, 2, 7, 255, 256, 10000, 32765, 32766, -1, -2, -3, -8, -256, -257, -32766, -32767]
        vals = []
        for k in ks:
            t = np.float32((k + 0.5) / 256)
            vals += [t, up(t), down(t)]
        fr = []
        for f in range(N_FRAMES):
            x = on_grid(tone(n, f)).copy()
            v = x.view(np.float32)
            for m, t in enumerate(vals):
                v[2 * (20 + m + f)] = t                            # I
                v[2 * (n - 20 - m - f) + 1] = vals[len(vals) - 1 - m]  # Q
            fr.append(ro(x))
        out.append(Case(f"ties_n{n}", n, iq.Cfg(0.0, 0.0), tuple(fr)))
        # +-127.99, +-128 (frame 0: finite, the blanker behind has no reference yet), then 1e30, +-inf and NaN in either arm, each
        # between two samples of 1e30 that the blanker behind hits: with its guard of 2 the tree sees zeros there
        x0 = tone(n, 0).copy()
        for m, z in enumerate([127.99 + 128j, -127.99 - 128j, 128 - 127.99j, -128 + 127.99j]):
            x0[(40 + 100 * m) % n] = z
        fr = [ro(x0)]
        big = np.complex64(complex(1e30, 1.0))
        odd = [complex(NAN, 1.0), complex(2.0, NAN), complex(INF, -3.0), complex(-INF, 3.0), complex(4.0, INF), complex(5.0, -INF), complex(NAN, NAN),
               complex(-1e30, 1e30), complex(1e30, -1e30)]
        for f in range(1, N_FRAMES):
            x = tone(n, f).copy()
            for m, z in enumerate(odd):
                j = (30 + 23 * m + 7 * f) % (n - 8) + 2
                x[j - 1], x[j], x[j + 1] = big, z, big
            x[0], x[1], x[2] = big, odd[f], big  # (and at the frame's start)
            fr.append(ro(x))
        out.append(Case(f"extremes_n{n}", n, iq.Cfg(MU8, 0.0), tuple(fr), BL_GUARD))
        # every component at the clamp: the largest per-thread and per-workgroup sums (S_ii = S_qq = S_iq = n 32767^2), A = 0; then
        # the Q arm at the other clamp (S_iq = -n 32767^2); then the tone
        fr = (ro(np.full(n, 200 + 200j, np.complex64)), ro(np.full(n, 200 - 200j, np.complex64)), tones[2], tones[3])
        out.append(Case(f"clamp_n{n}", n, iq.Cfg(1.0, 0.0), fr))
        # (A + B) 2^-16 equal to min_power: I, Q = +-1 gives A = B = 65536 and exactly 2.0 -- measured; the tone's 1600 or so is
        # far above, an arm of +-0.5 gives 0.5: not measured
        eq = pattern(n, [(1, 1), (-1, 1), (1, -1), (-1, -1)])
        low = pattern(n, [(0.5, 0.5), (-0.5, 0.5), (0.5, -0.5), (-0.5, -0.5)])
        out.append(Case(f"minpower_eq_n{n}", n, iq.Cfg(1.0, 2.0), (ro(eq), ro(low), ro(eq), tones[3])))
        # ... and just below it.  The double next below 2.0 is out of reach: the sums are integers, and sum / n takes few bit patterns
        # at these n (none at all at 256, a power of two), so no frame lands on it -- a search over two samples' 2^32 values found
        # none.  The nearest a frame comes: one sample of the same frame one LSB lower, (A + B) 2^-16 = 2 - 511 / (65536 n) or so.
        # Not measured; host/iq_check.cpp is held to the rule on sums as close as doubles get (tests/test_host_iq.py).
        below = eq.copy()
        below[8] = complex(255 / 256, 1)
        out.append(Case(f"minpower_below_n{n}", n, iq.Cfg(1.0, 2.0), (ro(below), ro(eq), ro(below), tones[3])))
        # an all-zero frame (A = 0), then live ones; a Q arm of zeros (B = 0), then live ones
        zero = np.zeros(n, np.complex64)
        out.append(Case(f"zero_then_live_n{n}", n, iq.Cfg(1.0, 0.0), (ro(zero), tones[1], tones[2], ro(zero))))
        noq = tones[0].copy()
        noq.imag = 0
        out.append(Case(f"q_zero_n{n}", n, iq.Cfg(1.0, 0.0), (ro(noq), tones[1], ro(noq), tones[3])))
        # a step that lands exactly on c = 0.5: three quarters of the samples (v, -v), a quarter (v, v): A = B, C = -A / 2, so
        # ep = -1/2, g = 1 and c_next = c + 1/2.  From c0 = 0: 0.5, taken.  From c0 = 2^-24 (which moves no quantised sample): the next
        # float beyond, refused.  The same below zero with the Q arm mirrored.
        land = pattern(n, [(1, -1), (-1, 1), (1, -1), (-1, -1), (-1, 1), (1, -1), (-1, 1), (1, 1)])
        for name, c0, x in (("limit_c_on", 0.0, land), ("limit_c_beyond", 2.0 ** -24, land), ("limit_c_on_neg", 0.0, np.conj(land)),
                            ("limit_c_beyond_neg", -2.0 ** -24, np.conj(land))):
            out.append(Case(f"{name}_n{n}", n, iq.Cfg(1.0, 0.0, c0, 1.0), (ro(x), tones[1], ro(x), tones[3])))
        # ... and on d = 2: I = +-1 on ten samples of sixteen, Q' = +-1 on six, uncorrelated and without DC: A = 5/8, B = 3/8 of 65536, eg = 1/4,
        # g = 5/4, d_next = (float)(1.25 d0) = 2 for d0 about 1.6 -- the Q arm comes in as +-0.625, which d0 brings within a
        # thousandth of an LSB of +-1
        for name, beyond in (("limit_d_on", False), ("limit_d_beyond", True)):
            d0 = d0_landing(1.25, beyond)
            q_in = float(np.float32(1.0 / d0))
            x = pattern(n, [(1, q_in), (-1, q_in), (1, -q_in), (-1, -q_in), (1, 0), (-1, 0), (1, 0), (-1, 0), (1, 0), (-1, 0), (0, q_in), (0, -q_in),
                            (0, 0), (0, 0), (0, 0), (0, 0)])
            out.append(Case(f"{name}_n{n}", n, iq.Cfg(1.0, 0.0, 0.0, d0), (ro(x), tones[1], ro(x), tones[3])))
        # a quadruple c, I, d, Q for which either fused product-sum differs from rule 1: held at a calibration
        c0, d0 = float(np.float32(-0.0523)), float(np.float32(0.9537))
        fr = []
        for f in range(N_FRAMES):
            x = tone(n, f).copy()
            for m, j in enumerate([0, 15, 16, n // 2, n - 1]):
                x[j] = fused_differs(c0, d0, (m + f) % 2)
            fr.append(ro(x))
        out.append(Case(f"fused_n{n}", n, iq.Cfg(0.0, 0.0, c0, d0), tuple(fr)))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case_ids() -> list[str]:
    return [c.name for c in crafted()]


def by_name(name: str) -> Case:
    return next(c for c in crafted() if c.name == name)


@functools.lru_cache(maxsize=None)
def model_run(case: Case) -> tuple:
    """((corrected frames), (records), (the frames behind the blanker, if the case has one), (the tree's raw frames)) of a crafted
    case under the model: computed once, read-only"""
    ys, recs = iq.run(case.frames, case.cfg)
    zs = list(ys)
    if case.blanker is not None:
        zs, _ = bl.run(ys, case.blanker)
    raws, hist = [], None
    for y, z in zip(ys, zs):
        y.setflags(write=False)
        z.setflags(write=False)
        raw, hist = behind(case.n, z, hist)
        raw.setflags(write=False)
        raws.append(raw)
    return tuple(ys), tuple(recs), tuple(zs), tuple(raws)


# ---- integer frames ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def integer_frames(fmt: int, n: int, seed: int = 0, frames: int = N_FRAMES) -> tuple:
    """Frames of n integer samples in format `fmt`: the imbalanced tone (offsets included: worth removing) with noise of sigma 4
    dongle LSB, as a direct-conversion front end delivers it"""
    from sdrreceiver_amd import ingest
    scale, lo, hi, dt, mid = {ingest.CU8: (1, 0, 255, np.uint8, 127), ingest.CS8: (1, -128, 127, np.int8, 0),
                              ingest.CS16: (256, -32768, 32767, np.int16, 0)}[fmt]
    out = []
    for f in range(frames):
        x = tone(n, f, noise=4.0, seed=1000 + 13 * fmt + seed).view(np.float32).astype(np.float64)
        v = np.clip(np.rint(x * scale) + mid, lo, hi).astype(dt)
        v.setflags(write=False)
        out.append(v)
    return tuple(out)


# ---- wrong devices: each one thing a kernel could get wrong ---------------------------------------------------------------------
WRONG = ["fma", "stats_of_input", "q_truncates", "q_without_clamp", "means_not_subtracted", "new_pair_same_frame", "c_without_g", "step_in_fp32",
         "padding_counted", "partial_sums_32bit", "siq_of_magnitudes", "min_power_strict", "rejected_step_clamps"]
# the crafted case that catches each (tests/test_iq_model.py checks every one of these)
CAUGHT_BY = {"fma": "fused_n256", "stats_of_input": "tone_mu1_n256", "q_truncates": "ties_n256", "q_without_clamp": "clamp_n256",
             "means_not_subtracted": "tone_mu1_n1296", "new_pair_same_frame": "tone_mu1_n256", "c_without_g": "tone_mu1_n4368",
             "step_in_fp32": "tone_mu1_n4368", "padding_counted": "tone_mu1_n4112", "partial_sums_32bit": "clamp_n4368",
             "siq_of_magnitudes": "tone_mu1_n256", "min_power_strict": "minpower_eq_n1296", "rejected_step_clamps": "limit_c_beyond_n256"}


def _wrap32(v: int, signed: bool) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if signed and v >= 1 << 31 else v


def apply_wrong(x, cfg: iq.Cfg, state: iq.State, how) -> tuple:
    """iqbal.apply with one thing wrong; how = None is the definition itself (written out a second time)"""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    n = x.size
    D = np.float64

    def corrected(c, d):
        y = x.copy()
        f, g = x.view(np.float32), y.view(np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            if how == "fma":
                q = fma_q(c, d, x)
            else:
                q = np.float32(c) * f[0::2] + np.float32(d) * f[1::2]
        q = q.astype(np.float32)
        q[np.isnan(q)] = np.array([iq.NAN_BITS], np.uint32).view(np.float32)[0]
        g[1::2] = q
        return y

    def quant(v):
        with np.errstate(over="ignore", invalid="ignore"):
            w = v.astype(np.float32) * np.float32(256)
        w = np.where(np.isnan(w), np.float32(0), w)
        w = np.clip(w, -(2.0 ** 24), 2.0 ** 24) if how == "q_without_clamp" else np.clip(w, -iq.CLAMP, iq.CLAMP)  # (2^24: some 32-bit conversion)
        return (np.trunc(w) if how == "q_truncates" else np.rint(w)).astype(np.int64)

    def stats(y):
        f = (x if how == "stats_of_input" else y).view(np.float32)
        qi, qq = quant(f[0::2]), quant(f[1::2])
        terms = [qi, qq, np.abs(qi) * np.abs(qq) if how == "siq_of_magnitudes" else qi * qq, qi * qi, qq * qq]
        if how == "partial_sums_32bit":  # a workgroup's sums kept in 32 bits, the workgroups added in 64
            tot = []
            for k, t in enumerate(terms):
                tot.append(sum(_wrap32(int(t[b: b + iq.WORKGROUP].sum()), k < 3) for b in range(0, n, iq.WORKGROUP)))
        else:
            tot = [int(t.sum()) for t in terms]
        return dict(zip(iq.SUMS, tot))

    def step(s, c, d):
        c, d, mu = np.float32(c), np.float32(d), np.float32(cfg.mu)
        out = {"measured": 0, "adapted": 0, "rejected": 0, "c": float(c), "d": float(d)}
        T = np.float32 if how == "step_in_fp32" else D
        N = T(-(-n // iq.TILE) * iq.TILE if how == "padding_counted" else n)
        with np.errstate(over="ignore", invalid="ignore"):
            mi, mq = T(s["sum_i"]) / N, T(s["sum_q"]) / N
            if how == "means_not_subtracted":
                mi, mq = T(0), T(0)
            A, B, C = T(s["sum_ii"]) / N - mi * mi, T(s["sum_qq"]) / N - mq * mq, T(s["sum_iq"]) / N - mi * mq
            p = (A + B) * T(2.0 ** -16)
            enough = p > T(np.float32(cfg.min_power)) if how == "min_power_strict" else p >= T(np.float32(cfg.min_power))
            if not (A > 0 and B > 0 and enough):
                return out
            out["measured"] = 1
            if not mu > 0:
                return out
            m = T(mu)
            ep, eg = C / A, (A - B) / (A + B)
            g = T(1) + m * eg
            cn = np.float32((T(c) - m * ep) if how == "c_without_g" else g * (T(c) - m * ep))
            dn = np.float32(g * T(d))
        if iq.pair_ok(cn, dn):
            out.update(adapted=1, c=float(cn), d=float(dn))
        elif how == "rejected_step_clamps" and np.isfinite(cn) and np.isfinite(dn):
            out.update(rejected=1, c=float(np.clip(cn, -iq.MAX_C, iq.MAX_C)), d=float(np.clip(dn, iq.MIN_D, iq.MAX_D)))
        else:
            out["rejected"] = 1
        return out

    y = corrected(state.c, state.d)
    s = stats(y)
    r = step(s, state.c, state.d)
    if how == "new_pair_same_frame":
        y = corrected(r["c"], r["d"])
    rec = {"frame": state.frame, "n_complex": n, "measured": r["measured"], "adapted": r["adapted"], "rejected": r["rejected"], "c_bits": iq.bits(state.c),
           "d_bits": iq.bits(state.d), "next_c_bits": iq.bits(r["c"]), "next_d_bits": iq.bits(r["d"]), **s}
    return y, rec, iq.State(r["c"], r["d"], state.frame + 1)


def run_wrong(frames, cfg, how) -> tuple[list, list]:
    state, out, recs = iq.State.initial(cfg), [], []
    for x in frames:
        y, rec, state = apply_wrong(x, cfg, state, how)
        out.append(y)
        recs.append(rec)
    return out, recs


def same_run(a, b) -> bool:
    """Two (frames, records) runs with the same bits and the same figures"""
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[0], b[0])) and list(a[1]) == list(b[1])  # (b may hold more)
