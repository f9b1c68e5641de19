"""What the impulse blanker's tests share: the frame lengths, the crafted cases (three cf32 frames each, with their settings),
the noise-and-pulse run, and twelve wrong devices as variants of the model (sdrreceiver_amd.blank).

Frame lengths: the smallest that exercise k_blank's geometry -- 256 (less than a tile: the shortest frame sdrx_finalize takes),
1296 (a tile plus 272), 4112 (four tiles plus the shortest last tile of 16) and one workgroup plus 272, which crosses the
workgroup boundary (blank.WORKGROUP = 4096 samples).

A crafted frame is a background of unit power (bin 1016, whose lower edge is 1.0) with a few samples of another power, so with
ratio 4 and the median the threshold of frames 1 and 2 is exactly 4.0 unless the case says otherwise; frame 0 always runs at
thr = +inf and only sets the reference."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import resample_ref as rr
from sdrreceiver_amd import blank as bl

LENGTHS = (256, 1296, 4112, bl.WORKGROUP + 272)
GUARDS = (0, 1, 16, 17, 64)
N_FRAMES = 3
MEDIAN = 32768
F32_MAX = float(np.finfo(np.float32).max)


# 4112 is no frame a tree takes (sdrx_finalize wants a last chunk of 256 samples at the least), so a frame with a last tile of 16
# reaches the blanker the one way it can: at the input rate of a resampler, here 257 -> 256 with 8 taps per phase, whose tree has 4096
RS_4112 = (256, 257, 8, 4112, 4096)


def rs_case(n: int):
    """The resample_ref case a frame length needs behind the blanker, or None"""
    return RS_4112 if n == 4112 else None


def tree(n: int):
    """front_ref's tiny tree for frames of n at the blanker: a main with a USB and a compress sub, and a parent-less compress leaf"""
    return rr.tree(rs_case(n) or (1, 1, 8, n, n))


def receiver_kw(n: int) -> dict:
    """The Receiver arguments tree(n) needs beside the blanker's"""
    c = rs_case(n)
    return dict(input_rate=rr.rates(c)[0], resample_taps=rr.random_taps(c)) if c else {}


def behind(n: int, y, hist=None):
    """(the tree's raw frame, the resampler's history) for the blanker's output frame y"""
    from sdrreceiver_amd import resample as rs
    c = rs_case(n)
    if not c:
        return y, None
    return rs.apply(y, rr.random_taps(c), c[0], c[1], hist)


def effect_tree(n: int):
    """The same tree at frame length n (the oracle takes any) with leaf scales at which the noise-and-pulse run saturates no payload, so that a payload's error is a measure of the
    error in front of it: the USB leaf's gain 0.05 / 128, and both compress leaves in the nibble format with scalecomp 128 (an
    int8 then holds the chain's +-128; the 8-bit format has no scale and clips at +-1)"""
    from sdrreceiver_amd import topology as tp
    t = rr.tree((1, 1, 8, n, n))
    for i, v in enumerate(t.vfos):
        if v.demod_usb:
            v.gain = tp._g(0.05 / 128)
        elif not t.children(i):
            v.cstyle, v.scalecomp = 1, 128
    return t


@dataclasses.dataclass(frozen=True, eq=False)  # (hashed by identity: crafted() builds each once)
class Case:
    name: str
    n: int
    cfgs: tuple      # one bl.Cfg per frame
    frames: tuple    # N_FRAMES complex64 arrays of n samples (read-only)

    @property
    def guard(self) -> int:
        return self.cfgs[0].guard


# ---- samples of an exact power ------------------------------------------------------------------------------------------------
def sample_of_power(p) -> np.complex64:
    """A cf32 sample whose model power is exactly the float p (searched: re = sqrt(p) rounded, a small im to land on p)"""
    p = np.float32(p)
    re0 = np.float32(np.sqrt(np.float64(p)))
    for re in (re0, np.nextafter(re0, np.float32(0)), np.nextafter(re0, np.float32(np.inf))):
        for k in range(0, 4000):
            im = np.float32(np.sqrt(np.float64(p)) * 1e-5 * k)
            z = np.complex64(complex(re, im))
            if bl.power(np.array([z]))[0] == p:
                return z
    raise AssertionError(f"no sample of power {p!r}")


@functools.lru_cache(maxsize=None)
def fused_differs(thr) -> np.complex64:
    """A sample whose power is exactly thr (no hit) where fma(re, re, fl(im im)) gives the next float above (a hit): searched"""
    thr = np.float32(thr)
    rng = np.random.default_rng(11)
    for _ in range(200000):
        re = np.float32(rng.uniform(0.3, 0.95) * np.sqrt(float(thr)))
        im = np.float32(np.sqrt(float(thr) - float(re) ** 2))
        z = np.complex64(complex(re, im))
        fused = np.float32(float(re) * float(re) + float(np.float32(im * im)))
        if bl.power(np.array([z]))[0] == thr and fused == up(thr):
            return z
    raise AssertionError("no such sample")


def up(p) -> np.float32:
    return np.nextafter(np.float32(p), np.float32(np.inf))


def down(p) -> np.float32:
    return np.nextafter(np.float32(p), np.float32(0))


def background(n, amp=1.0) -> np.ndarray:
    """Unit power with every sample another phase pattern (a wrong index shows): (+-amp, 0) and (0, +-amp) in a fixed order"""
    j = np.arange(n)
    x = np.zeros(n, np.complex64)
    x.real = np.where(j % 4 == 0, amp, np.where(j % 4 == 2, -amp, 0)).astype(np.float32)
    x.imag = np.where(j % 4 == 1, amp, np.where(j % 4 == 3, -amp, 0)).astype(np.float32)
    return x


def with_samples(n, at: dict, amp=1.0) -> np.ndarray:
    """background(n) with the samples `at` = {index: complex sample}"""
    x = background(n, amp)
    for j, z in at.items():
        assert 0 <= j < n, (j, n)
        x[j] = z
    x.setflags(write=False)
    return x


HIT = np.complex64(8 + 0j)  # power 64 > 4


def hits_at(n, positions) -> np.ndarray:
    return with_samples(n, {int(j): (HIT if k % 2 == 0 else np.complex64(-8j)) for k, j in enumerate(sorted(set(positions)))})


def cfg(guard, ratio=4.0, floor=0.0, rank=MEDIAN) -> bl.Cfg:
    return bl.Cfg(float(ratio), float(floor), int(rank), int(guard))


def boundaries(n) -> list[int]:
    """The last sample in front of every lane-row, tile and workgroup boundary kind the frame has (15 | 16, 1023 | 1024, 4095 | 4096)"""
    return [b - 1 for b in (bl.LANE, bl.TILE, bl.WORKGROUP) if b < n]


@functools.lru_cache(maxsize=None)
def crafted() -> tuple:
    out = []
    for n in LENGTHS:
        half = n // 2
        assert 65536 * half == MEDIAN * n
        for G in GUARDS:
            c = (cfg(G),) * N_FRAMES
            # hits at sample 0 and n - 1; then a frame with none: the run at the end of frame 1 continues into frame 2 (G >= 1)
            out.append(Case(f"ends_n{n}_G{G}", n, c, (hits_at(n, [n // 3]), hits_at(n, [0, n - 1]), hits_at(n, []))))
            # the sample in front of every boundary, then the sample behind it; frame 1 has no hit in its last G samples: no carry
            b = boundaries(n)
            out.append(Case(f"bounds_n{n}_G{G}", n, c, (hits_at(n, []), hits_at(n, b), hits_at(n, [j + 1 for j in b]))))
            # two hits 2 G apart (one run) and, in the same frame far away, 2 G + 2 apart (two runs); a hit G // 2 from the end of
            # frame 1: frame 2 starts with G - G // 2 carried samples, and has a pair across the first lane boundary itself
            a, far = 100 - G, n - 300 - 3 * G
            pair2 = [a, a + 2 * G] + ([far, far + 2 * G + 2] if n > 1024 else [])
            f2 = [a, a + 2 * G + 2] if n <= 1024 else [max(0, 15 - G // 2), 16 + G // 2 + 1]
            out.append(Case(f"pairs_n{n}_G{G}", n, c, (hits_at(n, [5]), hits_at(n, pair2 + [n - 1 - G // 2]), hits_at(n, f2))))
        # the threshold and the rank at their edges (G = 1).  Frame 0: exactly half the samples at power 0.25 (bin 1000), so the
        # median is reached IN bin 1000 (65536 cum == rank n exactly): thr of frame 1 = 4 * 0.25 = 1.0 and the unit background sits
        # AT it -- no hit; one sample at the next float above is one.  Frame 1 has one sample fewer at 0.25 and one at a power one
        # ulp below 1.0 (bin 1015): the median falls into bin 1015, thr of frame 2 = 4 * 0.9375 = 3.75.
        q = sample_of_power(0.25)
        low0 = {j: q for j in range(0, 2 * half, 2)}
        low1 = dict(list(low0.items())[1:])
        low1.update({1: sample_of_power(up(1.0)), 3: sample_of_power(down(1.0)), n - 9: sample_of_power(up(1.0))})
        f2 = {7: sample_of_power(3.75), 21: sample_of_power(up(3.75)), 40: sample_of_power(down(3.75)), 77: fused_differs(3.75)}
        out.append(Case(f"edges_n{n}", n, (cfg(1),) * N_FRAMES, (with_samples(n, low0), with_samples(n, low1), with_samples(n, f2))))
        # rank_q16 = 1 (the lowest occupied bin) and 65536 (the highest); a floor above and below fl(ratio * edge)
        spread = {3: sample_of_power(0.25), 50: sample_of_power(2.0), 51: sample_of_power(6.0), 90: sample_of_power(16.0), n - 3: sample_of_power(64.0)}
        for name, cc in (("rank1", cfg(2, rank=1)), ("rank65536", cfg(2, ratio=1.0, rank=65536)), ("floor_above", cfg(2, floor=8.0)),
                         ("floor_below", cfg(2, floor=3.0))):
            out.append(Case(f"{name}_n{n}", n, (cc,) * N_FRAMES, (with_samples(n, spread),) * N_FRAMES))
        # samples of 1e30 (p = +inf, bin 2040) where the threshold is live; rank 65536 then makes bin 2040 the reference, thr = +inf,
        # and frame 2 has no hit whatever it holds
        big = np.complex64(complex(1e30, -1e30))
        out.append(Case(f"inf_n{n}", n, (cfg(3, rank=65536),) * N_FRAMES,
                        (with_samples(n, {9: HIT}), with_samples(n, {0: big, n // 2: big, n - 1: np.complex64(1e30)}), with_samples(n, {11: np.complex64(1000.0)}))))
        # an all-zero frame, then live ones: ref_bin = 0, edge = 0.0, thr = floor = 0 -- every non-zero sample is a hit
        zero = np.zeros(n, np.complex64)
        zero.setflags(write=False)
        live = with_samples(n, {j: 0 for j in range(40, 40 + 30)})
        out.append(Case(f"zero_then_live_n{n}", n, (cfg(4),) * N_FRAMES, (zero, live, hits_at(n, [n // 2]))))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case_ids() -> list[str]:
    return [c.name for c in crafted()]


@functools.lru_cache(maxsize=None)
def model_run(case: Case) -> tuple:
    """((blanked frames), (records), (the tree's raw frames)) of a crafted case under the model: computed once, read-only"""
    ys, recs = bl.run(case.frames, list(case.cfgs))
    raws, hist = [], None
    for y in ys:
        y.setflags(write=False)
        raw, hist = behind(case.n, y, hist)
        raw.setflags(write=False)
        raws.append(raw)
    return tuple(ys), tuple(recs), tuple(raws)


# ---- the noise-and-pulse run ----------------------------------------------------------------------------------------------------
NP_N, NP_SEEDS, NP_SIGMA, NP_PULSES, NP_LEN, NP_CODE = 4112, 40, 8.0, 5, 4, 25000
NP_CFG = bl.Cfg(32.0, 0.0, MEDIAN, 8)


@functools.lru_cache(maxsize=None)
def noise_and_pulses(seed: int) -> tuple:
    """((clean CS16 frames), (the same with pulses), (pulse sample masks)): Gaussian noise of sigma = 8 dongle LSB (2048 int16 codes),
    five 4-sample pulses of +-25 000 codes per frame, at least 64 samples apart and off the frame's ends"""
    rng = np.random.default_rng(7000 + seed)
    clean, dirty, masks = [], [], []
    for f in range(N_FRAMES):
        v = np.clip(np.rint(rng.standard_normal(2 * NP_N) * NP_SIGMA * 256), -32768, 32767).astype(np.int16)
        slots = rng.permutation((NP_N - 128) // 128)[:NP_PULSES]
        w, mask = v.copy(), np.zeros(NP_N, bool)
        for s in slots:
            j = 64 + 128 * int(s) + int(rng.integers(0, 60))
            sign = rng.choice([-1, 1], size=2 * NP_LEN)
            w[2 * j: 2 * (j + NP_LEN)] = (sign * NP_CODE).astype(np.int16)
            mask[j: j + NP_LEN] = True
        for a in (v, w, mask):
            a.setflags(write=False)
        clean.append(v), dirty.append(w), masks.append(mask)
    return tuple(clean), tuple(dirty), tuple(masks)


@functools.lru_cache(maxsize=None)
def integer_frames(fmt: int, n: int, seed: int = 0, frames: int = N_FRAMES) -> tuple:
    """Frames of n integer samples in format `fmt` for the GPU tests: noise of sigma = 8 dongle LSB around a DC offset of a few LSB
    (worth removing), five 4-sample pulses near the rails in every frame"""
    from sdrreceiver_amd import ingest
    rng = np.random.default_rng(8000 + 13 * fmt + seed)
    scale, lo, hi, dt, mid = {ingest.CU8: (1, 0, 255, np.uint8, 127), ingest.CS8: (1, -128, 127, np.int8, 0),
                              ingest.CS16: (256, -32768, 32767, np.int16, 0)}[fmt]
    out = []
    for f in range(frames):
        v = np.rint((rng.standard_normal(2 * n) * NP_SIGMA + np.tile([3.0, -2.0], n)) * scale) + mid
        for s in rng.permutation((n - 128) // 48)[:NP_PULSES]:
            j = 64 + 48 * int(s)
            v[2 * j: 2 * (j + NP_LEN)] = mid + rng.choice([-100, 100], size=2 * NP_LEN) * scale
        v = np.clip(v, lo, hi).astype(dt)
        v.setflags(write=False)
        out.append(v)
    return tuple(out)


# ---- wrong devices: each one thing a kernel could get wrong ---------------------------------------------------------------------
WRONG = ["fma", "ge_threshold", "no_carry", "guard_one_sided", "hist_after_blanking", "rank_strict", "bin_upper_edge", "thr_from_same_frame",
         "floor_ignored", "runs_per_tile", "natural_order_read", "runs_recount_at_frame_start"]
# the crafted case that catches each (tests/test_blank_model.py checks every one of these)
CAUGHT_BY = {"fma": "edges_n256", "ge_threshold": "edges_n256", "no_carry": "ends_n256_G16", "guard_one_sided": "bounds_n1296_G1",
             "hist_after_blanking": "rank1_n256", "rank_strict": "edges_n1296", "bin_upper_edge": "edges_n256",
             "thr_from_same_frame": "ends_n256_G0", "floor_ignored": "floor_above_n256", "runs_per_tile": "bounds_n1296_G1",
             "natural_order_read": "bounds_n256_G0", "runs_recount_at_frame_start": "ends_n256_G1"}


def tiled(x) -> np.ndarray:
    """The frame as it lies in tile-layout memory (sdrx_dev.h), padded with zeros to whole tiles: what a kernel that forgot the
    layout would read in natural order"""
    n = x.size
    total = -(-n // 1024) * 1024
    g = np.arange(n)
    c, r = g >> 10, g & 1023
    ln, i = r >> 4, r & 15
    idx = c * 1024 + (i >> 1) * 128 + ln * 2 + (i & 1)
    t = np.zeros(total, np.complex64)
    t[idx] = x
    return t


def apply_wrong(x, cfg: bl.Cfg, state: bl.State, how) -> tuple:
    """blank.apply with one thing wrong; how = None is the definition itself (written out a second time)"""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    n, G = x.size, int(cfg.guard)
    f = x.view(np.float32)
    re, im = f[0::2], f[1::2]
    with np.errstate(over="ignore", invalid="ignore"):
        if how == "fma":  # fma(re, re, fl(im im)): one rounding fewer
            p = (re.astype(np.float64) * re.astype(np.float64) + (im * im).astype(np.float64)).astype(np.float32)
        else:
            p = (re * re) + (im * im)
    if how == "natural_order_read":
        pr = bl.power(tiled(x)[:n])  # the powers of whatever lies at the natural index in tile-layout memory
    else:
        pr = p

    def thr_of(ref_bin):
        if ref_bin < 0:
            return np.float32(np.inf)
        e = bl.edge(ref_bin + 1) if how == "bin_upper_edge" else bl.edge(ref_bin)
        with np.errstate(over="ignore"):
            t = np.float32(np.float32(cfg.ratio) * e)
        return t if how == "floor_ignored" else max(t, np.float32(cfg.floor))

    def rank(hist):
        cum = 0
        for b in range(bl.BINS):
            cum += int(hist[b])
            if (65536 * cum > cfg.rank_q16 * n) if how == "rank_strict" else (65536 * cum >= cfg.rank_q16 * n):
                return min(b, bl.MAX_BIN)
        return bl.MAX_BIN

    hist = np.bincount(bl.bin_of(pr), minlength=bl.BINS)
    nxt = rank(hist)
    thr = thr_of(nxt if how == "thr_from_same_frame" else state.ref_bin)
    hit = (pr >= thr) if how == "ge_threshold" else (pr > thr)
    carry = 0 if how == "no_carry" else min(n, max(0, G - state.tail_gap))
    c = np.concatenate([[0], np.cumsum(hit, dtype=np.int64)])
    j = np.arange(n)
    lo = j if how == "guard_one_sided" else np.maximum(j - G, 0)  # (one-sided: the guard in front of a hit only)
    blank = c[np.minimum(j + G + 1, n)] - c[lo] > 0
    blank[:carry] = True
    y = x.copy()
    y[blank] = 0
    if how == "hist_after_blanking":
        nxt = rank(np.bincount(bl.bin_of(bl.power(y)), minlength=bl.BINS))
    where = np.flatnonzero(hit)
    tail_gap = min(bl.NO_HIT, n - 1 - int(where[-1])) if where.size else bl.NO_HIT
    before = np.concatenate([[False if how == "runs_recount_at_frame_start" else state.last_blank], blank[:-1]])
    if how == "runs_per_tile":
        before[np.arange(0, n, bl.TILE)[1:]] = False
    rec = {"frame": state.frame, "n_complex": n, "measured": 1, "thr_bits": bl.thr_bits(thr), "ref_bin": state.ref_bin, "next_ref_bin": nxt,
           "hits": int(hit.sum()), "blanked": int(blank.sum()), "runs": int((blank & ~before).sum()), "carry_in": carry}
    return y, rec, bl.State(nxt, tail_gap, bool(blank[-1]), state.frame + 1)


def run_wrong(frames, cfgs, how) -> tuple[list, list]:
    state, out, recs = bl.State(), [], []
    for x, c in zip(frames, cfgs):
        y, rec, state = apply_wrong(x, c, state, how)
        out.append(y)
        recs.append(rec)
    return out, recs


def same_run(a, b) -> bool:
    """Two (frames, records) runs with the same bits and the same figures"""
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[0], b[0])) and list(a[1]) == list(b[1])  # (b may hold more)
