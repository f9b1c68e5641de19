"""What the frequency shift's tests share: the frame lengths, the crafted cases (four cf32 frames each, with their settings) and
the wrong devices as variants of the model (sdrreceiver_amd.shift).

Frame lengths: blank_ref's, at the head of the ingest chain -- 256 (less than a tile), 1296 (a tile plus 272), 4112 (the input of
a 256/257 resampler, as blank_ref.rs_case reaches it: the stage then sees the tree's 4096, four whole tiles, and the frame that
comes in and the frame the stage sees differ in length) and 4368, one workgroup plus 272.  `Case.nt` is what the stage sees.

A frame is a tone in noise (iq_ref.tone) with crafted samples in it; crafted samples are zero or have component magnitudes in
[2^-10, 2^10], so no product is subnormal."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

import blank_ref as br
import iq_ref as ir
from sdrreceiver_amd import shift as sh

LENGTHS = br.LENGTHS
assert LENGTHS == (256, 1296, 4112, sh.WORKGROUP + 272)
N_FRAMES = 4
M32 = sh.M32
INCS = (0, 1, 255, 256, 2 ** 16, 2 ** 24, 2 ** 31, 2 ** 32 - 1, 3451912, 0x9E3779B1)
NAN = np.float32(np.nan)
INF = np.float32(np.inf)

rs_case, tree, receiver_kw, behind = br.rs_case, br.tree, br.receiver_kw, br.behind


def tree_len(n: int) -> int:
    """The tree's raw frame -- what the stage sees -- for frames of n at the head of the chain"""
    c = rs_case(n)
    return c[4] if c else n


@dataclasses.dataclass(frozen=True, eq=False)  # (hashed by identity: crafted() builds each once)
class Case:
    name: str
    n: int                 # the frame that comes in
    cfgs: tuple            # one sh.Cfg per frame; one that is another object than its predecessor is set in front of its frame
    frames: tuple          # N_FRAMES complex64 arrays of n samples (read-only)
    finite: bool = True    # False: NaN and Inf samples -- compared on the raw frame and the records only

    @property
    def nt(self) -> int:
        return tree_len(self.n)


def ro(x) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.complex64)
    x.setflags(write=False)
    return x


def wrap_at(inc: int, j0: int) -> int:
    """A phase0 with which the phase passes 2^32 between samples j0 - 1 and j0 of frame 0 (0 < inc < 2^31): sample j0 has phase
    inc // 2, sample j0 - 1 has inc // 2 - inc below zero, which is just below 2^32"""
    return (inc // 2 - j0 * inc) & M32


def wrap_targets(nt: int) -> list[int]:
    """Inside a lane's 16 samples (6 | 7), on a tile boundary (1023 | 1024) and on the workgroup boundary (4095 | 4096), as far
    as the stage's frame has them"""
    return [j for j in (7, sh.TILE, sh.WORKGROUP) if j < nt]


def crafted_samples(rng, k: int) -> np.ndarray:
    """k samples whose components have magnitudes 2^e, e uniform in [-10, 10], and random signs"""
    mag = np.exp2(rng.uniform(-10, 10, 2 * k))
    return (mag * rng.choice([-1.0, 1.0], 2 * k)).astype(np.float32).view(np.complex64)


def base_frames(n: int, seed: int) -> list[np.ndarray]:
    """Four frames of the tone in noise, with crafted magnitudes on either side of every boundary the stage's frame has"""
    rng = np.random.default_rng(9100 + seed)
    nt, out = tree_len(n), []
    for f in range(N_FRAMES):
        x = ir.tone(n, f, noise=6.0, seed=seed, dc=False).copy()
        at = sorted({0, n - 1} | {j + d for j in (15, 1023, 4095) if j + 1 < nt for d in (0, 1)})
        x[at] = crafted_samples(rng, len(at))
        out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def crafted() -> tuple:
    out = []
    for n in LENGTHS:
        nt = tree_len(n)
        targets = wrap_targets(nt)
        for k, inc in enumerate(INCS):
            # every increment, the 2^32 wrap of frame 0 on one of the boundaries in turn (0 and the increments of 2^31 and beyond: a phase0 with all bytes live)
            ph = wrap_at(inc, targets[k % len(targets)]) if 0 < inc < 2 ** 31 else 0x89ABCDEF
            c = sh.Cfg(inc, ph)
            out.append(Case(f"inc{inc:08x}_n{n}", n, (c,) * N_FRAMES, tuple(ro(x) for x in base_frames(n, k))))
        for j0 in targets:  # one increment on every boundary
            c = sh.Cfg(3451912, wrap_at(3451912, j0))
            out.append(Case(f"wrap{j0}_n{n}", n, (c,) * N_FRAMES, tuple(ro(x) for x in base_frames(n, 20 + j0))))
        # the advance n inc of a frame wraps several times (about n / 2 + n / 5 times): the phase behind the frame is the product mod 2^32
        c = sh.Cfg(2 ** 31 + 0x33333333, 0x01020304)
        out.append(Case(f"advance_wraps_n{n}", n, (c,) * N_FRAMES, tuple(ro(x) for x in base_frames(n, 31))))
        # the increment changes behind frame 1 (the phase carries on), and a phase is loaded behind frame 2
        a, b, d = sh.Cfg(3451912, 0x40000000), sh.Cfg(0xFF000123, 0), sh.Cfg(0xFF000123, 0xC0FFEE00, sh.LOAD_PHASE)
        out.append(Case(f"change_n{n}", n, (a, a, b, d), tuple(ro(x) for x in base_frames(n, 32))))
        if rs_case(n):
            continue  # (crafted zeros and non-finite samples do not survive a resampler in front of the stage)
        # signed zeros: every combination in either component, alone and beside a finite component, at the identity and in motion
        z = np.array([0.0, -0.0, 0.0, -0.0, 1.5, -1.5, 0.0, -0.0, 0.0, 0.0, -0.0, -0.0, 0.0, -0.0, 2.0, -2.0], np.float32).view(np.complex64)
        fr = []
        for f in range(N_FRAMES):
            x = base_frames(n, 33)[f]
            x[16 * f: 16 * f + 8] = z
            x[n - 8:] = z[::-1]
            fr.append(ro(x))
        out.append(Case(f"zeros_identity_n{n}", n, (sh.Cfg(0, 0),) * N_FRAMES, tuple(fr)))
        out.append(Case(f"zeros_n{n}", n, (sh.Cfg(0x12345678, 0x0FEDCBA9),) * N_FRAMES, tuple(fr)))
        # NaN, +-Inf and -0 samples
        odd = [complex(NAN, 1.0), complex(2.0, NAN), complex(INF, -3.0), complex(-INF, 3.0), complex(4.0, INF), complex(5.0, -INF), complex(NAN, NAN),
               complex(INF, INF), complex(-0.0, -0.0), complex(INF, 0.0), complex(0.0, -INF)]
        fr = []
        for f in range(N_FRAMES):
            x = base_frames(n, 34)[f]
            for m, v in enumerate(odd):
                x[(5 + 23 * m + 7 * f) % n] = v
            x[n - 1 - f] = odd[f]
            fr.append(ro(x))
        out.append(Case(f"nonfinite_n{n}", n, (sh.Cfg(0x9E3779B1, 5),) * N_FRAMES, tuple(fr), finite=False))
        out.append(Case(f"nonfinite_identity_n{n}", n, (sh.Cfg(0, 0),) * N_FRAMES, tuple(fr), finite=False))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case_ids() -> list[str]:
    return [c.name for c in crafted()]


def by_name(name: str) -> Case:
    return next(c for c in crafted() if c.name == name)


@functools.lru_cache(maxsize=None)
def tree_frames(case: Case) -> tuple:
    """The frames as they reach the stage: the case's own, or what the resampler in front makes of them; read-only"""
    out, hist = [], None
    for x in case.frames:
        z, hist = behind(case.n, x, hist)
        z = ro(z)
        out.append(z)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def model_run(case: Case) -> tuple:
    """((the frames that reach the stage), (the shifted frames: the tree's raw frames), (records)) of a crafted case under the
    model: computed once, read-only"""
    zs = tree_frames(case)
    ys, recs = sh.run(zs, list(case.cfgs))
    for y in ys:
        y.setflags(write=False)
    return zs, tuple(ys), tuple(recs)


# ---- wrong devices: each one thing a kernel or its launch code could get wrong ----------------------------------------------------
FMA = ["fma_re_first", "fma_re_second", "fma_im_first", "fma_im_second"]  # one fused product-sum of the four (x) could hold
WRONG = FMA + ["assoc_a_bc", "low_byte_rounded", "two_tables", "conjugate", "phase_not_advanced", "advance_in_frame", "advance_padded", "inc_one_frame_late",
               "phase_fp32"]
# the crafted case that catches each (tests/test_shift_model.py checks every one of these)
CAUGHT_BY = {"fma_re_first": "inc0034ac08_n256", "fma_re_second": "inc0034ac08_n256", "fma_im_first": "inc0034ac08_n256", "fma_im_second": "inc0034ac08_n256",
             "assoc_a_bc": "inc0034ac08_n256", "low_byte_rounded": "inc000000ff_n256", "two_tables": "inc0034ac08_n1296", "conjugate": "inc01000000_n256",
             "phase_not_advanced": "inc00000001_n256", "advance_in_frame": "inc0034ac08_n4112", "advance_padded": "inc0034ac08_n1296",
             "inc_one_frame_late": "change_n256", "phase_fp32": "inc9e3779b1_n4368"}


@functools.lru_cache(maxsize=None)
def tables11() -> tuple:
    """The two-table variant: 11 + 11 bits"""
    out = []
    for denom in (2048.0, 4194304.0):
        k = np.arange(2048)
        out.append(np.array([complex(np.float32(math.cos(2 * math.pi * j / denom)), np.float32(math.sin(2 * math.pi * j / denom))) for j in k], np.complex64))
    return tuple(out)


def cmul_wrong(a, b, how) -> np.ndarray:
    """shift.cmul, or with one of its four product-sums fused: the product taken exactly (24 x 24 bits fit a double) and added to
    the other, rounded, product in double"""
    a, b = np.asarray(a, dtype=np.complex64), np.asarray(b, dtype=np.complex64)
    ar, ai, br_, bi = (np.ascontiguousarray(v, dtype=np.float32) for v in (a.real, a.imag, b.real, b.imag))
    D = np.float64
    y = np.empty(np.broadcast(a, b).shape, np.complex64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        rr, ii, ri, ir_ = ar * br_, ai * bi, ar * bi, ai * br_
        re, im = rr - ii, ri + ir_
        if how == "fma_re_first":
            re = (ar.astype(D) * br_.astype(D) - ii.astype(D)).astype(np.float32)
        elif how == "fma_re_second":
            re = (rr.astype(D) - ai.astype(D) * bi.astype(D)).astype(np.float32)
        elif how == "fma_im_first":
            im = (ar.astype(D) * bi.astype(D) + ir_.astype(D)).astype(np.float32)
        elif how == "fma_im_second":
            im = (ri.astype(D) + ai.astype(D) * br_.astype(D)).astype(np.float32)
        y.real, y.imag = re, im
    return y


def apply_wrong(x, state: sh.State, how, in_frame: int) -> tuple:
    """shift.apply with one thing wrong; how = None is the definition itself (written out a second time).  `in_frame`: the length
    of the frame that came in at the head of the chain."""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    n = x.size
    A, B, C = sh.tables()
    j = np.arange(n, dtype=np.uint64)
    if how == "phase_fp32":  # the phase kept as a float in turns, one fp32 addition a sample
        step = np.float32(state.inc / 2.0 ** 32)
        acc = np.cumsum(np.concatenate([[np.float32(state.phase / 2.0 ** 32)], np.full(n - 1, step, np.float32)]), dtype=np.float32)
        p = (np.floor((acc.astype(np.float64) % 1.0) * 2.0 ** 32).astype(np.uint64) & np.uint64(M32)).astype(np.uint32)
    else:
        p = ((np.uint64(state.phase) + j * np.uint64(state.inc)) % np.uint64(1 << 32)).astype(np.uint32)
    if how == "low_byte_rounded":
        p = ((p.astype(np.uint64) + np.uint64(128)) & np.uint64(M32)).astype(np.uint32)
    mul = (lambda a, b: cmul_wrong(a, b, how)) if how in FMA else (lambda a, b: cmul_wrong(a, b, None))
    if how == "two_tables":
        T1, T2 = tables11()
        rot = mul(T1[(p >> np.uint32(21)).astype(np.intp)], T2[((p >> np.uint32(10)) & np.uint32(2047)).astype(np.intp)])
    else:
        a, b, c = A[(p >> np.uint32(24)).astype(np.intp)], B[((p >> np.uint32(16)) & np.uint32(255)).astype(np.intp)], C[((p >> np.uint32(8)) & np.uint32(255)).astype(np.intp)]
        rot = mul(a, mul(b, c)) if how == "assoc_a_bc" else mul(mul(a, b), c)
    if how == "conjugate":
        rot = np.conj(rot)
    y = mul(x, rot)
    f = y.view(np.float32)
    f[np.isnan(f)] = np.array([sh.NAN_BITS], np.uint32).view(np.float32)[0]
    steps = {"phase_not_advanced": 0, "advance_in_frame": in_frame, "advance_padded": -(-n // sh.TILE) * sh.TILE}.get(how, n)
    nxt = (state.phase + steps * state.inc) % (1 << 32)
    rec = {"frame": state.frame, "n_complex": n, "applied": 1, "phase": state.phase, "inc": state.inc, "next_phase": nxt, "next_inc": state.inc}
    return y, rec, sh.State(nxt, state.inc, state.frame + 1)


def run_wrong(case: Case, how) -> tuple[list, list]:
    """A case's frames, as they reach the stage, through apply_wrong"""
    cfgs = case.cfgs
    state, out, recs = sh.State.initial(cfgs[0]), [], []
    pending = None
    for f, x in enumerate(tree_frames(case)):
        if how == "inc_one_frame_late" and pending is not None:
            state, pending = dataclasses.replace(state, inc=pending), None
        if f and cfgs[f] is not cfgs[f - 1]:
            new = sh.load(state, cfgs[f])
            if how == "inc_one_frame_late":
                pending, new = new.inc, dataclasses.replace(new, inc=state.inc)
            state = new
        y, rec, state = apply_wrong(x, state, how, case.n)
        out.append(y)
        recs.append(rec)
    return out, recs


def same_run(a, b) -> bool:
    """Two (frames, records) runs with the same bits and the same figures"""
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[0], b[0])) and list(a[1]) == list(b[1])


# ---- integer frames ----------------------------------------------------------------------------------------------------------------
integer_frames = ir.integer_frames
