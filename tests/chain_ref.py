"""What the tests of the ingest chain as a whole share: the composed model, the cases, their frames, and eleven wrong devices.

The stages in front of level 0 -- format conversion, DC-bias removal, ADC meter, impulse blanker, half-band front stages,
rational resampler -- each have a numpy model the device is held to bit for bit (sdrreceiver_amd.ingest, oracle.binding.dc_correct,
adc_ref, sdrreceiver_amd.blank / front / resample).  :class:`Chain` composes them in the device's order and carries the state of one
receiver across frames; nothing here is new arithmetic.  The wrong devices are variants of the composition, each one thing a
LAUNCH PATH could get wrong (a buffer, a frame length, a history slot, a state that a drain resets): what the per-stage tests
cannot see.

The cases, 8 frames each -- enough to visit each slot of the two-slot history and record buffers four times:

    A  CS8 -> blanker G = 17 -> 2 complex stages K = 3                      9472 -> 2368          3 blanker workgroups, the middle
                                                                                                  one with both halos in the frame
    B  CS16 -> DC -> blanker G = 1 -> 1 stage K = 31 -> 16/25, T = 24       6400 -> 3200 -> 2048  the longest front history; all
                                                                                                  three stages behind DC removal
    C  CU8 -> blanker G = 8 -> 3 stages K = 7 -> 3/4, T = 16                13824 -> 1728 -> 1296 4 blanker workgroups, short last
                                                                                                  tiles at every rate
    D  CS16 -> blanker G = 64 -> 1 stage K = 7 -> 256/257, T = 8            8224 -> 4112 -> 4096  a last workgroup of two lanes, a
                                                                                                  front tile of 16 outputs
    E  RS16 / RU12 -> real stage + 2 complex K = 7 -> 5/3, T = 16           6144 -> 768 -> 1280   real input, an upsampler, no blanker
    F  CS16 -> blanker G = 64 (G = 0 in one frame), nothing behind it       20752                 hand-placed hits on a background
    W  A's chain in front of seven parent-less VFOs                         as A                  level 0 does not read the frame itself

The taps are the built-in designs (unit gain: the tree sees samples of the range it is meant for), handed over as arrays so that
the model needs no device to know them."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import adc_ref as ar
import blank_ref as br
import front_ref as fx
import resample_ref as rr
from oracle import binding as ob
from sdrreceiver_amd import blank as bl, front as fr, ingest, resample as rs, topology as tp

N_FRAMES = 8
ATTEN_DB = 60.0
PULSE_LEN = 4
WG, HALO = bl.WORKGROUP, bl.HALO


@dataclasses.dataclass(frozen=True, eq=False)  # (hashed by identity: CASES holds each once)
class Case:
    name: str
    fmts: tuple            # the formats the frames alternate among
    in_frame: int          # what a frame call takes: complex samples, or real samples where the first stage is the real one
    guard: int | None      # the blanker's guard; None: no blanker
    real: bool
    stages: int            # 0: no front stage
    K: int
    rs: tuple | None       # resample_ref's (L, M, T, n_in, n); None: no resampler
    n0: int                # the front stage's output frame (the resampler's input, where there is one)
    n: int                 # the tree's frame
    correct_dc: bool = False
    wide: bool = False     # the tree of seven parent-less VFOs

    def topo(self) -> tp.Topology:
        t = rr.tree(self.rs or (1, 1, 8, self.n, self.n))
        if self.wide:  # six more parent-less leaves behind the main and its two subs: seven VFOs on level 0
            n, fs = self.n, 4 * self.n
            for j in range(5):
                t.vfos.append(tp.VfoDesc(topic=f"RAW{4 + j:02d}", parent=-1, fs=fs, decimate_count=0, mixer_freq=float((-1) ** j * (n // (17 + 2 * j))),
                                         demod_usb=False, cstyle=j & 1, samples_per_buffer=n))
            t.name = "chainW"
        return t

    def front_taps(self):
        return fr.design(self.K, ATTEN_DB)[0] if self.stages else None

    def rs_taps(self):
        return rs.design(*rr.rates(self.rs), self.rs[2], ATTEN_DB)[0] if self.rs else None

    def cfg(self, f: int = 0):
        """The blanker's settings of frame f (None: no blanker)"""
        if self.guard is None:
            return None
        if self.name == "F":
            return br.cfg(0 if f == F_G0_FRAME else self.guard)
        return bl.Cfg(br.NP_CFG.ratio, br.NP_CFG.floor, br.NP_CFG.rank_q16, self.guard)

    def receiver_kw(self, stages_on: bool = True) -> dict:
        """The Receiver arguments of the case beside the launch options; stages_on False: its twin without the stages"""
        if not stages_on:
            return {}
        kw = dict(adc_meter=True)
        if self.stages:
            kw.update(front_stages=self.stages, front_real=self.real, front_taps=self.front_taps())
        if self.rs:
            kw.update(input_rate=rr.rates(self.rs)[0], resample_taps=self.rs_taps())
        if self.guard is not None:
            kw.update(blanker=self.cfg(0))
        return kw


R = (ingest.RS16, ingest.RU12)
CASES = {c.name: c for c in (
    Case("A", (ingest.CS8,), 9472, 17, False, 2, 3, None, 2368, 2368),
    Case("B", (ingest.CS16,), 6400, 1, False, 1, 31, rr.CASES[3], 3200, 2048, correct_dc=True),
    Case("C", (ingest.CU8,), 13824, 8, False, 3, 7, rr.CASES[2], 1728, 1296),
    Case("D", (ingest.CS16,), 8224, 64, False, 1, 7, br.RS_4112, 4112, 4096),
    Case("E", R, 6144, None, True, 3, 7, rr.CASES[4], 768, 1280),
    Case("F", (ingest.CS16,), 5 * WG + 272, 64, False, 0, 0, None, 5 * WG + 272, 5 * WG + 272),
    Case("W", (ingest.CS8,), 9472, 17, False, 2, 3, None, 2368, 2368, wide=True),
)}
for _c in CASES.values():
    assert _c.in_frame == (fr.in_frame(_c.n0, _c.stages) if _c.stages else _c.n0) and (_c.rs[3:] == (_c.n0, _c.n) if _c.rs else _c.n0 == _c.n)


# ---- frames -------------------------------------------------------------------------------------------------------------------
def pulse_plan(n: int, G: int) -> tuple:
    """Where the 4-sample pulses of frames 0 .. 7 start, for a frame of n samples at the blanker.  Frame 0 sets the reference.
    1: across 4095 | 4096 and 8191 | 8192; 2: ending at n - 1 - G // 2, so that frame 3 starts with G - G // 2 carried samples;
    3: in the last workgroup; 4: at sample 0; 5: beginning at 4096 (workgroup 0 learns of it through its rear halo alone) and
    ending at 8191 (workgroup 2 through its front halo alone); 6: across a lane row, a tile, ending at 4095, and across
    12287 | 12288; 7: at sample 0, across 8191 | 8192 and ending at n - 1.  (Boundaries the frame does not have are left out.)"""
    last = (n - 1) // WG * WG
    plan = ([],
            [4094] + ([8190] if n > 8194 else []),
            [n - PULSE_LEN - G // 2],
            [last + (n - last) // 2],
            [0],
            [4096] + ([8188] if n > 8192 else []),
            [14, 1022, 4092] + ([12286] if n > 12290 else []),
            [0] + ([8190] if n > 8194 else []) + [n - PULSE_LEN])
    for starts in plan:
        assert all(0 <= s and s + PULSE_LEN <= n for s in starts) and all(b - a > PULSE_LEN for a, b in zip(starts, starts[1:]))
    return plan


BOUNDARY_FRAME = 1  # the frame whose run crosses 4095 | 4096
CARRY_FRAME = 3     # the frame that starts with carried samples


@functools.lru_cache(maxsize=None)
def frames(case: Case) -> tuple:
    """((samples, fmt), ...) of the case's eight frames, read-only.  A, B, C, D, W: blank_ref.integer_frames' noise (sigma = 8
    dongle LSB around a DC offset of a few LSB) with pulse_plan's pulses of +-100 LSB in place of its random ones.  E: full-range
    real samples, RS16 and RU12 alternating.  F: see f_frames."""
    if case.name == "F":
        return f_frames(case.in_frame)
    out = []
    if case.real:
        for f in range(N_FRAMES):
            fmt = case.fmts[f % len(case.fmts)]
            out.append((fx.full_range(fmt, case.in_frame, 4000 + f), fmt))
    else:
        n, fmt = case.in_frame, case.fmts[0]
        rng = np.random.default_rng(9000 + 13 * fmt + n)
        scale, lo, hi, dt, mid = {ingest.CU8: (1, 0, 255, np.uint8, 127), ingest.CS8: (1, -128, 127, np.int8, 0),
                                  ingest.CS16: (256, -32768, 32767, np.int16, 0)}[fmt]
        for starts in pulse_plan(n, case.guard):
            v = np.rint((rng.standard_normal(2 * n) * br.NP_SIGMA + np.tile([3.0, -2.0], n)) * scale) + mid
            for j in starts:
                v[2 * j: 2 * (j + PULSE_LEN)] = mid + rng.choice([-100, 100], size=2 * PULSE_LEN) * scale
            out.append((np.clip(v, lo, hi).astype(dt), fmt))
    for v, _ in out:
        v.setflags(write=False)
    return tuple(out)


F_FULL_FRAME, F_G64_FRAME, F_G0_FRAME, F_EACH_FRAME = 1, 2, 3, 4
F_RUN = (3500, 5000)  # a run of consecutive hits that starts inside workgroup 0 and covers workgroup 1 entirely
F_EDGES = (4095, 4096, 8191, 8192, 12287, 12288)
F_EACH = (17, WG + 1000, 2 * WG + 2500, 3 * WG + 4095, 4 * WG, 5 * WG + 200)  # one hit in each of the six workgroups


def f_frames(n: int) -> tuple:
    """Case F: blank_ref.background (unit power: CS16 codes of +-256) with hits of power 64 (ratio 4 at the median: thr = 4.0).
    0: the reference; 1: F_RUN; 2: F_EDGES with G = 64; 3: F_EDGES with G = 0; 4: F_EACH; 5: a hit at n - 1 - 32, so that
    6 starts with 32 carried samples; 7: hits at 0 and n - 1."""
    assert F_RUN[0] < WG and F_RUN[0] + F_RUN[1] >= 2 * WG and n == 5 * WG + 272
    hits = ([n // 3], range(F_RUN[0], F_RUN[0] + F_RUN[1]), F_EDGES, F_EDGES, F_EACH, [n - 1 - 32], [9000], [0, n - 1])
    out = []
    for h in hits:
        x = br.hits_at(n, list(h))
        v = (x.view(np.float32) * np.float32(256.0)).astype(np.int16)
        assert np.array_equal(ingest.to_float(v), x.view(np.float32))
        v.setflags(write=False)
        out.append((v, ingest.CS16))
    return tuple(out)


# ---- the blanker once more, workgroup by workgroup: where a launch of several workgroups can go wrong ------------------------------
def blank_by_workgroups(x, cfg: bl.Cfg, state: bl.State, how=None) -> tuple:
    """blank.apply computed the way k_blank is laid out -- every workgroup of 4096 samples dilates the hits of its own samples and
    of a halo of 128 on either side, and counts the runs that begin in it, knowing of the sample in front of its first one.
    how None: the definition.  "ignores_rear_halo": a workgroup that is not the last sees no hit behind its own samples.
    "wg_last_blank": every workgroup takes the previous FRAME's last blank bit for the sample in front of its first one.
    "clusters": nothing in front of any workgroup is blank -- `runs` is then the number of per-workgroup clusters."""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    n, G = x.size, int(cfg.guard)
    p = bl.power(x)
    thr = bl.threshold(state.ref_bin, cfg)
    hit = p > thr
    carry = min(n, max(0, G - state.tail_gap))
    blank = np.zeros(n, bool)
    for base in range(0, n, WG):
        end = min(base + WG, n)
        lo, hi = max(base - HALO, 0), min(end + HALO, n)
        if how == "ignores_rear_halo" and end < n:
            hi = end
        blank[base:end] = bl.dilate(hit[lo:hi], G)[base - lo: end - lo]
    blank[:carry] = True
    runs = 0
    for base in range(0, n, WG):
        seg = blank[base: base + WG]
        first = False if how == "clusters" else state.last_blank if base == 0 or how == "wg_last_blank" else blank[base - 1]
        runs += int((seg & ~np.concatenate([[first], seg[:-1]])).sum())
    y = x.copy()
    y[blank] = 0
    where = np.flatnonzero(hit)
    tail_gap = min(bl.NO_HIT, n - 1 - int(where[-1])) if where.size else bl.NO_HIT
    nxt = bl.rank_bin(np.bincount(bl.bin_of(p), minlength=bl.BINS), n, cfg.rank_q16)
    rec = {"frame": state.frame, "n_complex": n, "measured": 1, "thr_bits": bl.thr_bits(thr), "ref_bin": state.ref_bin, "next_ref_bin": nxt,
           "hits": int(hit.sum()), "blanked": int(blank.sum()), "runs": runs, "carry_in": carry}
    return y, rec, bl.State(nxt, tail_gap, bool(blank[-1]), state.frame + 1)


# ---- the composed model ---------------------------------------------------------------------------------------------------------
Step = dataclasses.make_dataclass("Step", ["blank_in", "blank_out", "rec", "front_out", "raw", "adc"])

WRONG = ["blanker_behind_front", "blanker_at_tree_length", "front_zero_history", "stage2_stage1_history", "resampler_history_unblanked",
         "dc_fed_blanked", "adc_fed_blanked", "ignores_rear_halo", "wg_last_blank", "carry_dropped_with_front", "slots_mod3"]
# the case that catches each (tests/test_chain_model.py checks every one of these)
CAUGHT_BY = {"blanker_behind_front": "A", "blanker_at_tree_length": "A", "front_zero_history": "C", "stage2_stage1_history": "A",
             "resampler_history_unblanked": "D", "dc_fed_blanked": "B", "adc_fed_blanked": "A", "ignores_rear_halo": "A",
             "wg_last_blank": "C", "carry_dropped_with_front": "D", "slots_mod3": "E"}


class _Slots:
    """A state a stage keeps in a two-slot parity buffer: frame f reads what frame f - 1 wrote.  With mod3 the slot is taken from
    frame % 3 where the code has frame & 1 (the slots `p` and `p ^ 1` of a buffer that then needs four)."""

    def __init__(self, mod3: bool):
        self.mod3, self.slots = mod3, [None] * 4

    def read(self, f: int):
        return self.slots[(f % 3) ^ 1] if self.mod3 else self.slots[(f & 1) ^ 1]

    def write(self, f: int, value) -> None:
        self.slots[f % 3 if self.mod3 else f & 1] = value

    def delivered(self, f: int):
        """What the host finds for frame f: it looks into the slot of the frame's parity"""
        return self.slots[f & 1]


class Chain:
    """The state of one receiver of `case` across frames: the DC accumulator, the blanker's state, every front stage's history,
    the resampler's, the frame number.  `how`: one of WRONG, or None for the definition."""

    def __init__(self, case: Case, how: str | None = None):
        assert how is None or how in WRONG
        self.case, self.how = case, how
        self.h, self.h_rs = case.front_taps(), case.rs_taps()
        self.dc = np.zeros(2, np.float32)
        self.st = bl.State()
        self.cfg = case.cfg(0)
        mod3 = how == "slots_mod3"
        self.front_hist, self.rs_hist, self.recs, self.adcs = _Slots(mod3), _Slots(mod3), _Slots(mod3), _Slots(mod3)
        self.shadow_front, self.shadow_rs = None, None  # the histories of the chain WITHOUT the blanker ("resampler_history_unblanked")
        self.frame = 0

    def set_blanker(self, cfg: bl.Cfg) -> None:
        self.cfg = cfg

    def _blank(self, x):
        how = self.how if self.how in ("ignores_rear_halo", "wg_last_blank") else None
        st = self.st
        if self.how == "carry_dropped_with_front" and self.case.stages:
            st = dataclasses.replace(st, tail_gap=bl.NO_HIT)
        if how:
            y, rec, self.st = blank_by_workgroups(x, self.cfg, st, how)
        else:
            y, rec, self.st = bl.apply(x, self.cfg, st)
        return y, rec

    def _front(self, x, f):
        c = self.case
        if not c.stages:
            return x
        hists = None if self.how == "front_zero_history" else self.front_hist.read(f)
        if self.how == "stage2_stage1_history":
            y, hists = fx.run_wrong(x, self.h, c.stages, c.real, hists, "stage2_stage1_history")
        else:
            y, hists = fr.run(x, self.h, c.stages, c.real, hists)
        self.front_hist.write(f, hists)
        return y

    def step(self, samples, fmt, correct_dc: bool = False, converted=None) -> Step:
        """One frame of integer samples: (the blanker's input, its output, its record, the front stage's output -- the
        resampler's input --, the tree's raw frame, the ADC record); None where the case has no such stage.  `converted`: the
        frame behind the conversion and the DC-bias removal where the model's is not to be used (a DC form that is held to a
        tolerance: everything behind it is then the model of what that form delivered)."""
        c, how, f = self.case, self.how, self.frame
        x = fx.to_input(samples, fmt)
        if converted is not None:
            x = np.ascontiguousarray(converted, dtype=np.complex64).reshape(-1)
            assert x.size == c.in_frame and how is None
        elif correct_dc:
            iq = x.view(np.float32).copy()
            before = self.dc.copy()
            ob.dc_correct(iq, self.dc)
            x = iq.view(np.complex64)
        adc_of = fx.adc_pair_model if ingest.is_real(fmt) else ar.model
        adc_samples = samples
        blank_in = blank_out = rec = None
        y = x
        if c.guard is not None and how == "blanker_behind_front":
            y = self._front(x, f)
            blank_in = y
            blank_out, rec = self._blank(y)
            y = blank_out
        elif c.guard is not None:
            blank_in = x
            if how == "blanker_at_tree_length" and c.n < x.size:
                head, rec = self._blank(x[: c.n])
                blank_out = np.concatenate([head, x[c.n:]])
            else:
                blank_out, rec = self._blank(x)
            gone = blank_out.view(np.uint64) != x.view(np.uint64)  # the samples the blanker changed
            if how == "dc_fed_blanked" and correct_dc:  # the accumulator follows the frame behind the blanker
                z = fx.to_input(samples, fmt).copy()
                z[gone] = 0
                self.dc = before
                ob.dc_correct(z.view(np.float32), self.dc)
            if how == "adc_fed_blanked":  # the meter counts the codes of the samples that were left
                adc_samples = np.array(samples)
                zero = 127 if fmt == ingest.CU8 else 0
                adc_samples[0::2][gone], adc_samples[1::2][gone] = zero, zero
            y = self._front(blank_out, f)
        else:
            y = self._front(x, f)
        front_out = y if c.stages else None
        raw = y
        if c.rs:
            L, M = c.rs[:2]
            hist = self.rs_hist.read(f)
            if how == "resampler_history_unblanked" and c.guard is not None:
                # the history is the tail of what the resampler's input would be WITHOUT the blanker
                shadow, self.shadow_front = fr.run(x, self.h, c.stages, c.real, self.shadow_front) if c.stages else (x, None)
                hist, self.shadow_rs = self.shadow_rs, shadow[shadow.size - (c.rs[2] - 1):].copy()
            raw, hist = rs.apply(y, self.h_rs, L, M, hist)
            self.rs_hist.write(f, hist)
        self.recs.write(f, rec)
        self.adcs.write(f, adc_of(adc_samples, fmt, frame=f))
        self.frame += 1
        return Step(blank_in, blank_out, self.recs.delivered(f), front_out, raw, self.adcs.delivered(f))


@functools.lru_cache(maxsize=None)
def model_run(case: Case, how: str | None = None) -> tuple:
    """The eight Steps of a case under the model (or a wrong device): computed once, read-only"""
    m = Chain(case, how)
    out = []
    for f, (v, fmt) in enumerate(frames(case)):
        if case.guard is not None and case.cfg(f) != m.cfg:
            m.set_blanker(case.cfg(f))
        s = m.step(v, fmt, case.correct_dc)
        for a in (s.blank_in, s.blank_out, s.front_out, s.raw):
            if a is not None:
                a.setflags(write=False)
        out.append(s)
    return tuple(out)


def same_step(a: Step, b: Step) -> bool:
    """Two Steps with the same bits and the same figures"""
    for u, v in ((a.blank_in, b.blank_in), (a.blank_out, b.blank_out), (a.front_out, b.front_out), (a.raw, b.raw)):
        if (u is None) != (v is None) or (u is not None and (u.size != v.size or not np.array_equal(_bits(u), _bits(v)))):
            return False
    return a.rec == b.rec and a.adc == b.adc


def same_run(a, b) -> bool:
    return len(a) == len(b) and all(same_step(u, v) for u, v in zip(a, b))


def _bits(x) -> np.ndarray:
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.complex64 else np.uint32)
