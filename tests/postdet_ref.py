"""What the post-detection filter's tests share: the small trees, the crafted frames and the wrong devices as variants of the model
(sdrreceiver_amd.postdet).

Trees.  "a" is detect_ref.tree_a (root frame 16 384) with filters on its detector leaves: exactly one block of 4096 stream samples
(parent-less, below a main, below a main of a main), two whole blocks, half a block; T = 1, 2, 17, 64, 255, 256; R = 1, 2, 16; beside
USB and IQ leaves and an unfiltered FM leaf.  "c" has a root frame of 30 720: parent-less leaves of 15 360 (three blocks and 3072),
leaves of 7680 (a block and a partial one) and of 60 below a main of a main -- 60 < T - 1 = 63, the history spans more than one frame
-- with R = 3, 5 and 6, for which no block edge is a multiple of R, and R = 16; beside unfiltered AM and FM leaves and an IQ leaf.

Crafted frames are STREAMS, as detect_ref's are: the model tests use them as they are, the GPU tests feed them to parent-less leaves
with no decimation and a mixer at 0 Hz and hold the device to the model on the device's own stream."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import detect_ref as dr
from sdrreceiver_amd import detect as dt, postdet as pd
from sdrreceiver_amd.topology import Topology

FS = dr.FS
N_CRAFT = dr.N_CRAFT  # 4368 = 16 * 3 * 7 * 13: a block and a partial one; R = 1, 2, 3, 6, 16 divide it
N_FRAMES = dr.N_FRAMES
BLOCK = dr.BLOCK
f32 = np.float32
ro = dr.ro


def taps_random(T: int, seed: int) -> tuple:
    """T float32 taps with no symmetry (a reversed or shifted filter is another filter), about unit gain"""
    rng = np.random.default_rng(9100 + seed)
    h = rng.uniform(-1.0, 1.0, T) / np.sqrt(T) + 1.0 / T
    return tuple(h.astype(f32).tolist())


def taps_lowpass(T: int, cutoff_hz: float, atten_db: float = 60.0, fs: float = FS) -> tuple:
    return tuple(pd.design(fs, cutoff_hz, T, atten_db)[0].tolist())


def _with(topo: Topology, filters: dict, name: str) -> Topology:
    v = [dataclasses.replace(d, post_taps=filters[i][0], post_decim=filters[i][1]) if i in filters else d for i, d in enumerate(topo.vfos)]
    return Topology(fs=topo.fs, frame=topo.frame, vfos=v, name=name)


def tree_a() -> Topology:
    return _with(dr.tree_a(), {
        1: (taps_random(17, 1), 2),     # AM 8192 below a main: two blocks
        2: (taps_random(64, 2), 16),    # FM 4096 below a main: exactly one block
        6: (taps_random(255, 3), 1),    # AM 4096 below a main of a main
        7: (taps_random(256, 4), 2),    # FM 2048 below a main of a main
        9: ((0.75,), 1),                # AM 4096, parent-less: T = 1
        10: (taps_random(2, 5), 1),     # FM 4096, parent-less
    }, "postdet-a")                     # 11: an FM leaf without a filter (and without a topic)


def tree_c() -> Topology:
    t = Topology(fs=FS, frame=30720, name="postdet-c")
    L = dr._leaf
    t.vfos.append(L("", -1, FS, 30720, 1, -2500.0, cstyle=1))                  # 0: main, 15 360
    t.vfos.append(L("AM0", -1, FS, 30720, 1, 4000.0, dt.AM))                   # 1: 15 360
    t.vfos.append(L("FM0", -1, FS, 30720, 1, -4000.0, dt.FM, gain=1.0))        # 2: 15 360
    t.vfos.append(L("AM1", 0, FS // 2, 15360, 1, 800.0, dt.AM))                # 3: 7680
    t.vfos.append(L("FM1", 0, FS // 2, 15360, 1, -800.0, dt.FM))               # 4: 7680
    t.vfos.append(L("", 0, FS // 2, 15360, 1, 500.0, cstyle=1))                # 5: main below main, 7680
    t.vfos.append(L("AM2", 5, FS // 4, 7680, 7, 100.0, dt.AM, gain=0.7))       # 6: 60
    t.vfos.append(L("FM2", 5, FS // 4, 7680, 7, -100.0, dt.FM, gain=0.7))      # 7: 60
    t.vfos.append(L("AM3", 0, FS // 2, 15360, 1, 1800.0, dt.AM))               # 8: 7680, no filter
    t.vfos.append(L("FM3", 0, FS // 2, 15360, 2, -1800.0, dt.FM))              # 9: 3840
    t.vfos.append(L("IQ0", 0, FS // 2, 15360, 1, -700.0, cstyle=0))            # 10
    t.vfos.append(L("FM4", 5, FS // 4, 7680, 1, 300.0, dt.FM))                 # 11: 3840, no filter
    t.vfos.append(L("AM4", 0, FS // 2, 15360, 0, 2600.0, dt.AM))               # 12: 15 360 below a main
    return _with(t, {
        1: (taps_random(64, 11), 6),    # three blocks and 3072, R = 6
        2: (taps_random(255, 12), 5),   # R = 5
        3: (taps_random(256, 13), 3),   # a block and a partial one, R = 3
        4: (taps_random(17, 14), 6),
        6: (taps_random(64, 15), 1),    # n = 60 < T - 1
        7: (taps_random(64, 16), 3),    # ... decimated
        9: (taps_random(2, 17), 16),    # R = 16
        12: (taps_random(17, 18), 5),
    }, "postdet-c")


TREES = {"a": tree_a, "c": tree_c}


def filtered_leaves(topo):
    return [i for i, v in enumerate(topo.vfos) if len(v.post_taps)]


def detector_leaves(topo):
    return [i for i, v in enumerate(topo.vfos) if v.detector]


def tree_frames(topo, n_frames: int = N_FRAMES, seed: int = 0):
    return dr.tree_frames(topo, n_frames, seed)


def classes(topos) -> set:
    """The classes of filtered leaf-frames a set of trees covers (the issue's list), for the coverage test"""
    out = set()
    for topo in topos:
        for i in filtered_leaves(topo):
            d = topo.vfos[i]
            n, T, R = d.n_stage_out, len(d.post_taps), d.post_decim
            blocks = -(-n // BLOCK)
            if n < T - 1:
                out.add("short")
            if n == BLOCK:
                out.add("one_block")
            if blocks == 2 and n % BLOCK:
                out.add("block_and_partial")
            if blocks >= 2 and BLOCK % R:
                out.add(f"edge_R{R}")
            if blocks >= 3:
                out.add("three_blocks")
            out.add(f"R{R}")
            out.add(f"T{T}")
            out.add("am" if d.detector == dt.AM else "fm")
            out.add("below_main" if d.parent >= 0 and topo.vfos[d.parent].parent < 0 else "below_main_of_main" if d.parent >= 0 else "parentless")
    return out


def run_leaf(d, z, gain, state):
    """The model's record of one frame of detector leaf `d` (a VfoDesc) on its stream `z`: filtered or not"""
    if len(d.post_taps):
        return pd.run(d.detector, z, gain, d.post_taps, d.post_decim, state)
    return dt.run(d.detector, z, gain, state.det)


# ---- crafted streams ----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    frames: tuple            # read-only complex64 streams
    taps: tuple
    decim: int
    gain_am: float = 1.0
    gain_fm: float = 1.0
    gpu: bool = True         # False: a model-only case (a frame length no parent-less leaf can have)
    gain_steps: tuple = ()   # per frame, a factor on both gains (sdrx_set_gains in front of that frame); (): 1 throughout


def _split(x, n=N_CRAFT):
    return tuple(ro(x[f * n:(f + 1) * n]) for f in range(x.size // n))


TONE_IN, TONE_OUT, TONE_T, TONE_CUT, TONE_ATT, TONE_R = 480.0, 4000.0, 129, 1500.0, 60.0, 6


@functools.lru_cache(maxsize=None)
def crafted() -> tuple:
    rng = np.random.default_rng(9111)
    n = N_FRAMES * N_CRAFT
    t = np.arange(n, dtype=np.float64)
    noise = lambda s: s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))  # noqa: E731
    out = []
    # a single non-zero value of pre, six samples in front of a block edge in frame 1: the taps read back, across the edge.  AM: an
    # envelope of 0.5 with one sample of 0.875 (the carrier is 0.5 and a little); FM: one phase step of a quarter turn.
    k = N_CRAFT + BLOCK - 6
    x = np.where(np.arange(n) < k, 0.5 + 0j, 0.5j)
    x[k] = 0.875j
    out.append(Case("impulse", _split(x), taps_random(64, 21), 1))
    out.append(Case("impulse_r3", _split(x), taps_random(17, 22), 3))
    # an AM tone pair inside and outside the pass band of a designed low-pass (pass to 1065 Hz, stop from 1935 Hz), decimated by 6
    env = 0.4 * (1 + 0.3 * np.sin(2 * np.pi * TONE_IN / FS * t) + 0.3 * np.sin(2 * np.pi * TONE_OUT / FS * t))
    out.append(Case("am_tone_pair", _split(env * np.exp(1j * (0.3 + 2 * np.pi * 0.01 * t))), taps_lowpass(TONE_T, TONE_CUT, TONE_ATT), TONE_R, 0.7, 0.7))
    # an FM tone whose deviation steps between frames, a little modulation on it
    step = np.pi * (np.repeat([0.1, 0.4, -0.3, 0.2], N_CRAFT) + 0.05 * np.sin(2 * np.pi * 29.0 / N_CRAFT * t))
    out.append(Case("fm_step", _split(0.5 * np.exp(1j * np.cumsum(step)) + noise(1e-3)), taps_lowpass(64, 3000.0), 2, 0.7, 1.0))
    # a frame of zeros between live ones: the history drains into it, and is zero behind it
    x = 0.3 * np.exp(1j * 2 * np.pi * 0.11 * t) * (1 + 0.4 * np.sin(0.01 * t)) + noise(1e-3)
    x[N_CRAFT:2 * N_CRAFT] = 0
    out.append(Case("zeros", _split(x), taps_random(255, 23), 16))
    # amplitudes that wrap the int16 before the filter and not behind it: pre alternates in sign sample by sample -- AM: an envelope
    # of 0.1 / 3.9, +-1.9 g about the carrier; FM: phase steps of +-0.9 pi at gain 3 -- and the low-pass takes that away
    amp = np.where(np.arange(n) % 2 == 0, 0.1, 3.9)
    ph = np.cumsum(np.where(np.arange(n) % 2 == 0, 0.9 * np.pi, -0.9 * np.pi))
    out.append(Case("wrap", _split(amp * np.exp(1j * ph)), taps_lowpass(64, 3000.0), 2, 1.5, 3.0))
    # the carrier and the gain of the frame before are in the history: a carrier that steps between frames, T = 256
    amp = np.repeat([0.2, 0.6, 0.05, 0.9], N_CRAFT) * (1 + 0.5 * np.sin(2 * np.pi * 11.0 / N_CRAFT * t))
    out.append(Case("carrier_step", _split(amp * np.exp(1j * 2 * np.pi * 0.07 * t) + noise(1e-3)), taps_random(256, 24), 1))
    # ... and a gain that changes between frames (sdrx_set_gains): the history keeps the old gain's values
    out.append(Case("gain_step", _split(amp * np.exp(1j * np.cumsum(0.2 * np.pi * np.sin(0.003 * t))) + noise(1e-3)), taps_random(64, 26), 3, 0.5, 0.75,
                    gain_steps=(1.0, 0.5, 2.0, 1.25)))
    # model only: frames of 48 samples under T = 64 -- the history spans more than one frame
    m = 8 * 48
    tt = np.arange(m, dtype=np.float64)
    x = 0.4 * (1 + 0.5 * np.sin(2 * np.pi * tt / 37.0)) * np.exp(1j * np.cumsum(0.3 * np.pi * np.sin(2 * np.pi * tt / 53.0)))
    out.append(Case("short", _split(x, 48), taps_random(64, 25), 3, gpu=False))
    return tuple(out)


def gpu_cases():
    return [c for c in crafted() if c.gpu]


def case_ids(cases=None):
    return [c.name for c in (crafted() if cases is None else cases)]


def gain_of(case: Case, kind: int, f: int = 0) -> float:
    """The gain frame `f` of the case runs with (a float32 value, as the library holds it)"""
    g = case.gain_am if kind == dt.AM else case.gain_fm
    return float(f32(g * case.gain_steps[f])) if case.gain_steps else float(f32(g))


def model_run(case: Case, kind: int):
    """The model's records of the case's frames for one detector: a list of postdet.run() results"""
    st = pd.State()
    return [pd.run(kind, z, gain_of(case, kind, f), case.taps, case.decim, st) for f, z in enumerate(case.frames)]


# ---- the wrong devices ----------------------------------------------------------------------------------------------------------------
WRONG = ("fma", "descending", "taps_reversed", "hist_zero", "hist_wrong_parity", "halo_zero", "hist_not_merged", "phase_last",
         "filter_int16", "am_halo_this_carrier", "gain_behind", "meter_over_n")
WRONG_KINDS = {w: ((dt.AM,) if w == "am_halo_this_carrier" else (dt.AM, dt.FM)) for w in WRONG}


def _fir(pre, h, R, hist, wrong):
    """postdet.fir with the wrong device's arithmetic: (y, the T - 1 values in front of the next frame)"""
    T = h.size
    if wrong == "taps_reversed":
        h = h[::-1]
    ext = np.concatenate([hist, pre]).astype(f32)
    n = pre.size
    at = np.arange(n // R, dtype=np.int64) * R + (T - 1) + (R - 1 if wrong == "phase_last" else 0)
    acc = np.zeros(at.size, f32)
    order = range(T - 1, -1, -1) if wrong == "descending" else range(T)
    with np.errstate(all="ignore"):
        for t in order:
            x = ext[at - t]
            if wrong == "halo_zero":  # a block with blk >= 1 sees zeros in front of its first sample
                first = (at - (T - 1)) // BLOCK * BLOCK
                x = np.where((first > 0) & (at - (T - 1) - t < first), f32(0), x)
            if wrong == "fma":
                acc = (acc.astype(np.float64) + h[t].astype(np.float64) * x.astype(np.float64)).astype(f32)
            else:
                acc = acc + h[t] * x
    if wrong == "hist_not_merged" and n < T - 1:
        new = np.concatenate([np.zeros(T - 1 - n, f32), pre])
    else:
        new = ext[ext.size - (T - 1):].copy()
    return acc, new


def wrong_run(case: Case, kind: int, wrong: str):
    """The records a wrong device would emit for the case: a list of dicts with `payload` and the meter figures"""
    from sdrreceiver_amd import meter
    h = np.asarray(case.taps, f32)
    T, R = h.size, case.decim
    det = dt.State()
    slots = [np.zeros(T - 1, f32), np.zeros(T - 1, f32)]  # the history slot per frame parity: frame f reads f & 1, writes (f & 1) ^ 1
    e_tail = np.zeros(0, f32)
    out = []
    for f, z in enumerate(case.frames):
        g = f32(gain_of(case, kind, f))
        g_pre = f32(1.0) if wrong == "gain_behind" else g
        pre = pd.pre_of(kind, z, g_pre, det)
        if wrong == "filter_int16":
            pre = (dt.quantise(pre)[0].astype(np.float64) / 32768.0).astype(f32)
        hist = slots[f & 1]
        if wrong == "hist_zero":
            hist = np.zeros(T - 1, f32)
        elif wrong == "hist_wrong_parity":
            hist = slots[(f & 1) ^ 1]
        elif wrong == "am_halo_this_carrier" and f > 0:  # the frame before's envelope under this frame's carrier
            e = dt.envelope(z)
            c = dt.carrier(e)
            tail = np.concatenate([np.zeros(max(T - 1 - e_tail.size, 0), f32), ((e_tail - c).astype(f32) * g).astype(f32)[-(T - 1):]]) if T > 1 else hist
            hist = tail.astype(f32)
        y, new = _fir(pre, h, R, hist, wrong)
        if wrong == "gain_behind":
            y = (y * g).astype(f32)
        slots[(f & 1) ^ 1] = new
        if kind == dt.AM:
            e_tail = dt.envelope(z)
        pay, scaled = dt.quantise(y)
        rec = meter.meters_from_payload(dt._UsbLike, pay, scaled)
        if wrong == "meter_over_n":  # the record of the n values in front of the decimation
            full = _fir(pre, h, 1, hist, "")[0]
            p2, s2 = dt.quantise(full)
            rec = meter.meters_from_payload(dt._UsbLike, p2, s2)
        rec["payload"] = pay
        out.append(rec)
    return out
