"""What the detector leaves' tests share: the small trees, the crafted frames and the wrong devices as variants of the model
(sdrreceiver_amd.detect).

Trees (root fs 30 720).  The leaf-frames cover less than one block of 4096 samples (2048, 3136, 1568), exactly one (4096), two
whole ones (8192), one and a partial one (6272), three and a rest of 256 (12 544) and an odd length (49: the last pair is half
empty); parent-less leaves, leaves below a main and below a main of a main; USB, IQ, AM and FM leaves in one tree.

Crafted frames are STREAMS: the model tests use them as they are.  The GPU tests feed them to parent-less leaves with no decimation
and a mixer at 0 Hz, whose oscillator is a positive real number (the reference's amplitude stabiliser holds it near 0.975): the
leaf's stream is the frame scaled by it, component by component -- zeros stay zeros, signs, axes, diagonals and exact pi steps stay
what they are, 1e-20 still underflows -- and the device is held to the model on that stream."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from sdrreceiver_amd import detect as dt, meter
from sdrreceiver_amd.topology import Topology, VfoDesc

FS = 30720
N_CRAFT = 4096 + 272  # a block and a partial one; a legal raw frame
N_FRAMES = 4
BLOCK = 4096
f32 = np.float32


def ro(x) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.complex64)
    x.setflags(write=False)
    return x


# ---- trees --------------------------------------------------------------------------------------------------------------------------
def _leaf(topic, parent, fs, spb, d, freq, det=0, usb=False, gain=0.5, **kw):
    return VfoDesc(topic=topic, parent=parent, fs=fs, decimate_count=d, mixer_freq=float(freq), demod_usb=usb, gain=float(f32(gain)),
                   samples_per_buffer=spb, detector=det, **kw)


def tree_a() -> Topology:
    """Root frame 16 384.  Parent-less AM and FM leaves of exactly 4096; main 0 (8192 at 15 360 S/s) with an AM leaf of 8192, an FM
    leaf of 4096, a USB leaf, an IQ leaf, and main 3 below it (4096 at 7680 S/s) with an AM leaf of 4096, an FM leaf of 2048 and an
    IQ leaf; a leaf without a topic of either kind (not published)."""
    t = Topology(fs=FS, frame=16384, name="detect-a")
    t.vfos.append(_leaf("", -1, FS, 16384, 1, 3000.0, cstyle=1))                 # 0: main, 8192
    t.vfos.append(_leaf("AM0", 0, FS // 2, 8192, 0, 1200.0, dt.AM))              # 1
    t.vfos.append(_leaf("FM0", 0, FS // 2, 8192, 1, -2100.0, dt.FM))             # 2
    t.vfos.append(_leaf("", 0, FS // 2, 8192, 1, 500.0, cstyle=1))               # 3: main below main, 4096
    t.vfos.append(_leaf("USB0", 0, FS // 2, 8192, 2, 900.0, usb=True, gain=0.05))  # 4
    t.vfos.append(_leaf("IQ0", 0, FS // 2, 8192, 1, -700.0, cstyle=0))           # 5
    t.vfos.append(_leaf("AM1", 3, FS // 4, 4096, 0, 300.0, dt.AM, gain=0.7))     # 6
    t.vfos.append(_leaf("FM1", 3, FS // 4, 4096, 1, -450.0, dt.FM, gain=0.9))    # 7
    t.vfos.append(_leaf("IQ1", 3, FS // 4, 4096, 1, 200.0, cstyle=1, scalecomp=4))  # 8
    t.vfos.append(_leaf("AM2", -1, FS, 16384, 2, -5000.0, dt.AM))                # 9: parent-less, 4096
    t.vfos.append(_leaf("FM2", -1, FS, 16384, 2, 6100.0, dt.FM, gain=1.0))       # 10
    t.vfos.append(_leaf("", 0, FS // 2, 8192, 1, 1500.0, dt.FM))                 # 11: no topic
    return t


def tree_b() -> Topology:
    """Root frame 25 088.  Parent-less AM and FM leaves of 12 544 (three blocks and 256); a main (12 544 at 15 360 S/s) with AM and FM
    leaves of 6272 (a block and a partial one), 3136, 1568 and 49 samples."""
    t = Topology(fs=FS, frame=25088, name="detect-b")
    t.vfos.append(_leaf("", -1, FS, 25088, 1, -2500.0, cstyle=1))                # 0: main, 12 544
    t.vfos.append(_leaf("AM0", -1, FS, 25088, 1, 4000.0, dt.AM))                 # 1
    t.vfos.append(_leaf("FM0", -1, FS, 25088, 1, -4000.0, dt.FM, gain=1.0))      # 2
    t.vfos.append(_leaf("AM1", 0, FS // 2, 12544, 1, 800.0, dt.AM))              # 3: 6272
    t.vfos.append(_leaf("FM1", 0, FS // 2, 12544, 1, -800.0, dt.FM))             # 4
    t.vfos.append(_leaf("AM2", 0, FS // 2, 12544, 2, 1800.0, dt.AM, gain=0.7))   # 5: 3136
    t.vfos.append(_leaf("FM2", 0, FS // 2, 12544, 3, -1800.0, dt.FM, gain=0.7))  # 6: 1568
    t.vfos.append(_leaf("AM3", 0, FS // 2, 12544, 8, 100.0, dt.AM))              # 7: 49
    t.vfos.append(_leaf("FM3", 0, FS // 2, 12544, 8, -100.0, dt.FM))             # 8: 49
    return t


def tree_pair(n: int = N_CRAFT, gain_am: float = 1.0, gain_fm: float = 1.0) -> Topology:
    """Two parent-less leaves with no decimation and a mixer at 0 Hz, AM (0) and FM (1): their stream is the frame times a positive
    real number."""
    t = Topology(fs=FS, frame=n, name="detect-pair")
    t.vfos.append(_leaf("AM", -1, FS, n, 0, 0.0, dt.AM, gain=gain_am))
    t.vfos.append(_leaf("FM", -1, FS, n, 0, 0.0, dt.FM, gain=gain_fm))
    return t


TREES = {"a": tree_a, "b": tree_b}


def detector_leaves(topo):
    return [i for i, v in enumerate(topo.vfos) if v.detector]


def tree_frames(topo, n_frames: int = N_FRAMES, seed: int = 0):
    """Raw frames for a tree: a few AM and FM carriers over noise, continuous across frames"""
    rng = np.random.default_rng(7300 + seed)
    n = topo.frame
    t = np.arange(n_frames * n, dtype=np.float64)
    x = 0.02 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    for k, f0 in enumerate((4200.0, -3900.0, 3900.0, 1800.0, -5000.0, 6100.0, -700.0)):
        fm = 2 * np.pi * (120.0 + 31 * k) / FS
        amp = 0.1 * (1 + 0.5 * np.sin(fm * t))
        ph = 2 * np.pi * f0 / FS * t + 1.5 * np.sin(1.7 * fm * t)
        x += amp * np.exp(1j * ph)
    return [ro(x[f * n:(f + 1) * n]) for f in range(n_frames)]


# ---- crafted streams ----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    frames: tuple            # N_FRAMES read-only complex64 streams of N_CRAFT samples
    gain_am: float = 1.0
    gain_fm: float = 1.0
    signal: tuple = ()       # the detector kinds for which this is a signal case (>= 95 % of the payload non-zero)


def _split(x):
    return tuple(ro(x[f * N_CRAFT:(f + 1) * N_CRAFT]) for f in range(N_FRAMES))


@functools.lru_cache(maxsize=None)
def crafted() -> tuple:
    rng = np.random.default_rng(7311)
    n = N_FRAMES * N_CRAFT
    t = np.arange(n, dtype=np.float64)
    noise = lambda s: s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))  # noqa: E731
    out = []
    for depth in (0.3, 1.0):  # AM tones over noise
        env = 0.4 * (1 + depth * np.sin(2 * np.pi * 37.0 / N_CRAFT * t))
        out.append(Case(f"am_tone_{depth}", _split(env * np.exp(1j * (0.3 + 2 * np.pi * 0.01 * t)) + noise(1e-3)), 0.7, 0.7, (dt.AM,)))
    # an FM tone at +-fs/8 deviation: the phase step swings between +-pi/4 (a quarter of full scale at gain 1)
    step = np.pi / 4 * np.sin(2 * np.pi * 29.0 / N_CRAFT * t)
    out.append(Case("fm_tone", _split(0.5 * np.exp(1j * np.cumsum(step)) + noise(1e-3)), 0.7, 1.0, (dt.FM,)))
    # a carrier that steps between frames (the AM carrier is the frame's own), modulated
    amp = np.repeat([0.2, 0.6, 0.05, 0.9], N_CRAFT) * (1 + 0.5 * np.sin(2 * np.pi * 11.0 / N_CRAFT * t))
    out.append(Case("carrier_step", _split(amp * np.exp(1j * 2 * np.pi * 0.07 * t) + noise(1e-3)), 1.0, 1.0, (dt.AM, dt.FM)))
    # a frame of zeros between two frames of signal: z[-1] = 0 behind it, a carrier of 0 in it
    x = 0.3 * np.exp(1j * 2 * np.pi * 0.11 * t) * (1 + 0.4 * np.sin(0.01 * t)) + noise(1e-3)
    x[N_CRAFT:2 * N_CRAFT] = 0
    out.append(Case("zeros", _split(x)))
    # components of 1e-20: the squares underflow to zero, the products of FM too
    x = (1e-20 * (rng.choice([-1.0, 1.0], n) + 1j * rng.choice([-1.0, 1.0], n)))
    x[::7] = 0.25 + 0.25j
    out.append(Case("tiny", _split(x)))
    # amplitudes that wrap the int16: |pre| up to 6 (AM) and 3 (FM)
    amp = 4.0 * (1 + 0.9 * np.sin(2 * np.pi * 5.0 / N_CRAFT * t))
    out.append(Case("wrap", _split(amp * np.exp(1j * np.cumsum(0.9 * np.pi * np.sin(0.002 * t))) + noise(1e-2)), 1.5, 3.0))
    # a phase step of exactly pi, sample by sample and across the frame and block boundaries
    x = 0.5 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1 + 1j)
    out.append(Case("pi_step", _split(x), 1.0, 1.0))
    # samples on the axes and diagonals of ANG: multiples of 45 degrees with power-of-two magnitudes, in random order
    k = rng.integers(0, 8, n)
    unit = np.array([1, 1 + 1j, 1j, -1 + 1j, -1, -1 - 1j, -1j, 1 - 1j])[k]
    out.append(Case("axes", _split(unit * np.exp2(rng.integers(-6, 3, n))), 0.9, 0.9))
    return tuple(out)


def case_ids():
    return [c.name for c in crafted()]


# ---- the model over a case, and the wrong devices -----------------------------------------------------------------------------------
def model_run(case: Case, kind: int, gain=None):
    """The model's records of the case's frames for one detector: a list of detect.run() results"""
    g = gain if gain is not None else (case.gain_am if kind == dt.AM else case.gain_fm)
    st = dt.State()
    return [dt.run(kind, z, g, st) for z in case.frames]


def _q16(pre):
    return dt.quantise(pre)[0]


def _fm_from(a, b, p, q, gain, swap_ang=False, conj_other=False):
    with np.errstate(all="ignore"):
        d_re = ((a * p).astype(f32) + (b * q).astype(f32)).astype(f32)
        d_im = (((a * q).astype(f32) - (b * p).astype(f32)) if conj_other else ((b * p).astype(f32) - (a * q).astype(f32))).astype(f32)
        x = dt.ang(d_re, d_im) if swap_ang else dt.ang(d_im, d_re)
        return (x * f32(gain)).astype(f32)


WRONG = ("fma_square", "sqrt_of_double_sum", "carrier_prev_frame", "carrier_fp32", "carrier_padded", "zprev_zero", "zprev_wrong_parity",
         "block_start_zero", "conj_other_factor", "ang_swapped", "gain_before_sub", "saturate")
WRONG_KIND = {w: (dt.AM if i < 5 or w == "gain_before_sub" else dt.FM) for i, w in enumerate(WRONG)}
WRONG_KIND["saturate"] = dt.AM


def wrong_run(case: Case, wrong: str):
    """The payloads a wrong device would emit for the case (the detector kind is WRONG_KIND[wrong])"""
    kind = WRONG_KIND[wrong]
    g = f32(case.gain_am if kind == dt.AM else case.gain_fm)
    out, c_prev, lasts = [], f32(0), [0j, 0j]
    for f, z in enumerate(case.frames):
        re, im = z.real.astype(f32), z.imag.astype(f32)
        n = z.size
        with np.errstate(all="ignore"):
            if kind == dt.AM:
                e = dt.envelope(z)
                if wrong == "fma_square":
                    e = np.sqrt((re.astype(np.float64) * re + (im * im).astype(f32)).astype(f32))
                elif wrong == "sqrt_of_double_sum":
                    e = np.sqrt(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2).astype(f32)
                c = dt.carrier(e)
                if wrong == "carrier_prev_frame":
                    c, c_prev = c_prev, c
                elif wrong == "carrier_fp32":
                    c = f32(np.cumsum(e, dtype=f32)[-1] / f32(n))
                elif wrong == "carrier_padded":
                    c = f32(np.float64(dt.carrier_sum(e)) / np.float64(256 * ((n + BLOCK - 1) // BLOCK * BLOCK)))
                if wrong == "gain_before_sub":
                    pre = ((e * g).astype(f32) - f32(c * g)).astype(f32)
                else:
                    pre = ((e - c).astype(f32) * g).astype(f32)
                if wrong == "saturate":
                    out.append(np.clip(np.trunc(pre.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16))
                else:
                    out.append(_q16(pre))
            else:
                zp = lasts[f & 1] if wrong == "zprev_wrong_parity" else 0j if wrong == "zprev_zero" else lasts[(f & 1) ^ 1]
                prev = np.concatenate([np.asarray([zp], np.complex64), z[:-1]])
                if wrong == "block_start_zero":
                    prev[BLOCK::BLOCK] = 0
                p, q = prev.real.astype(f32), prev.imag.astype(f32)
                out.append(_q16(_fm_from(re, im, p, q, g, wrong == "ang_swapped", wrong == "conj_other_factor")))
                lasts[f & 1] = complex(z[-1])  # (the slot frame f + 1 reads is "the other parity's": index f & 1 here)
    return out
