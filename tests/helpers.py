"""Shared helpers for the test-suite (test infrastructure)."""
from __future__ import annotations

import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the reference's shipped INI profiles (its sample_ini/ folder), kept as data fixtures
SAMPLE_INI = os.path.join(GOLDEN, "sample_ini")


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def topo_54w_golden():
    """The tree tests/golden/make_golden.py used for profile_54w.npz."""
    from sdrreceiver_amd import topology as tp
    t = tp.config4(6)
    t.vfos.append(tp.VfoDesc(topic="VFO41", parent=0, fs=240000, decimate_count=2, mixer_freq=105571.0,
                             late_decimate=5, filter_bw=0, gain=tp._gain_pct(4), cstyle=1,
                             samples_per_buffer=60000))
    t.vfos.append(tp.VfoDesc(topic="VFO44", parent=0, fs=240000, decimate_count=2, mixer_freq=-74731.0,
                             late_decimate=5, filter_bw=4000, gain=tp._gain_pct(4), cstyle=1,
                             samples_per_buffer=60000))
    return t


def topo_compress_golden():
    from sdrreceiver_amd import topology as tp
    t = tp.Topology(fs=1536000, frame=384000, name="compress")
    for cs, sc, top in ((1, 1, "IQ4A"), (1, 16, "IQ4B"), (0, 1, "IQ8")):
        t.vfos.append(tp.VfoDesc(topic=top, parent=-1, fs=1536000, decimate_count=3, mixer_freq=-496000.0,
                                 demod_usb=False, cstyle=cs, scalecomp=sc, samples_per_buffer=384000))
    return t


def topo_288k_golden():
    from sdrreceiver_amd import topology as tp
    t = tp.Topology(fs=288000, frame=57600, bufsplit=5, name="288k")
    t.vfos.append(tp.VfoDesc(parent=-1, fs=288000, decimate_count=0, mixer_freq=0.0, demod_usb=False, cstyle=1,
                             samples_per_buffer=57600))
    t.vfos.append(tp.VfoDesc(topic="VFO51", parent=0, fs=288000, decimate_count=0, mixer_freq=54578.0,
                             late_decimate=6, filter_bw=10000, gain=tp._gain_pct(4), cstyle=1,
                             samples_per_buffer=57600))
    return t


GOLDEN_TREES = {
    # fixture file -> (topology factory, frames)
    "config1.npz": ("config1", 6),
    "profile_25e.npz": ("profile_25e", 5),
    "profile_54w.npz": ("54w", 5),
    "compress.npz": ("compress", 2),
    "profile_288k.npz": ("288k", 6),
}


def golden_topology(key):
    from sdrreceiver_amd import topology as tp
    return {"config1": tp.config1, "profile_25e": tp.profile_25e, "54w": topo_54w_golden,
            "compress": topo_compress_golden, "288k": topo_288k_golden}[key]()


# ---- the sdr_25E shapes of the retune, meter and device-frame tests ------------------------------------------------------------
def tree_1536():
    """The sdr_25E shapes: two mains; d=5 12 k subs on main 1 (one with the 4 kHz low-pass), d=2 48 k subs on main 2 (10 kHz
    low-pass, none, and a 1 kHz low-pass of more than 256 taps: k_lpf_long)."""
    from sdrreceiver_amd.topology import Topology, VfoDesc
    t = Topology(fs=1536000, frame=384000, bufsplit=4, center_frequency=1545600000, name="retune-1536")
    m = dict(parent=-1, fs=1536000, demod_usb=False, cstyle=1, samples_per_buffer=384000)
    t.vfos.append(VfoDesc(decimate_count=2, mixer_freq=484000.0, **m))
    t.vfos.append(VfoDesc(decimate_count=3, mixer_freq=-496000.0, **m))
    a = dict(parent=0, fs=384000, decimate_count=5, gain=float(np.float32(0.05)), cstyle=1, samples_per_buffer=96000)
    t.vfos.append(VfoDesc(topic="VFO01", mixer_freq=110854.0, filter_bw=4000, **a))
    t.vfos.append(VfoDesc(topic="VFO06", mixer_freq=-3063.0, **a))
    b = dict(parent=1, fs=192000, decimate_count=2, gain=float(np.float32(0.03)), cstyle=1, samples_per_buffer=48000)
    t.vfos.append(VfoDesc(topic="VFO19", mixer_freq=-41300.0, filter_bw=10000, **b))
    t.vfos.append(VfoDesc(topic="VFO16", mixer_freq=11400.0, **b))
    t.vfos.append(VfoDesc(topic="VFO25", mixer_freq=-61500.0, filter_bw=1000, **b))
    return t


def tree_mixed():
    """tree_1536 (d=5 and d=2 USB subs, the 10 kHz low-pass, a 1 kHz low-pass of more than 256 taps:
    k_lpf_long) plus two childless mains: compress() with cstyle 0 / scalecomp 1 and cstyle 1 / scalecomp 4."""
    from sdrreceiver_amd.topology import VfoDesc
    t = tree_1536()
    t.name = "meter-1536"
    t.vfos.append(VfoDesc(topic="IQ0", parent=-1, fs=1536000, decimate_count=4, mixer_freq=200000.0, demod_usb=False,
                          cstyle=0, scalecomp=1, samples_per_buffer=384000))
    t.vfos.append(VfoDesc(topic="IQ1", parent=-1, fs=1536000, decimate_count=3, mixer_freq=-300000.0, demod_usb=False,
                          cstyle=1, scalecomp=4, samples_per_buffer=384000))
    return t


# ---- the reference AS SHIPPED (-Ofast, SDRReceiver.pro:74-75): tests/golden/ofast_*.npz ------------------------------
OFAST_FIXTURES = {"ofast_config1.npz": "config1", "ofast_profile_25e.npz": "profile_25e", "ofast_54w.npz": "54w"}
OFAST_REL_TOL = 1e-5  # north_star: "within 1e-5 relative float tolerance"


def check_against_ofast_fixture(g, topo, f, stream_of, payload_of, o2_payload_of=None):
    """Frame `f` of an implementation (`stream_of(i)` -> complex64 or None, `payload_of(i)` -> int16) against the -Ofast
    fixture `g`: every final complex stream within 1e-5 of max|ref| at the stored positions (head + every 128th sample),
    every int16 payload within +-1 LSB of the shipped build's.  The fixture holds that payload as a patch against the -O2
    build's: `o2_payload_of(i)` must return the -O2 payload bit for bit (default: the implementation itself, i.e. it
    claims to BE the -O2 result) -- patched, its sha must be the -Ofast payload's, which proves the reconstruction and,
    for the default, that the implementation equals the shipped build everywhere outside the patch.
    Returns (worst relative stream error, patched samples, payload samples)."""
    worst, patched, total = 0.0, 0, 0
    for i, v in enumerate(topo.vfos):
        z = stream_of(i)
        if z is not None:
            scale = float(g[f"f{f}_v{i}_stream_absmax"])
            e = max(float(np.abs(z[:256] - g[f"f{f}_v{i}_stream_head"]).max()), float(np.abs(z[::128] - g[f"f{f}_v{i}_stream_every128"]).max()))
            assert e <= OFAST_REL_TOL * scale, (f, i, "stream", e / scale)
            worst = max(worst, e / scale)
        if not topo.children(i) and v.demod_usb:
            got = payload_of(i)
            shipped = (o2_payload_of(i) if o2_payload_of else got).copy()
            idx, val = g[f"f{f}_v{i}_pay_idx"], g[f"f{f}_v{i}_pay_val"]
            shipped[idx] = val
            assert sha(shipped) == str(g[f"f{f}_v{i}_pay_sha"]), (f, i, "not the -Ofast payload: the -O2 payload it was rebuilt from is not bit-exact")
            assert np.abs(got.astype(np.int32) - shipped.astype(np.int32)).max() <= 1, (f, i, "payload beyond 1 LSB of the shipped build")
            patched += idx.size
            total += got.size
    return worst, patched, total


# ---- the capture-like stream (tests/golden/capture_25e.npz; BASELINE.json north_star: "on recorded IQ") -------------------------
def capture_frames():
    """(fixture, topology, [dongle bytes of frame 0, 1, ...]): sdrreceiver_amd.synth.capture_like_u8 regenerated and checked
    against the sha256 the fixture was made from (another numpy / libm could round a sample differently: then the fixture
    does not apply and the tests say so instead of comparing apples with pears)."""
    import pytest
    from sdrreceiver_amd import synth, topology as tp
    g = golden("capture_25e.npz")
    topo = tp.profile_25e()
    n = int(g["frames"])
    u8 = synth.capture_like_u8(n, topo.frame, topo.fs)
    if hashlib.sha256(u8.tobytes()).hexdigest() != str(g["input_sha256"]):
        pytest.skip("capture_like_u8 does not reproduce the bytes capture_25e.npz was generated from on this numpy build")
    return g, topo, [u8[2 * topo.frame * f: 2 * topo.frame * (f + 1)] for f in range(n)]


def check_capture_frame_exact(g, topo, f, stream_of, payload_of):
    """Frame `f` against the -O2 reference's outputs in the fixture: sha256 of every final complex stream and of every int16
    payload (stream_of(i) may return None where an implementation keeps no decimate[0])."""
    for i, v in enumerate(topo.vfos):
        z = stream_of(i)
        assert z is None or sha(z) == str(g[f"f{f}_v{i}_stream_sha"]), (f, i, "stream")
        if not topo.children(i):
            assert sha(payload_of(i)) == str(g[f"f{f}_v{i}_pay_sha"]), (f, i, "payload")


# ---- seeded random trees (tests/test_gpu_parity.py, tests/test_dropin_qt.py, tools/dropin_run.py random:<seed>) ----------
def random_topology(rng):
    """A random tree inside the library's documented restrictions: 1-3 levels, depths 0-4, frames of
    16 * 2^k * m samples (last chunk partial), rates 1x-4x the frame, USB leaves with and without the
    audio low-pass and the /5 or /6 late decimation, IQ leaves with both compress styles."""
    from sdrreceiver_amd.topology import Topology, VfoDesc, _g
    depth_budget = 7
    n_root = 16 * (1 << depth_budget) * int(rng.integers(3, 13))  # 6 144 .. 24 576, divisible by 16 * 2^7
    fs_root = n_root * int(rng.choice([1, 2, 4]))
    t = Topology(fs=fs_root, frame=n_root, name="rnd")

    def leaf(parent, fs, n, used):
        d = int(rng.integers(0, min(4, depth_budget - used) + 1))
        rate, n_out = fs >> d, n >> d
        usb = rng.random() < 0.75
        late = 0
        if usb and rng.random() < 0.3:
            for L in (5, 6):
                if n_out % L == 0 and (n_out // L) >= 64 and rate % L == 0:
                    late = L
                    break
        out_rate = rate // late if late else rate
        bw = int(out_rate / rng.uniform(2.3, 12.0)) if (usb and rng.random() < 0.5) else 0
        t.vfos.append(VfoDesc(topic=f"L{len(t.vfos):03d}"[:5], parent=parent, fs=fs, decimate_count=d,
                                 mixer_freq=float(int(rng.integers(-fs // 2 + 1, fs // 2))), demod_usb=usb, late_decimate=late,
                                 filter_bw=bw, gain=_g(float(rng.uniform(0.01, 0.08))), cstyle=int(rng.integers(0, 2)),
                                 scalecomp=int(rng.choice([1, 2, 4])), samples_per_buffer=n))

    def inner(parent, fs, n, used, level):
        d = int(rng.integers(0, 3))
        t.vfos.append(VfoDesc(parent=parent, fs=fs, decimate_count=d, mixer_freq=float(int(rng.integers(-fs // 2 + 1, fs // 2))),
                                 demod_usb=False, cstyle=1, samples_per_buffer=n))
        me = len(t.vfos) - 1
        for _ in range(int(rng.integers(1, 4))):
            if level < 2 and rng.random() < 0.3:
                inner(me, fs >> d, n >> d, used + d, level + 1)
            else:
                leaf(me, fs >> d, n >> d, used + d)

    for _ in range(int(rng.integers(1, 4))):
        if rng.random() < 0.7:
            inner(-1, fs_root, n_root, 0, 1)
        else:
            leaf(-1, fs_root, n_root, 0)
    return t


# ---- the adversarial input of VERDICT r5 item 3: a quiet band under one strong carrier -------------------------------------------
# (Hz from the raw centre, LSB): outside both main VFOs' bands / 2 kHz into VFO05's 12 kHz channel -- its neighbours under main
# VFO 1 get it as an interferer 40 dB over their own noise after the main VFO's decimation
ADVERSARIAL_CARRIERS = {"carrier outside every band": (100000.0, 100.0), "carrier inside VFO05's passband": (-483866.0, 100.0)}
# What the reference's OWN two builds (-O2, the canonical oracle, and -Ofast, as shipped: SDRReceiver.pro:74-75) differ by on these
# inputs, max|a - b| / max|a| over every final complex stream of the sdr_25E tree, 5 frames (measured by
# tests/test_oracle_vs_reference.py::test_reference_builds_under_a_strong_carrier, which holds the figures to +-15 %): rounding
# noise of the fp32 mixer scales with the TOTAL input, the bar with the quiet channel's own output.
REFERENCE_BUILDS_DIFFER = {"carrier outside every band": 2.14e-6, "carrier inside VFO05's passband": 4.01e-6}


def adversarial_frames(topo, case, n_frames=5, seed=606):
    """sdr_25E-shaped input: +-1 LSB of noise and ONE carrier of 100 LSB, phase-continuous over the frames"""
    from sdrreceiver_amd import synth
    f_c, a_c = ADVERSARIAL_CARRIERS[case]
    rng = np.random.default_rng(seed)
    for f in range(n_frames):
        yield f, synth.tone_frame(topo.frame, topo.fs, [(f_c, a_c)], f * topo.frame) + rng.integers(-1, 2, 2 * topo.frame).astype(np.float32)


# ---- tests/golden/dc_reference.npz: the DC-bias removal of the REAL sdrj::demodData (sdrj.cpp:266-305) ---------------------------
# Byte streams from the integer generator synth.Lcg (no numpy RNG: the fixture does not depend on its version).  A regime is
# (frame length, frames, kind, parameters); "noise" is an offset (di, dq) plus Lcg noise of standard deviation sigma per
# component, "pattern" a sequence of per-frame byte patterns, "step" two noise regimes, the second from half way through.
DC_REFERENCE_REGIMES = {
    # the DC_STREAMS regimes of test_gpu_parity.py, 14 frames of 384 000 samples from the zero state
    "capture": (384000, 14, "noise", (1.3, -0.7, 7.0), "offsets of the capture-like stream"),
    "binade": (384000, 14, "noise", (0.25, 4.94, 7.0), "next to a binade boundary and a rounding threshold"),
    "opposite": (384000, 14, "noise", (100.0, -120.0, 10.0), "large, opposite signs (one estimate pinned to its threshold)"),
    "pinned": (384000, 14, "noise", (30.0, -2.0, 3.0), "an offset ten times the noise (pinned)"),
    "nooffset": (384000, 14, "noise", (0.0, 0.02, 7.0), "no offset at all (the estimate wanders through zero)"),
    "quiet": (384000, 14, "noise", (1.3, -0.7, 2.0), "quiet front end"),
    "strong": (384000, 14, "noise", (1.3, -0.7, 50.0), "strong carriers"),
    # constant and extreme bytes; 480 000 = 468.75 blocks of 1 024 (a partial last block)
    "const0": (480000, 3, "pattern", ("0",), "constant 0"),
    "const127": (480000, 3, "pattern", ("127",), "constant 127"),
    "const255": (480000, 3, "pattern", ("255",), "constant 255"),
    "alt": (480000, 3, "pattern", ("alt",), "alternating 0 / 255 samples"),
    "extremes": (57600, 8, "pattern", ("255", "255", "0", "0", "127", "127", "alt", "alt"), "extremes in turn, short frames"),
    "step": (384000, 8, "step", ((20.0, -10.0, 5.0), (-30.0, 15.0, 5.0)), "an offset step half way through"),
    "capture480": (480000, 6, "noise", (1.3, -0.7, 7.0), "capture-like offsets, partial last block"),
    "lcg": (384000, 9, "lcg", (), "the synthetic LCG frames of host/demo.cpp (components -8 ... 8)"),
}


def _lcg_noise(lcg, n, sigma):
    """n values of mean 0 and standard deviation sigma: the sum of four 24-bit uniforms on [-1/2, 1/2) (exact in float64),
    scaled by sigma * sqrt(3)."""
    u = (lcg.draw(4 * n) >> np.uint32(8)).astype(np.float64) / float(1 << 24) - 0.5
    return u.reshape(n, 4).sum(axis=1) * (sigma * np.sqrt(3.0))


def _noise_bytes(lcg, n_complex, di, dq, sigma):
    z = _lcg_noise(lcg, 2 * n_complex, sigma)
    z[0::2] += di
    z[1::2] += dq
    return np.clip(np.rint(z) + 127, 0, 255).astype(np.uint8)


def dc_reference_bytes(rid):
    """The dongle bytes of regime `rid`, one array per frame (2 * frame bytes each)."""
    from sdrreceiver_amd import synth
    n, frames, kind, par, _ = DC_REFERENCE_REGIMES[rid]
    lcg = synth.Lcg(1000 + sorted(DC_REFERENCE_REGIMES).index(rid))
    out = []
    for f in range(frames):
        if kind == "noise":
            out.append(_noise_bytes(lcg, n, *par))
        elif kind == "step":
            out.append(_noise_bytes(lcg, n, *par[0 if f < frames // 2 else 1]))
        elif kind == "lcg":
            if f == 0:
                lcg = synth.Lcg(1)  # host/demo.cpp's stream: x = 1 at the start
            out.append(synth.lcg_frame_u8(n, lcg))
        else:
            p = par[f % len(par)]
            if p == "alt":
                b = np.zeros(2 * n, np.uint8)
                b[0::4] = 255
                b[1::4] = 255
            else:
                b = np.full(2 * n, int(p), np.uint8)
            out.append(b)
    return out


def fnv1a64(a) -> int:
    """FNV-1a 64 of the bytes of `a` (host/demo.cpp prints it for every message and spectrum)."""
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h
