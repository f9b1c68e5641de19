"""Live comparison of the plain-C oracle with the REAL reference build (oracle/_ref), where it
exists (the build container; it also travels to the GPU box as a built .so).  Bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import DC_REFERENCE_REGIMES, SAMPLE_INI, bits, dc_reference_bytes, golden, golden_topology, sha
from oracle import binding as ob
from sdrreceiver_amd import synth, topology as tp

pytestmark = pytest.mark.skipif(not ob.have_reference(), reason="oracle/_ref/libsdrref.so not built")


def _try_reference():
    try:
        ob.load("reference")
    except OSError as e:  # e.g. the Qt runtime is absent on this box
        pytest.skip(f"reference build not loadable here: {e}")


@pytest.mark.parametrize("key,frames", [("config1", 5), ("54w", 2), ("288k", 6), ("compress", 1)])
def test_trees_bit_exact(key, frames):
    _try_reference()
    topo = golden_topology(key)
    trees = {k: ob.build_tree(k, topo) for k in ("port", "reference")}
    lcg = synth.Lcg(3)
    for f in range(frames):
        iq = synth.lcg_frame(topo.frame, lcg) + synth.tone_frame(topo.frame, topo.fs, [(-380000.0, 20.0)], f * topo.frame)
        for k in trees:
            ob.process_roots(trees[k][1], iq)
        for i, v in enumerate(topo.vfos):
            a, b = trees["port"][0][i], trees["reference"][0][i]
            for s in range(v.decimate_count + 1):
                assert np.array_equal(bits(a.stream(s)), bits(b.stream(s))), (key, f, i, s)
            if not topo.children(i):
                if v.demod_usb:
                    assert np.array_equal(a.usb(), b.usb()), (key, f, i)
                else:
                    assert np.array_equal(a.iq(), b.iq()), (key, f, i)
    for i, v in enumerate(topo.vfos):
        a, b = trees["port"][0][i], trees["reference"][0][i]
        assert a.outputRate == b.outputRate
        for which in ("fir_usb", "fir_dec", "hilbert"):
            assert np.array_equal(bits(a.taps(which)), bits(b.taps(which)))


def test_long_audio_filters_bit_exact():
    """Pins the oracle where the GPU test of k_lpf_long relies on it: audio low-pass filters far above the
    shipped profiles' 29-155 taps (filter_bandwidth 500 Hz at 48 kS/s = 925 taps, 35 Hz at 12 kS/s = 3 303
    taps: longer than a frame's 3 000 outputs), 4 frames, against the real reference build."""
    _try_reference()
    t = tp.Topology(fs=1536000, frame=384000, name="longlpf")
    t.vfos.append(tp.VfoDesc(parent=-1, fs=1536000, decimate_count=3, mixer_freq=-496000.0, demod_usb=False, cstyle=1,
                             samples_per_buffer=384000))
    t.vfos.append(tp.VfoDesc(topic="W0", parent=0, fs=192000, decimate_count=2, mixer_freq=-41300.0, filter_bw=500,
                             gain=tp._g(0.05), cstyle=1, samples_per_buffer=48000))
    t.vfos.append(tp.VfoDesc(parent=-1, fs=1536000, decimate_count=2, mixer_freq=484000.0, demod_usb=False, cstyle=1,
                             samples_per_buffer=384000))
    t.vfos.append(tp.VfoDesc(topic="N0", parent=2, fs=384000, decimate_count=5, mixer_freq=110854.0, filter_bw=35,
                             gain=tp._g(0.05), cstyle=1, samples_per_buffer=96000))
    trees = {k: ob.build_tree(k, t) for k in ("port", "reference")}
    assert [len(trees["reference"][0][i].taps("fir_usb")) for i in (1, 3)] == [925, 3303]
    lcg = synth.Lcg(8)
    for f in range(4):
        iq = synth.lcg_frame(t.frame, lcg) + synth.tone_frame(t.frame, t.fs, [(-496000.0 - 40000.0, 30.0)], f * t.frame)
        for k in trees:
            ob.process_roots(trees[k][1], iq)
        for i in (1, 3):
            a, b = trees["port"][0][i], trees["reference"][0][i]
            assert np.array_equal(bits(a.taps("fir_usb")), bits(b.taps("fir_usb")))
            assert np.array_equal(a.usb(), b.usb()), (f, i)


def test_random_designs_and_tables():
    _try_reference()
    rng = np.random.default_rng(5)
    for _ in range(12):
        fs = int(rng.choice([12000, 24000, 48000, 60000, 240000]))
        fc = float(rng.integers(500, fs // 2))
        tw = fc / 4
        assert np.array_equal(bits(ob.low_pass("port", 2, fs, fc, tw)), bits(ob.low_pass("reference", 2, fs, fc, tw)))
    for fs, f in [(48000, 1234), (96000, -47999), (12000, 5999), (24000, -1)]:
        assert np.array_equal(bits(ob.osc_table("port", fs, f)), bits(ob.osc_table("reference", fs, f)))
    for n in (100, 3000, 12000):
        assert np.array_equal(bits(ob.hilbert_taps("port", 125, n)), bits(ob.hilbert_taps("reference", 125, n)))


def test_fir_newest_sample_excluded():
    """FIR::FIRUpdateAndProcess (dsp.cpp:59-71) sums the N samples BEFORE the newest one."""
    _try_reference()
    R = ob.load("reference")
    taps = np.array([1, 10, 100], np.float32)
    x = np.array([1, 2, 3, 4, 5], np.float32)
    y = np.zeros(5, np.float32)
    R.fn("fir_run")(taps.ctypes.data, 3, x.ctypes.data, None, 5, y.ctypes.data)
    # y[m] = 1*x[m-3] + 10*x[m-2] + 100*x[m-1]
    assert list(y) == [0, 100, 210, 321, 432]


def test_ini_parser_matches_qsettings():
    _try_reference()
    R = ob.load("reference")
    fn = R.fn("qsettings_dump")
    fn.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    ini_dir = SAMPLE_INI
    for name in sorted(os.listdir(ini_dir)):
        path = os.path.join(ini_dir, name)
        buf = C.create_string_buffer(1 << 20)
        fn(path.encode(), buf, 1 << 20)
        qs = dict(line.split("=", 1) for line in buf.value.decode().splitlines() if "=" in line)
        mine = tp.parse_ini(open(path, encoding="utf-8", errors="replace").read())
        keys = [k for k in qs if not k.startswith("#") and "/#" not in k]
        assert keys, name
        for k in keys:
            assert mine.get(k) == qs[k], (name, k, mine.get(k), qs[k])


@pytest.mark.parametrize("key,frames", [("config1", 3), ("profile_25e", 3), ("54w", 2)])
def test_shipped_ofast_build_agrees_with_the_o2_build(key, frames):
    """The reference as shipped is compiled -Ofast (SDRReceiver.pro:74-75), which lets the compiler reassociate the
    filter sums; the canonical oracle is the -O2 build.  Both real builds on the same frames: every stream of the tree
    within 1e-5 of max|ref| (measured: 2.5e-7), int16 audio within +-1 LSB (measured: 2 / 120 / 66 samples of
    9 000 / 657 000 / 156 000 differ), taps and NCO start identical."""
    _try_reference()
    if not ob.have_reference_ofast():
        pytest.skip("oracle/_ref/libsdrref_ofast.so not built")
    topo = golden_topology(key)
    a_nodes, a_roots = ob.build_tree("reference", topo)
    b_nodes, b_roots = ob.build_tree("reference_ofast", topo)
    lcg = synth.Lcg(1)
    differing = 0
    for f in range(frames):
        iq = synth.lcg_frame(topo.frame, lcg)
        ob.process_roots(a_roots, iq)
        ob.process_roots(b_roots, iq)
        for i, v in enumerate(topo.vfos):
            a, b = a_nodes[i].stream(), b_nodes[i].stream()
            assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max(), (key, f, i)
            if not topo.children(i) and v.demod_usb:
                pa, pb = a_nodes[i].usb().astype(np.int32), b_nodes[i].usb().astype(np.int32)
                assert np.abs(pa - pb).max() <= 1, (key, f, i)
                differing += int((pa != pb).sum())
    assert differing > 0  # (the two builds DO differ: the tolerance above is not vacuous)


@pytest.mark.parametrize("fixture", ["ofast_config1.npz", "ofast_profile_25e.npz", "ofast_54w.npz"])
def test_ofast_fixtures_are_what_the_ofast_build_produces(fixture):
    """tests/golden/ofast_*.npz regenerate from oracle/_ref/libsdrref_ofast.so (the GPU box and CI hold only the fixtures)."""
    from helpers import OFAST_FIXTURES, check_against_ofast_fixture, golden
    _try_reference()
    if not ob.have_reference_ofast():
        pytest.skip("oracle/_ref/libsdrref_ofast.so not built")
    g = golden(fixture)
    topo = golden_topology(OFAST_FIXTURES[fixture])
    nodes, roots = ob.build_tree("reference_ofast", topo)
    lcg = synth.Lcg(1)
    for f in range(int(g["frames"])):
        ob.process_roots(roots, synth.lcg_frame(topo.frame, lcg))
        for i, v in enumerate(topo.vfos):
            assert np.array_equal(bits(nodes[i].stream()[:256]), bits(g[f"f{f}_v{i}_stream_head"]))
            if not topo.children(i) and v.demod_usb:
                assert sha(nodes[i].usb()) == str(g[f"f{f}_v{i}_pay_sha"])


@pytest.mark.parametrize("case", ["carrier outside every band", "carrier inside VFO05's passband"])
def test_reference_builds_under_a_strong_carrier(case):
    """What "within 1e-5 of the CPU reference" can mean next to a strong carrier: the reference's own two
    builds -- -O2 (the canonical oracle) and -Ofast (as shipped) -- on +-1 LSB of noise under one 100 LSB carrier differ by
    2-4e-6 of max|stream| on the quiet VFOs: the rounding noise of ANY fp32 mixer scales with the total input, the bar with
    the channel's own output.  The figures the GPU test of the tolerance / robust arithmetics is read against
    (helpers.REFERENCE_BUILDS_DIFFER), held here to +-15 %."""
    from helpers import REFERENCE_BUILDS_DIFFER, adversarial_frames
    from sdrreceiver_amd import topology as tp
    _try_reference()
    if not ob.have_reference_ofast():
        pytest.skip("oracle/_ref/libsdrref_ofast.so not built")
    topo = tp.profile_25e()
    a_nodes, a_roots = ob.build_tree("reference", topo)
    b_nodes, b_roots = ob.build_tree("reference_ofast", topo)
    worst, lsb = 0.0, 0
    for f, iq in adversarial_frames(topo, case):
        ob.process_roots(a_roots, iq)
        ob.process_roots(b_roots, iq)
        for i, v in enumerate(topo.vfos):
            a, b = a_nodes[i].stream(), b_nodes[i].stream()
            worst = max(worst, float(np.abs(a - b).max() / np.abs(a).max()))
            if not topo.children(i) and v.demod_usb:
                lsb = max(lsb, int(np.abs(a_nodes[i].usb().astype(np.int32) - b_nodes[i].usb().astype(np.int32)).max()))
    print(f"{case}: -O2 vs -Ofast build of the reference: worst stream difference {worst:.3g} of max|stream|, int16 within {lsb} LSB")
    assert lsb == 1 and abs(worst / REFERENCE_BUILDS_DIFFER[case] - 1.0) < 0.15, worst


# ---- the byte LUT and the DC-bias removal of the REAL sdrj / sdr (oracle/_ref/libsdrjref*.so; one stream per process) --------
needs_sdrj = pytest.mark.skipif(not ob.have_sdrj_reference(), reason="oracle/_ref/libsdrjref.so / libsdrjref_ofast.so not built "
                                "(make -C oracle/ref needs the reference sources)")
SDRJ_BUILDS = [pytest.param(False, id="O2"), pytest.param(True, id="Ofast")]


def _port_dc(u8_frames):
    """bytes -> orc_u8_to_float -> orc_dc_correct from the zero state, frame by frame: the restatement under test."""
    state = np.zeros(2, np.float32)
    out = []
    for b in u8_frames:
        x = ob.u8_to_float(b)
        ob.dc_correct(x, state)
        out.append(x.view(np.complex64))
    return np.concatenate(out)


@needs_sdrj
@pytest.mark.parametrize("ofast", SDRJ_BUILDS)
def test_u8_lut_is_the_real_one(ofast):
    """orc_u8_to_float for all 256 byte values against sdr::floats.at() of a real sdr object (jonti/sdr.cpp:43-49,125;
    sdrj.cpp:158), and the fixture tests/golden/dc_reference.npz carries the same table."""
    b = np.arange(256, dtype=np.uint8)
    real = ob.sdrj_run([128], u8=b, dc=False, ofast=ofast)
    assert np.array_equal(bits(real["lut"]), bits(ob.u8_to_float(b)))
    assert np.array_equal(bits(real["samples"].view(np.float32)), bits(ob.u8_to_float(b)))  # demodData without DC: untouched
    assert np.array_equal(bits(golden("dc_reference.npz")["lut"]), bits(real["lut"]))


@needs_sdrj
@pytest.mark.parametrize("ofast", SDRJ_BUILDS)
@pytest.mark.parametrize("rid", sorted(DC_REFERENCE_REGIMES))
def test_dc_correct_is_the_real_demod_data(rid, ofast):
    """orc_dc_correct (oracle/vfo_oracle.c) against the real sdrj::demodData with setDCCorrection(true), bit for bit, on every
    regime of DC_REFERENCE_REGIMES: the DC_STREAMS regimes of test_gpu_parity.py over 14 x 384 000 samples from the zero
    state (the estimate climbs through its binades and settles), constant 0 / 127 / 255 and alternating 0 / 255 bytes,
    partial last blocks, an offset step half way.  The raw spectrum goes out on calls 5, 9, 13, ... after
    fftVFOSlot("Main") (sdrj.cpp:296-303) and holds that call's DC-corrected samples.  The live build also reproduces the
    committed fixture, so the GPU tests that read only the fixture stay pinned to the real code."""
    n, frames, _, _, _ = DC_REFERENCE_REGIMES[rid]
    u8 = dc_reference_bytes(rid)
    real = ob.sdrj_run([n] * frames, u8=np.concatenate(u8), dc=True, topic="Main", ofast=ofast)
    want = _port_dc(u8)
    assert real["samples"].size == want.size
    bad = np.flatnonzero(bits(real["samples"]) != bits(want))
    assert bad.size == 0, (rid, "first difference at sample", int(bad[0]) if bad.size else None)
    assert list(real["fft_calls"]) == list(range(5, frames + 1, 4)), real["fft_calls"]
    p = 0
    for call, ln in zip(real["fft_calls"], real["fft_len"]):
        assert ln == n
        assert np.array_equal(bits(real["fft_data"][p: p + ln]), bits(want[n * (call - 1): n * call])), (rid, call)
        p += ln
    g = golden("dc_reference.npz")
    for k in range(frames):
        assert sha(real["samples"][n * k: n * (k + 1)]) == str(g[f"{rid}_f{k}_sha"]), (rid, k, "fixture is stale")


@needs_sdrj
@pytest.mark.parametrize("ofast", SDRJ_BUILDS)
def test_real_dc_removal_does_not_depend_on_the_frame_split(ofast):
    """The accumulator carries across demodData calls: frames of unequal lengths that are not multiples of 16 samples
    give the bits of one whole-stream call (and of the oracle)."""
    rid = "capture"
    u8 = np.concatenate(dc_reference_bytes(rid)[:3])
    total = u8.size // 2
    cuts = [1, 15, 1023, 1025, 77777, 4099, 250001, 17, 300000 - 3]
    frames = cuts + [total - sum(cuts)]
    assert frames[-1] > 0 and all(c % 16 for c in cuts)
    whole = ob.sdrj_run([total], u8=u8, dc=True, topic="", ofast=ofast)
    split = ob.sdrj_run(frames, u8=u8, dc=True, topic="", ofast=ofast)
    assert np.array_equal(bits(whole["samples"]), bits(split["samples"]))
    assert np.array_equal(bits(whole["samples"]), bits(_port_dc([u8])))


@needs_sdrj
def test_python_host_dc_correct_is_the_real_one():
    """receiver._dc_correct (the mirror sdrj's float path) against the real demodData: from the zero state, and from the
    oracle's state after 12 frames of the dongle-like and pinned regimes (a settled estimate), on frames of 40 000 samples."""
    from sdrreceiver_amd.receiver import _dc_correct
    for rid in ("capture", "opposite", "step"):
        n, frames, _, _, _ = DC_REFERENCE_REGIMES[rid]
        u8 = dc_reference_bytes(rid)
        real = ob.sdrj_run([n] * frames, u8=np.concatenate(u8), dc=True, topic="")["samples"]
        state = np.zeros(2, np.float32)
        for k in range(frames):
            if k in (0, frames - 2):
                x = ob.u8_to_float(u8[k][: 2 * 40000])
                s = state.copy()
                _dc_correct(x, s)
                assert np.array_equal(bits(x.view(np.complex64)), bits(real[n * k: n * k + 40000])), (rid, k)
            ob.dc_correct(ob.u8_to_float(u8[k]), state)
