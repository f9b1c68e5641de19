"""Signed 8- and 16-bit sample ingest (sdrx_*_fmt, SDRX_FMT_CS8 / SDRX_FMT_CS16) with the DC-bias removal on the device.

The oracle of every new format is the existing one fed floats: ingest.to_float (the table of include/sdrx.h), ob.dc_correct
and ob.process_roots.  Two embeddings pin the formats to the REAL reference through fixtures already committed: for bytes
b <= 254, v8 = b - 127 and v16 = 256 (b - 127) are exactly the floats of the byte (tests/test_ingest_formats_model.py asserts
both, and that every regime used here holds no byte 255).  Everything is held bit for bit, except option dc_blocked_scan,
which is held to the bound and the model test_gpu_parity.py holds bytes to."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import bits, golden, sha, dc_reference_bytes
from oracle import binding as ob
from sdrreceiver_amd import _lib, ingest, topology as tp
from test_ingest_formats_model import EMBEDDED_REGIMES, embed_s8, embed_s16

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5  # test_gpu_parity.py's _check_tolerance
EMBED = {ingest.CS8: embed_s8, ingest.CS16: embed_s16}
NAME = {ingest.CU8: "cu8", ingest.CS8: "cs8", ingest.CS16: "cs16"}


@pytest.fixture(scope="module")
def Receiver():
    from sdrreceiver_amd.receiver import Receiver as R
    return R


def _code(call):
    from sdrreceiver_amd.receiver import SdrxError
    with pytest.raises(SdrxError) as e:
        call()
    return e.value.code, str(e.value)


def _check_exact(rx, nodes, topo, ctx):
    """test_gpu_parity.py's comparison of a whole tree with the oracle"""
    for i, v in enumerate(topo.vfos):
        got = rx.stream(i, missing_ok=True)
        assert got is None or np.array_equal(bits(got), bits(nodes[i].stream())), (ctx, i, "stream")
        if not topo.children(i):
            want = nodes[i].usb() if v.demod_usb else nodes[i].iq()
            assert np.array_equal(rx.output(i), want), (ctx, i, "payload")


def _check_twin(rx, twin, topo, ctx):
    """two receivers after the same frame: every payload, every stream and the raw frame bit for bit"""
    assert np.array_equal(bits(rx.raw()), bits(twin.raw())), (ctx, "raw")
    for i in range(len(topo.vfos)):
        a, b = rx.stream(i, missing_ok=True), twin.stream(i, missing_ok=True)
        assert (a is None) == (b is None) and (a is None or np.array_equal(bits(a), bits(b))), (ctx, i, "stream")
        if not topo.children(i):
            assert np.array_equal(rx.output(i), twin.output(i)), (ctx, i, "payload")


def _random_samples(rng, fmt, n_complex):
    """full-range samples of a signed format, both ends of the range forced in"""
    info = np.iinfo(ingest.FORMATS[fmt])
    v = rng.integers(info.min, info.max + 1, 2 * n_complex, dtype=ingest.FORMATS[fmt])
    v[[0, 3, -1]] = info.min
    v[[1, 2, -2]] = info.max
    return v


# ------------------------------------------------------------------------------------------- 1. embedding, no DC
def test_embedded_bytes_without_dc_are_the_byte_path(Receiver):
    topo = tp.config2()
    rxs = {fmt: Receiver.from_topology(topo, keep_streams=True) for fmt in (ingest.CU8, ingest.CS8, ingest.CS16)}
    nodes, roots = ob.build_tree("port", topo)
    rng = np.random.default_rng(21)
    for f in range(3):
        b = rng.integers(0, 255, 2 * topo.frame, dtype=np.uint8)
        b[:4] = (0, 254, 254, 0)
        rxs[ingest.CU8].process_u8(b)
        rxs[ingest.CS8].process_fmt(embed_s8(b))
        rxs[ingest.CS16].process_fmt(embed_s16(b))
        ob.process_roots(roots, ob.u8_to_float(b))
        for fmt in (ingest.CS8, ingest.CS16):
            _check_twin(rxs[fmt], rxs[ingest.CU8], topo, (NAME[fmt], f))
            assert rxs[fmt].published == rxs[ingest.CU8].published, (NAME[fmt], f)
            _check_exact(rxs[fmt], nodes, topo, (NAME[fmt], f))
    for rx in rxs.values():
        rx.close()


# ------------------------------------------------------------------------------------------- 2. genuine samples
@pytest.mark.parametrize("correct_dc", [False, True])
@pytest.mark.parametrize("fmt", [ingest.CS16, ingest.CS8], ids=NAME.get)
def test_full_range_samples_against_the_oracle(Receiver, fmt, correct_dc):
    topo = tp.config2()
    rx = Receiver.from_topology(topo)
    nodes, roots = ob.build_tree("port", topo)
    rng = np.random.default_rng(22 + fmt)
    state = np.zeros(2, np.float32)
    for f in range(3):
        v = _random_samples(rng, fmt, topo.frame)
        rx.process_fmt(v, correct_dc=correct_dc)
        iq = ingest.to_float(v)
        if correct_dc:
            ob.dc_correct(iq, state)
        ob.process_roots(roots, iq)
        assert np.array_equal(bits(rx.raw()), bits(iq.view(np.complex64))), (NAME[fmt], correct_dc, f, "raw")
        _check_exact(rx, nodes, topo, (NAME[fmt], correct_dc, f))
    rx.close()


# ------------------------------------------------------------------------------------------- 3. frame shapes
SHAPES = [1024, 1040, 1296, 2048, 4368, 8704, 16368, 20496, 69968]  # test_dc_bias_removal_on_frames_of_every_shape's list
SHAPE_CASES = [(n, True) for n in SHAPES] + [(n, False) for n in (1040, 4368, 69968)]


def _shape_tree(n, wide):
    """That test's two-root tree (level 0 reads the frame where it lies: root_direct), or six parent-less VFOs (a wide level 0)."""
    t = tp.Topology(fs=4 * n, frame=n, name=f"fmt{n}{'w' if wide else ''}")
    t.vfos.append(tp.VfoDesc(topic="DC0", parent=-1, fs=4 * n, decimate_count=1, mixer_freq=float(n // 3), filter_bw=0,
                             gain=tp._g(0.05), cstyle=1, samples_per_buffer=n))
    t.vfos.append(tp.VfoDesc(topic="IQ0", parent=-1, fs=4 * n, decimate_count=0, mixer_freq=-float(n // 5), demod_usb=False,
                             cstyle=0, samples_per_buffer=n))
    for j in range(4 if wide else 0):
        usb = j % 2 == 0
        t.vfos.append(tp.VfoDesc(topic=f"W{j}", parent=-1, fs=4 * n, decimate_count=1 if usb else 0, mixer_freq=float((j + 1) * (n // 9)),
                                 demod_usb=usb, filter_bw=0, gain=tp._g(0.05), cstyle=1 if usb else 0, samples_per_buffer=n))
    return t


@pytest.mark.parametrize("n,speculative", SHAPE_CASES)
def test_frames_of_every_shape(Receiver, n, speculative):
    """(As in the test the list comes from, a length whose last chunk would hold fewer than 256 samples grows by 256: the
    library takes no other.)"""
    if 0 < n % 1024 < 256:
        n += 256
    for wide in (False, True):
        t = _shape_tree(n, wide)
        for fmt in (ingest.CS8, ingest.CS16):
            rx = Receiver.from_topology(t, exact=True, dc_speculative=speculative)
            nodes, roots = ob.build_tree("port", t)
            rng = np.random.default_rng(n + fmt)
            state = np.zeros(2, np.float32)
            for f in range(3):
                v = _random_samples(rng, fmt, n)
                v[1::2] = v[1::2] // 4 + (60 << (8 * (fmt - 1)))  # a DC offset worth removing
                rx.process_fmt(v, correct_dc=True)
                iq = ingest.to_float(v)
                ob.dc_correct(iq, state)
                ob.process_roots(roots, iq)
                ctx = (n, "wide" if wide else "direct", NAME[fmt], speculative, f)
                assert np.array_equal(bits(rx.raw()), bits(iq.view(np.complex64))), (ctx, "raw frame after the DC-bias removal")
                _check_exact(rx, nodes, t, ctx)
            rx.close()
            for r in roots:
                r.free()


# ------------------------------------------------------------------------------------------- 4. the real sdrj through the embedding
@functools.lru_cache(maxsize=None)
def _regime(rid):
    return dc_reference_bytes(rid)


def _check_dc_fixture(g, rid, k, z, ctx):
    """test_gpu_parity.py's three figures: first 64 samples, every 4096th, sha256 of all bits"""
    n = int(g[f"{rid}_frame"])
    assert z.size == n, ctx
    assert np.array_equal(bits(z[:64]), bits(g[f"{rid}_f{k}_head"])), (ctx, "first 64 samples")
    assert np.array_equal(bits(z[::4096]), bits(g[f"{rid}_f{k}_every4096"])), (ctx, "every 4096th sample")
    assert sha(z) == str(g[f"{rid}_f{k}_sha"]), (ctx, "sha256 of the DC-corrected frame")


def _dc_topology(n):
    t = tp.Topology(fs=4 * n, frame=n, name=f"dcfmt{n}")
    t.vfos.append(tp.VfoDesc(topic="M", parent=-1, fs=4 * n, decimate_count=2, mixer_freq=float(n // 7), demod_usb=False, cstyle=1,
                             samples_per_buffer=n))
    return t


@pytest.mark.parametrize("fmt", [ingest.CS8, ingest.CS16], ids=NAME.get)
@pytest.mark.parametrize("rid,kw", [(rid, {}) for rid in EMBEDDED_REGIMES] + [("lcg", {"dc_blocks_per_step": 1}), ("lcg", {"dc_blocks_per_step": 8})],
                         ids=lambda p: p if isinstance(p, str) else "-".join(f"{k}={v}" for k, v in p.items()) or "default")
def test_dc_removal_of_embedded_bytes_is_the_real_sdrj(Receiver, rid, kw, fmt):
    g = golden("dc_reference.npz")
    u8 = _regime(rid)
    rx = Receiver.from_topology(_dc_topology(u8[0].size // 2), exact=True, **kw)
    for k, b in enumerate(u8):
        rx.process_fmt(EMBED[fmt](b), correct_dc=True)
        _check_dc_fixture(g, rid, k, rx.raw(), (rid, NAME[fmt], kw, k))
    rx.close()


# ------------------------------------------------------------------------------------------- 5. formats alternating
def test_one_accumulator_for_every_format(Receiver):
    g = golden("dc_reference.npz")
    u8 = _regime("lcg")
    rx = Receiver.from_topology(_dc_topology(u8[0].size // 2), exact=True)
    for k, b in enumerate(u8):
        fmt = (ingest.CU8, ingest.CS8, ingest.CS16)[k % 3]
        rx.process_fmt(b if fmt == ingest.CU8 else EMBED[fmt](b), correct_dc=True)
        _check_dc_fixture(g, "lcg", k, rx.raw(), ("alternating", NAME[fmt], k))
    rx.close()


# ------------------------------------------------------------------------------------------- 6. extremes
@pytest.mark.parametrize("fmt", [ingest.CS16, ingest.CS8], ids=NAME.get)
def test_extreme_samples(Receiver, fmt):
    n = 57600
    info = np.iinfo(ingest.FORMATS[fmt])
    alt = np.full(2 * n, info.max, ingest.FORMATS[fmt])
    alt[0::4] = info.min
    alt[1::4] = info.min
    patterns = [np.full(2 * n, info.min, ingest.FORMATS[fmt]), np.full(2 * n, info.max, ingest.FORMATS[fmt])]
    if fmt == ingest.CS16:
        patterns.append(alt)
    rx = Receiver.from_topology(_dc_topology(n), exact=True)
    state = np.zeros(2, np.float32)
    for k, v in enumerate(p for p in patterns for _ in range(2)):
        rx.process_fmt(v, correct_dc=True)
        iq = ingest.to_float(v)
        ob.dc_correct(iq, state)
        assert np.array_equal(bits(rx.raw()), bits(iq.view(np.complex64))), (NAME[fmt], k)
    rx.close()


# ------------------------------------------------------------------------------------------- 7. fractional samples
def test_fractional_int16_samples(Receiver):
    """int16 noise whose values are no multiples of 256 -- products fl(1e-6f * x) of samples with up to 16 significant bits,
    which bytes never produce.  The speculative chain's counters of the last frame are printed, not bounded: how often such
    samples tie has not been measured before."""
    n = 384000
    rx = Receiver.from_topology(_dc_topology(n), exact=True)
    rng = np.random.default_rng(77)
    state = np.zeros(2, np.float32)
    prev = rx.stats()
    for f in range(6):
        z = rng.standard_normal(2 * n) * (7 * 256)
        z[0::2] += 1.3 * 256 + 77
        z[1::2] += -0.7 * 256 - 31
        v = np.clip(np.rint(z), -32768, 32767).astype(np.int16)
        rx.process_fmt(v, correct_dc=True)
        iq = ingest.to_float(v)
        ob.dc_correct(iq, state)
        assert np.array_equal(bits(rx.raw()), bits(iq.view(np.complex64))), f
        st = rx.stats()
        assert st["dc_blocks"] - prev["dc_blocks"] == 2 * 375, (f, st, prev)
        print(f"frame {f}: dc_fallback_blocks +{st['dc_fallback_blocks'] - prev['dc_fallback_blocks']}, "
              f"dc_retried_blocks +{st['dc_retried_blocks'] - prev['dc_retried_blocks']} of 750")
        prev = st
    rx.close()


# ------------------------------------------------------------------------------------------- 8. dc_blocked_scan
def _check_tolerance(rx, nodes, topo, ctx):
    for i, v in enumerate(topo.vfos):
        ref = nodes[i].stream()
        got = rx.stream(i, missing_ok=True)
        scale = float(np.abs(ref).max())
        assert got is None or np.abs(got - ref).max() <= REL_TOL * scale, (ctx, i, "stream", np.abs(got - ref).max() / scale)
        if not topo.children(i) and v.demod_usb:
            pre_ref = nodes[i].usb_prequant()
            pre = rx.prequant(i).astype(np.float64)
            s = float(np.abs(pre_ref).max())
            assert np.abs(pre - pre_ref).max() <= REL_TOL * s, (ctx, i, "prequant", np.abs(pre - pre_ref).max() / s)
            assert np.abs(rx.output(i).astype(np.int32) - nodes[i].usb().astype(np.int32)).max() <= 1, (ctx, i)


def test_cs16_dc_bias_blocked_scan_option(Receiver):
    """test_u8_dc_bias_blocked_scan_option on int16: the same bytes (clipped at 254, the largest byte with an image), embedded;
    the same model -- the float64 IIR response through the oracle chain, to the usual tolerance --, the same bound on the
    reference recurrence's own wander around it, the same bound on the kernels' time."""
    import scipy.signal as sg
    topo = tp.config2()
    rx = Receiver.from_topology(topo, exact=True, keep_prequant=True, dc_blocked_scan=True)
    nodes, roots = ob.build_tree("port", topo)          # fed with the true IIR response
    rnodes, rroots = ob.build_tree("port", topo)        # fed with the reference's recurrence
    rng = np.random.default_rng(5)
    A = float(np.float32(1.0) - np.float32(0.000001))
    B = float(np.float32(0.000001))
    z = [np.zeros(1), np.zeros(1)]
    state = np.zeros(2, np.float32)
    rx.enable_kernel_timing(True)
    worst = 0.0
    for f in range(6):
        b = rng.integers(0, 256, 2 * topo.frame, dtype=np.uint8)
        b[0::2] = np.clip(b[0::2].astype(int) + 3, 0, 254)
        b[1::2] = np.clip(b[1::2].astype(int) - 2, 0, 254)
        rx.process_fmt(embed_s16(b), correct_dc=True)
        x = ob.u8_to_float(b)
        iq = x.copy()
        for comp in (0, 1):
            a, z[comp] = sg.lfilter([B], [1.0, -A], x[comp::2].astype(np.float64), zi=z[comp])
            iq[comp::2] = x[comp::2] - a.astype(np.float32)
        ob.process_roots(roots, iq)
        _check_tolerance(rx, nodes, topo, ("cs16-blocked-dc", f))
        ref = x.copy()
        ob.dc_correct(ref, state)
        ob.process_roots(rroots, ref)
        for i in (0, 1):
            want = rnodes[i].stream()
            worst = max(worst, float(np.abs(rx.stream(i) - want).max() / np.abs(want).max()))
    kt = rx.kernel_times()
    rx.close()
    print("worst", worst, kt["k_ingest"])
    assert 1e-6 < worst < 2e-4, worst
    assert kt["k_ingest"]["ms"] / kt["k_ingest"]["launches"] < 0.1, kt["k_ingest"]


@pytest.mark.parametrize("n", [1296, 69968])
def test_blocked_scan_with_a_short_last_chunk(Receiver, n):
    """Option dc_blocked_scan on frames that are no multiple of 1024: the padding behind the last chunk's samples, the guards on
    its stores and the lane that leaves the state.  1296 = one chunk + 272 samples (17 lanes), the smallest frame with a short
    last chunk and a carry-in; 69968 = 68 chunks + 336, where the carry-in loop runs more than one round per lane.  The same
    bytes as dongle bytes, int8 and int16: one result bit for bit, within the usual tolerance of the float64 IIR response."""
    import scipy.signal as sg
    topo = _shape_tree(n, wide=False)
    fmts = (ingest.CU8, ingest.CS8, ingest.CS16)
    rxs = {fmt: Receiver.from_topology(topo, exact=True, keep_streams=True, dc_blocked_scan=True) for fmt in fmts}
    rng = np.random.default_rng(n)
    A = float(np.float32(1.0) - np.float32(0.000001))
    B = float(np.float32(0.000001))
    z = [np.zeros(1), np.zeros(1)]
    for f in range(3):
        b = rng.integers(0, 256, 2 * n, dtype=np.uint8)
        b[0::2] = np.clip(b[0::2].astype(int) + 3, 0, 254)
        b[1::2] = np.clip(b[1::2].astype(int) - 2, 0, 254)
        rxs[ingest.CU8].process_u8(b, correct_dc=True)
        rxs[ingest.CS8].process_fmt(embed_s8(b), correct_dc=True)
        rxs[ingest.CS16].process_fmt(embed_s16(b), correct_dc=True)
        for fmt in (ingest.CS8, ingest.CS16):
            _check_twin(rxs[fmt], rxs[ingest.CU8], topo, (n, NAME[fmt], f))
        x = ob.u8_to_float(b)
        iq = x.copy()
        for comp in (0, 1):
            a, z[comp] = sg.lfilter([B], [1.0, -A], x[comp::2].astype(np.float64), zi=z[comp])
            iq[comp::2] = x[comp::2] - a.astype(np.float32)
        got = rxs[ingest.CU8].raw()
        err = float(np.abs(got - iq.view(np.complex64)).max())
        print(f"n {n} frame {f}: max |raw - model| {err:.3g}, bound {REL_TOL * float(np.abs(x).max()):.3g}")
        assert got.size == n and err <= REL_TOL * float(np.abs(x).max()), (n, f, err)
    for rx in rxs.values():
        rx.close()


# ------------------------------------------------------------------------------------------- 9. launch forms
def _forms_tree(n=20480):
    t = tp.Topology(fs=4 * n, frame=n, name="fmtforms")
    t.vfos.append(tp.VfoDesc(topic="M", parent=-1, fs=4 * n, decimate_count=0, mixer_freq=float(n // 7), demod_usb=False, cstyle=1,
                             samples_per_buffer=n))
    for j in range(3):
        t.vfos.append(tp.VfoDesc(topic=f"S{j}", parent=0, fs=4 * n, decimate_count=2, mixer_freq=float(n // 11) * (j + 1), filter_bw=0,
                                 gain=tp._g(0.05), cstyle=1, samples_per_buffer=n))
    t.vfos.append(tp.VfoDesc(topic="R", parent=-1, fs=4 * n, decimate_count=1, mixer_freq=-float(n // 5), demod_usb=False, cstyle=0,
                             samples_per_buffer=n))
    return t


@functools.lru_cache(maxsize=None)
def _forms_run():
    """Eight int16 frames with an offset, and what process_fmt makes of them frame by frame with DC removal: messages and raw."""
    from sdrreceiver_amd.receiver import Receiver
    topo = _forms_tree()
    rng = np.random.default_rng(9)
    frames = []
    for _ in range(8):
        v = _random_samples(rng, ingest.CS16, topo.frame)
        v[0::2] = v[0::2] // 8 + 5000
        frames.append(v)
    rx = Receiver.from_topology(topo)
    want = []
    for v in frames:
        rx.process_fmt(v, correct_dc=True)
        want.append((list(rx.published), rx.raw()))
    rx.close()
    assert all(len(m) == 4 for m, _ in want)
    return topo, frames, want


def _device(frames):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in frames]
    torch.cuda.synchronize()
    return out


def test_submit_fmt_with_two_frames_in_flight(Receiver):
    topo, frames, want = _forms_run()
    rx = Receiver.from_topology(topo)
    for k in range(0, len(frames), 2):
        rx.submit_fmt(frames[k], correct_dc=True)
        rx.submit_fmt(frames[k + 1], correct_dc=True)
        assert rx.in_flight() == 2
        rx.wait()
        assert rx.published == want[k][0], k
        rx.wait()
        assert rx.published == want[k + 1][0], k + 1
        assert np.array_equal(bits(rx.raw()), bits(want[k + 1][1])), k + 1
    rx.close()


def test_device_frames_queued_and_submitted(Receiver):
    topo, frames, want = _forms_run()
    dev = _device(frames)
    rx = Receiver.from_topology(topo)
    for k in range(3):  # three frames deep on the device queue, one fetch
        rx.process_device_fmt(dev[k].data_ptr(), topo.frame, ingest.CS16, correct_dc=True)
    rx.fetch()
    assert rx.published == want[2][0]
    assert np.array_equal(bits(rx.raw()), bits(want[2][1]))
    # a misaligned device pointer: refused, nothing queued, the accumulator untouched
    code, text = _code(lambda: rx.process_device_fmt(dev[3].data_ptr() + 4, topo.frame, ingest.CS16, correct_dc=True))
    assert code == _lib.SDRX_EINVAL and "16-byte aligned" in text
    code, _ = _code(lambda: rx.submit_device_fmt(dev[3].data_ptr() + 8, topo.frame, ingest.CS16, correct_dc=True))
    assert code == _lib.SDRX_EINVAL and rx.in_flight() == 0
    rx.submit_device_fmt(dev[3].data_ptr(), topo.frame, ingest.CS16, correct_dc=True)
    rx.submit_device_fmt(dev[4].data_ptr(), topo.frame, ingest.CS16, correct_dc=True)
    rx.wait()
    assert rx.published == want[3][0]
    rx.wait()
    assert rx.published == want[4][0]
    assert np.array_equal(bits(rx.raw()), bits(want[4][1]))
    for k in (5, 6):  # and back onto the device queue, then a host frame
        rx.process_device_fmt(dev[k].data_ptr(), topo.frame, ingest.CS16, correct_dc=True)
    rx.process_fmt(frames[7], correct_dc=True)
    assert rx.published == want[7][0]
    assert np.array_equal(bits(rx.raw()), bits(want[7][1]))
    rx.close()


def test_device_frames_of_the_other_formats(Receiver):
    """int8 and dongle bytes in device memory, without DC removal: what the host forms give."""
    topo = _forms_tree()
    rng = np.random.default_rng(10)
    for fmt in (ingest.CS8, ingest.CU8):
        host, rx = Receiver.from_topology(topo), Receiver.from_topology(topo)
        frames = [rng.integers(0, 256, 2 * topo.frame, dtype=np.uint8).view(ingest.FORMATS[fmt]) for _ in range(2)]
        dev = _device(frames)
        for k, v in enumerate(frames):
            host.process_fmt(v)
            rx.submit_device_fmt(dev[k].data_ptr(), topo.frame, fmt)
            rx.wait()
            assert rx.published == host.published and len(rx.published) == 4, (NAME[fmt], k)
        if fmt == ingest.CS8:
            assert np.array_equal(bits(rx.raw()), bits(host.raw()))
        else:  # the bytes went to level 0 where they lie: caller-owned memory, as after sdrx_submit_device
            assert _code(rx.raw)[0] == _lib.SDRX_ESTATE
        host.close()
        rx.close()


def test_mirror_sdrj_takes_the_three_dtypes():
    """receiver.sdrj's byte entry fed uint8, int8 and int16 arrays of the same sample values, DC correction on: the same
    messages from three radios."""
    from sdrreceiver_amd.receiver import sdrj, vfo

    def radio():
        main = vfo()
        main.setFs(1536000); main.setDecimationCount(2); main.setMixerFreq(484000); main.setDemodUSB(False)
        main.setCompressonStyle(1); main.init(384000, False)
        sub = vfo()
        sub.setZmqTopic("VFO01"); sub.setDecimationCount(5); sub.setFilterBandwidth(4000); sub.setGain(5 / 100)
        sub.setMixerFreq(110854); sub.setFs(384000); sub.setCompressonStyle(1); sub.init(96000, True, 0)
        main.setVFOs([sub])
        r = sdrj()
        r.setVFOs([main])
        r.setDCCorrection(True)
        return r

    radios = {fmt: radio() for fmt in (ingest.CU8, ingest.CS8, ingest.CS16)}
    rng = np.random.default_rng(12)
    for f in range(2):
        b = rng.integers(0, 255, 2 * 384000, dtype=np.uint8)
        radios[ingest.CU8].demodBytes(b)
        radios[ingest.CS8].demodBytes(embed_s8(b))
        radios[ingest.CS16].demodBytes(embed_s16(b))
        want = list(radios[ingest.CU8].published)
        assert len(want) == 1 and want[0][:2] == (b"VFO01", 12000)
        assert list(radios[ingest.CS8].published) == want and list(radios[ingest.CS16].published) == want, f
        assert np.array_equal(bits(radios[ingest.CS16].rx.raw()), bits(radios[ingest.CU8].rx.raw())), f


# ------------------------------------------------------------------------------------------- 10. groups
@pytest.mark.parametrize("members", [2, 3])
@pytest.mark.parametrize("correct_dc", [False, True])
def test_group_is_the_single_receiver(Receiver, members, correct_dc):
    from sdrreceiver_amd.receiver import Group
    topo, frames, _ = _forms_run()
    rx = Receiver.from_topology(topo)
    grp = Group.from_topology(topo, [0] * members)
    ctxs = [c for c in (grp.member_context(m)[0] for m in range(members)) if c.value]
    assert len(ctxs) == members
    for k, v in enumerate(frames[:3]):
        rx.process_fmt(v, correct_dc=correct_dc)
        if k == 1:
            grp.submit_fmt(v, correct_dc=correct_dc)
            grp.wait()
        else:
            grp.process_fmt(v, correct_dc=correct_dc)
        assert grp.published == rx.published and len(rx.published) == 4, (members, correct_dc, k)
        for i in topo.leaves_in_publish_order():
            assert np.array_equal(grp.output(i), rx.output(i)), (members, correct_dc, k, i)
        want = rx.raw()
        for m, ctx in enumerate(ctxs):
            out = np.zeros(2 * topo.frame, np.float32)
            got = C.c_int()
            assert grp.L.sdrx_get_raw(ctx, out.ctypes.data, topo.frame, C.byref(got)) == 0
            assert got.value == topo.frame and np.array_equal(bits(out.view(np.complex64)), bits(want)), (members, correct_dc, k, m)
    for call in (grp.L.sdrx_group_process_fmt, grp.L.sdrx_group_submit_fmt):  # an unknown format: refused, nothing in flight
        assert call(grp.h, frames[0].ctypes.data, topo.frame, 3, 0) == _lib.SDRX_EINVAL
        assert "SDRX_FMT_CS16" in grp.L.sdrx_group_last_error(grp.h).decode() and grp.in_flight() == 0
    grp.process_fmt(frames[3], correct_dc=correct_dc)
    rx.process_fmt(frames[3], correct_dc=correct_dc)
    assert grp.published == rx.published
    grp.close()
    rx.close()


# ------------------------------------------------------------------------------------------- 11. raw spectrum, raw watch
def test_raw_spectrum_and_raw_watch(Receiver):
    """SDRX_SPECTRUM_RAW and a watched parent-less leaf on int16 frames without DC removal: what the cf32 path fed
    to_float of the same samples gives.  Five frames: the raw spectrum's first update is due on the fifth."""
    n = 8 * 8704
    topo = tp.Topology(fs=4 * n, frame=n, name="fmtwatch")
    topo.vfos.append(tp.VfoDesc(parent=-1, fs=4 * n, decimate_count=3, mixer_freq=float(n // 3 + 37), demod_usb=False, cstyle=1,
                                samples_per_buffer=n))
    topo.vfos.append(tp.VfoDesc(topic="S1", parent=0, fs=n // 2, decimate_count=2, mixer_freq=float(n // 16 + 11), gain=0.01, cstyle=1,
                                samples_per_buffer=n // 8))
    topo.vfos.append(tp.VfoDesc(topic="R1", parent=-1, fs=4 * n, decimate_count=4, mixer_freq=float(n + 5), gain=0.01, cstyle=1,
                                samples_per_buffer=n))
    topo.vfos.append(tp.VfoDesc(topic="R2", parent=-1, fs=4 * n, decimate_count=3, mixer_freq=float(-n // 2), demod_usb=False, cstyle=0,
                                samples_per_buffer=n))
    ids = [2, 3]
    rxs = [Receiver.from_topology(topo, watch=True) for _ in range(2)]
    for rx in rxs:
        rx.set_watch(ids, [1, 1])
        rx.set_spectrum(_lib.SPECTRUM_RAW)
    rng = np.random.default_rng(11)
    for f in range(5):
        v = _random_samples(rng, ingest.CS16, n)
        rxs[0].process_fmt(v)
        rxs[1].process(ingest.to_float(v))
        a, b = (rx.watch(ids) for rx in rxs)
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (f, "watch", key)
        assert list(a["frame"]) == [f, f]
        for i in ids:
            (pa, fa), (pb, fb) = (rx.watch_psd(i) for rx in rxs)
            assert fa == fb == f and np.array_equal(pa.view(np.uint64), pb.view(np.uint64)), (f, i, "watch PSD")
        sa, sb = (rx.spectrum(_lib.SPECTRUM_RAW) for rx in rxs)
        assert sa["updates"] == sb["updates"] == (1 if f == 4 else 0), (f, sa["updates"], sb["updates"])
        for key in sa:
            assert np.array_equal(np.atleast_1d(sa[key]).view(np.uint8), np.atleast_1d(sb[key]).view(np.uint8)), (f, "spectrum", key)
        assert rxs[0].published == rxs[1].published
    for rx in rxs:
        rx.close()


# ------------------------------------------------------------------------------------------- 12. errors
def test_refusals_leave_the_context_running(Receiver):
    topo, frames, want = _forms_run()
    rx = Receiver.from_topology(topo)
    L, n = rx.L, topo.frame
    ptr = frames[0].ctypes.data

    def refused(rc, code, *words):
        text = L.sdrx_last_error(rx.h).decode()
        assert rc == code and all(w in text for w in words), (rc, text)
        assert rx.in_flight() == 0

    k = 0

    def next_frame_runs():
        nonlocal k
        rx.process_fmt(frames[k], correct_dc=True)
        assert rx.published == want[k][0] and np.array_equal(bits(rx.raw()), bits(want[k][1])), k
        k += 1

    for call in (L.sdrx_process_fmt, L.sdrx_submit_fmt):
        for fmt in (3, -1):
            refused(call(rx.h, ptr, n, fmt, 1), _lib.SDRX_EINVAL, "SDRX_FMT_CU8", "SDRX_FMT_CS8", "SDRX_FMT_CS16")
            next_frame_runs()
    refused(L.sdrx_process_fmt(rx.h, None, n, ingest.CS16, 1), _lib.SDRX_EINVAL, "null frame pointer")
    refused(L.sdrx_process_device_fmt(rx.h, None, n, ingest.CS16, 1), _lib.SDRX_EINVAL, "null frame pointer")
    next_frame_runs()
    refused(L.sdrx_process_fmt(rx.h, ptr, n - 16, ingest.CS16, 1), _lib.SDRX_EINVAL, f"frame of {n - 16} samples")
    refused(L.sdrx_submit_fmt(rx.h, ptr, n + 16, ingest.CS8, 0), _lib.SDRX_EINVAL, f"frame of {n + 16} samples")
    next_frame_runs()
    # a source whose last frame was int16: nothing of its own to share, as after a DC-corrected frame
    other = Receiver.from_topology(topo)
    src = Receiver.from_topology(topo)
    src.process_fmt(frames[0])
    assert _code(lambda: other.submit_shared(src))[0] == _lib.SDRX_ESTATE
    assert _code(lambda: other.process_shared(src))[0] == _lib.SDRX_ESTATE
    assert other.in_flight() == 0
    other.process_fmt(frames[0], correct_dc=True)  # (the refused context still runs: its first frame)
    assert other.published == want[0][0]
    src.process_u8(frames[0].view(np.uint8)[: 2 * n])  # ... and dongle bytes are shared as ever
    other.process_shared(src)
    assert len(other.published) == 4
    next_frame_runs()
    # in-flight limits as for sdrx_submit_u8
    rx2 = Receiver.from_topology(topo)
    rx2.submit_fmt(frames[0], correct_dc=True)
    rx2.submit_fmt(frames[1], correct_dc=True)
    assert _code(lambda: rx2.submit_fmt(frames[2], correct_dc=True))[0] == _lib.SDRX_ESTATE
    assert _code(lambda: rx2.process_fmt(frames[2], correct_dc=True))[0] == _lib.SDRX_ESTATE
    rx2.wait()
    rx2.wait()
    assert rx2.published == want[1][0]
    fresh = Receiver(device=0)
    assert fresh.L.sdrx_process_fmt(fresh.h, ptr, n, ingest.CS16, 0) == _lib.SDRX_ESTATE  # before finalize
    for r in (rx, rx2, other, src, fresh):
        r.close()
