"""The ADC meter on the device (option adc_meter, k_adc_meter): every record bit for bit tests/adc_ref.py's integer model.

Frames are small: the smallest sdrx_finalize takes (1024), ones that end mid-wave and mid-workgroup (1296, 16368, 69968) and
whole numbers of workgroups (the lattice's three-level tree, 65536); the 384 000 / 480 000-sample frames are the byte regimes of
tests/golden/dc_reference.npz.  tests/test_adc_model.py asserts what the crafted frames cross."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import adc_ref as ar
import lattice
import watch_ref as wr
from helpers import dc_reference_bytes
from sdrreceiver_amd import _lib, ingest
from sdrreceiver_amd.receiver import Group, Receiver, SdrxError
from test_gpu_ingest_formats import _dc_topology, _forms_tree, _regime, _shape_tree

pytestmark = pytest.mark.gpu

CU8, CS8, CS16 = ar.CU8, ar.CS8, ar.CS16
PARTIAL_BYTES, RECORD_BYTES = 176, 184  # adcmeter.hip's AdcPartial; sdrx_adc_meter


def _code(call):
    with pytest.raises(SdrxError) as e:
        call()
    return e.value.code


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _launches(rx):
    return {k: v["launches"] for k, v in rx.kernel_times().items()}


def _device(frames):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in frames]
    torch.cuda.synchronize()
    return out


def _member_record(L, ctx) -> dict:
    out = _lib.AdcMeterC()
    assert L.sdrx_get_adc_meter(ctx, C.byref(out)) == 0, L.sdrx_last_error(ctx).decode()
    return ingest.adc_dict(out)


# ---- crafted frames, full-range frames, formats alternating from frame to frame -------------------------------------------------
@pytest.mark.parametrize("n", [1024, ar.SMALL_N, ar.CRAFT_N, 69968])
def test_crafted_and_full_range_frames(n):
    """One receiver per size takes every crafted frame of every format in turn (so the format changes from frame to frame),
    then full-range random samples; DC removal on for every other frame: the record does not see it."""
    rx = Receiver.from_topology(_shape_tree(n, wide=False), adc_meter=True)
    frames = []
    names = sorted(ar.crafted(CS16, n)) if n != 69968 else ["all_lowest", "alternating", "boundaries", f"lowest_at_{n - 1}"]
    for name in names:
        for fmt in ar.FORMATS:
            frames.append((name, fmt, ar.crafted(fmt, n)[name]))
    for b in (0, 127, 128, 255):
        frames.append((f"bytes_{b}", CU8, ar.crafted(CU8, n)[f"bytes_{b}"]))
    for fmt in ar.FORMATS:
        frames.append(("full_range", fmt, ar.full_range(fmt, n, seed=n + fmt)))
    for f, (name, fmt, v) in enumerate(frames):
        rx.process_fmt(v, correct_dc=bool(f & 1))
        got, want = rx.adc_meter(), ar.model(v, fmt, frame=f)
        assert got == want, (n, name, ar.NAME[fmt], {k: (got[k], want[k]) for k in want if got[k] != want[k]})
    rx.close()


# ---- natural frames: the byte regimes of dc_reference.npz --------------------------------------------------------------------
NATURAL = [("lcg", ar.FORMATS), ("step", ar.FORMATS), ("capture480", ar.FORMATS), ("const0", ar.FORMATS), ("const255", (CU8,)),
           ("alt", (CU8,)), ("extremes", (CU8,))]


@functools.lru_cache(maxsize=None)
def _bytes_of(rid):
    return _regime(rid) if rid in ("lcg", "step", "capture480", "const0") else dc_reference_bytes(rid)


@pytest.mark.parametrize("rid,fmts", NATURAL, ids=[r for r, _ in NATURAL])
def test_byte_regimes_with_and_without_dc(rid, fmts):
    """Each regime as CU8, and as CS8 / CS16 through "to int8" / "times 256"; correct_dc 0 and 1 and both DC options: the same
    record every time."""
    frames = _bytes_of(rid)
    frames = frames if rid == "extremes" else frames[:1]
    n = frames[0].size // 2
    rxs = {"default": Receiver.from_topology(_dc_topology(n), adc_meter=True),
           "blocked": Receiver.from_topology(_dc_topology(n), adc_meter=True, dc_blocked_scan=True),
           "sequential": Receiver.from_topology(_dc_topology(n), adc_meter=True, dc_speculative=False)}
    count = dict.fromkeys(rxs, 0)
    for b in frames:
        for fmt in fmts:
            v = ar.from_bytes(b, fmt)
            want = ar.model(v, fmt)
            for key, dc in (("default", False), ("default", True), ("blocked", True), ("sequential", True)):
                rxs[key].process_fmt(v, correct_dc=dc)
                assert rxs[key].adc_meter() == dict(want, frame=count[key]), (rid, ar.NAME[fmt], key, dc)
                count[key] += 1
    for rx in rxs.values():
        rx.close()


# ---- launch forms -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forms_frames():
    topo = _forms_tree()
    n = topo.frame
    return topo, [ar.full_range(CS16, n, 1), ar.full_range(CS8, n, 2), ar.samples_of(ar._background(np.random.default_rng(3), CU8, n), CU8),
                  ar.full_range(CS16, n, 4)]


def _fmt_of(v):
    return ingest.infer_format(v)


def test_submit_with_two_frames_in_flight():
    topo, frames = _forms_frames()
    rx = Receiver.from_topology(topo, adc_meter=True)
    want = [ar.model(v, _fmt_of(v), frame=f) for f, v in enumerate(frames[:4])]
    rx.submit_fmt(frames[0], correct_dc=True)
    rx.submit_fmt(frames[1])
    assert _code(rx.adc_meter) == _lib.SDRX_ESTATE  # submitted, none delivered
    rx.wait()
    assert rx.in_flight() == 1 and rx.adc_meter() == want[0]  # frame 0's record while frame 1 is in flight
    rx.wait()
    assert rx.in_flight() == 0 and rx.adc_meter() == want[1]
    rx.submit_fmt(frames[2])
    assert rx.adc_meter() == want[1]  # frame 2 writes the other slot
    rx.submit_fmt(frames[3], correct_dc=True)
    rx.wait()
    assert rx.adc_meter() == want[2]
    rx.wait()
    assert rx.in_flight() == 0 and rx.adc_meter() == want[3]
    rx.close()


def test_device_frames_queued_and_submitted():
    topo, frames = _forms_frames()
    dev = _device(frames)
    n = topo.frame
    rx = Receiver.from_topology(topo, adc_meter=True)
    rx.process_device_fmt(dev[0].data_ptr(), n, CS16, correct_dc=True)
    assert rx.adc_meter() == ar.model(frames[0], CS16, frame=0)  # the getter runs what is outstanding first
    rx.submit_device_fmt(dev[1].data_ptr(), n, CS8)
    rx.submit_device_fmt(dev[2].data_ptr(), n, CU8)
    rx.wait()
    assert rx.adc_meter() == ar.model(frames[1], CS8, frame=1)
    rx.wait()
    assert rx.adc_meter() == ar.model(frames[2], CU8, frame=2)
    rx.process_device_fmt(dev[2].data_ptr(), n, CU8, correct_dc=True)
    rx.fetch()
    assert rx.adc_meter() == ar.model(frames[2], CU8, frame=3)
    rx.close()


@pytest.mark.parametrize("fuse,frame_pipeline", [(True, True), (True, False), (False, True), (False, False)])
def test_six_device_frames_queued_back_to_back(fuse, frame_pipeline):
    """A tree of three levels, six frames on the device queue, one fetch: the record is the last frame's."""
    topo = lattice.trees()["inner"]
    n = topo.frame
    frames = [ar.full_range((CS16, CS8, CU8)[k % 3], n, 40 + k) if k % 3 < 2 else ar.samples_of(ar._background(np.random.default_rng(k), CU8, n), CU8)
              for k in range(6)]
    dev = _device(frames)
    rx = Receiver.from_topology(topo, adc_meter=True, fuse=fuse, frame_pipeline=frame_pipeline)
    for k, v in enumerate(frames):
        rx.process_device_fmt(dev[k].data_ptr(), n, _fmt_of(v), correct_dc=k == 4)
    rx.fetch()
    assert rx.adc_meter() == ar.model(frames[5], _fmt_of(frames[5]), frame=5)
    rx.close()


def test_cf32_and_shared_frames_are_not_measured():
    topo, frames = _forms_frames()
    rx = Receiver.from_topology(topo, adc_meter=True)
    rx.process_fmt(frames[0])
    assert rx.adc_meter() == ar.model(frames[0], CS16, frame=0)
    rx.process_fmt(frames[1], correct_dc=True)
    assert rx.adc_meter() == ar.model(frames[1], CS8, frame=1)
    rx.process(ingest.to_float(frames[0]))  # the same values as cf32: not ADC samples (the slot holds frame 0's stale record)
    assert rx.adc_meter() == ar.unmeasured(2)
    rx.process_fmt(frames[1])
    assert rx.adc_meter() == ar.model(frames[1], CS8, frame=3)
    # a process_shared consumer reads the source's bytes: measured on the source, not on the consumer
    other = Receiver.from_topology(topo, adc_meter=True)
    rx.process_u8(frames[2])
    assert rx.adc_meter() == ar.model(frames[2], CU8, frame=4)
    other.process_shared(rx)
    assert other.adc_meter() == ar.unmeasured(0)
    other.process_fmt(frames[2])
    assert other.adc_meter() == ar.model(frames[2], CU8, frame=1)
    other.close()
    rx.close()


# ---- groups -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [2, 3])
def test_group_and_every_member(members):
    topo, frames = _forms_frames()
    grp = Group.from_topology(topo, [0] * members, adc_meter=True)
    ctxs = [c for c in (grp.member_context(m)[0] for m in range(members)) if c.value]
    assert len(ctxs) == members
    assert _code(grp.adc_meter) == _lib.SDRX_ESTATE  # nothing delivered yet
    plan = [(frames[0], True, "process"), (frames[2], False, "process"),  # (dongle bytes without DC removal: the group's own path)
            (frames[1], False, "submit"), (frames[2], True, "submit"), (frames[2], False, "u8")]
    for f, (v, dc, how) in enumerate(plan):
        if how == "process":
            grp.process_fmt(v, correct_dc=dc)
        elif how == "u8":
            grp.process_u8(v, correct_dc=dc)
        else:
            grp.submit_fmt(v, correct_dc=dc)
            grp.wait()
        want = ar.model(v, _fmt_of(v), frame=f)
        assert grp.adc_meter() == want, (members, f)
        for m, ctx in enumerate(ctxs):
            assert _member_record(grp.L, ctx) == want, (members, f, m)
    iq = ingest.to_float(frames[0])
    grp.process(iq)
    assert grp.adc_meter() == ar.unmeasured(len(plan))
    assert grp.L.sdrx_group_get_adc_meter(grp.h, None) == _lib.SDRX_EINVAL
    grp.close()
    early = Group([0] * members, adc_meter=True)
    assert _code(early.adc_meter) == _lib.SDRX_ESTATE  # before sdrx_group_finalize
    early.close()
    off = Group.from_topology(topo, [0] * members)
    off.process_fmt(frames[0])
    assert _code(off.adc_meter) == _lib.SDRX_ESTATE  # the option is off on every member
    off.close()


# ---- off means off; the error rules -------------------------------------------------------------------------------------------
def _watch_receiver(**kw):
    topo = wr.watch_tree()
    rx = Receiver.from_topology(topo, watch=True, meter=True, **kw)
    rx.set_watch([1, 2], [1, 1])
    rx.set_spectrum(1)
    rx.enable_kernel_timing(True)
    return rx


def test_off_means_off_and_errors():
    topo = wr.watch_tree()
    ids = [i for i in range(len(topo.vfos)) if not topo.children(i)]
    n = topo.frame
    frames = [ar.full_range(CS16, n, 70), ar.samples_of(ar._background(np.random.default_rng(71), CU8, n), CU8), ar.full_range(CS8, n, 72)]
    on, never = _watch_receiver(adc_meter=True), _watch_receiver()
    off = Receiver(watch=True, meter=True)  # the option named, and switched off
    off._chk(off.L.sdrx_set_option(off.h, b"adc_meter", 0))
    for d in topo.vfos:
        off.add_vfo(d)
    assert off.L.sdrx_get_adc_meter(off.h, C.byref(_lib.AdcMeterC())) == _lib.SDRX_ESTATE  # before sdrx_finalize
    off.finalize()
    off.set_watch([1, 2], [1, 1])
    off.set_spectrum(1)
    off.enable_kernel_timing(True)
    assert _code(on.adc_meter) == _lib.SDRX_ESTATE  # no frame delivered yet
    assert on.L.sdrx_get_adc_meter(on.h, None) == _lib.SDRX_EINVAL  # (the argument is looked at before the delivery)
    assert on.L.sdrx_get_adc_meter(None, C.byref(_lib.AdcMeterC())) == _lib.SDRX_EINVAL
    for f, v in enumerate(frames):
        for rx in (on, never, off):
            rx.process_fmt(v, correct_dc=f == 2)
        for rx in (on, off):
            for i in ids:
                assert np.array_equal(rx.output(i), never.output(i)), (f, i)
            assert rx.published == never.published, f
            ma, mb = rx.meters(ids), never.meters(ids)
            wa, wb = rx.watch(ids), never.watch(ids)
            sa, sb = rx.spectrum(1), never.spectrum(1)
            for a, b in ((ma, mb), (wa, wb), (sa, sb)):
                assert a.keys() == b.keys()
                for key in a:
                    assert np.array_equal(_bits(np.atleast_1d(a[key])), _bits(np.atleast_1d(b[key]))), (f, key)
        assert on.adc_meter() == ar.model(v, ingest.infer_format(v), frame=f)
    assert _code(off.adc_meter) == _lib.SDRX_ESTATE and _code(never.adc_meter) == _lib.SDRX_ESTATE  # the option is off
    assert off.L.sdrx_get_adc_meter(off.h, None) == _lib.SDRX_ESTATE  # (the option before the argument)
    assert off.stats()["device_bytes"] == never.stats()["device_bytes"]
    assert _launches(off) == _launches(never)
    # what the option holds: one partial per workgroup of a frame, the counter, and the record of both parities
    grown = on.stats()["device_bytes"] - never.stats()["device_bytes"]
    assert grown == -(-n // ar.WG) * PARTIAL_BYTES + 4 + 2 * RECORD_BYTES, grown
    assert _launches(on) == _launches(never)  # (k_adc_meter is not bracketed: SDRX_NKERNELS kinds, k_ingest is the conversion)
    # the option on and only cf32 frames: nothing more is launched or timed
    a, b = _watch_receiver(adc_meter=True), _watch_receiver()
    for v in frames[:2]:
        iq = ingest.to_float(frames[0])
        a.process(iq)
        b.process(iq)
    assert _launches(a) == _launches(b)
    assert a.adc_meter() == ar.unmeasured(1)
    for rx in (on, never, off, a, b):
        rx.close()


# ---- the C++ host layer: sdrj::adcMeter and adc_levels behind sdrx_demo --adc -------------------------------------------------
def test_demo_prints_the_record_of_every_frame(tmp_path):
    from sdrreceiver_amd import synth
    from test_topology import INI_25E_LIKE
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    demo = os.path.join(root, "host", "sdrx_demo")
    subprocess.check_call(["make", "-C", os.path.join(root, "host")], stdout=subprocess.DEVNULL)
    profile = tmp_path / "profile.ini"
    profile.write_text(INI_25E_LIKE)
    plain = subprocess.check_output([demo, str(profile), "--frames", "2", "--format", "cs16"], text=True).splitlines()
    lines = subprocess.check_output([demo, str(profile), "--frames", "2", "--format", "cs16", "--adc"], text=True).splitlines()
    adc = [ln.split() for ln in lines if ln.startswith("adc ")]
    assert [ln for ln in lines if not ln.startswith("adc ")] == plain and len(adc) == 2  # the messages are what they were
    lcg = synth.Lcg(1)
    for f, got in enumerate(adc):
        n = int(got[3])
        v = ar.from_bytes(synth.lcg_frame_u8(n, lcg), CS16)  # the demo's stream: components -8 .. 8, times 256
        m = ar.model(v, CS16, frame=f)
        lv = ingest.adc_levels(m)
        want = ["adc", f, "cs16", n, m["i"]["sum"], m["q"]["sum"], m["i"]["sum_sq"], m["q"]["sum_sq"], m["sum_iq"], m["i"]["min"], m["i"]["max"],
                m["q"]["min"], m["q"]["max"], 0, 0, lv["bits_used"], "|"]
        assert got[:len(want)] == [str(x) for x in want], (f, got)
        assert float(got[len(want)]) == pytest.approx(lv["peak"], rel=1e-5) and float(got[len(want) + 1]) == pytest.approx(lv["headroom_db"], abs=1e-3)
    floats = subprocess.check_output([demo, str(profile), "--frames", "1", "--adc"], text=True).splitlines()
    assert floats[-1] == "adc 0 unmeasured"
