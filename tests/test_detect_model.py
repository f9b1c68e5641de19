"""The detector leaves' model (sdrreceiver_amd.detect, the definition the device is held to): the ABI additions, ANG's accuracy
against double atan2, the crafted cases of tests/detect_ref.py -- every wrong device changes a payload, the signal cases are signal
--, the properties the definition promises, the INI key and the refusals that need no device.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import detect_ref as dr
from helpers import SAMPLE_INI
from sdrreceiver_amd import _lib, detect as dt, topology as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sdrx_set_detector", "sdrx_get_detector"]
# ANG against double atan2.  The bound is derived: an error of delta rad moves the payload by delta / pi gain 32768 LSB, so at gain 1
# (full scale = a deviation of fs / 2) delta must stay below pi / 32768 = 9.6e-5 rad to stay within one LSB.  ANG_WORST is the
# value this test found on its grid when the polynomial was designed (DESIGN.md 4z records it): the test asserts twice that too.
ANG_BOUND = 9.6e-5
ANG_WORST = 1.83e-6


def test_abi_additions():
    hdr = open(os.path.join(ROOT, "include", "sdrx.h")).read()
    declared = set(re.findall(r"\b(sdrx_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.sdrx_abi_version() == 5
    for name, v in (("SDRX_DETECT_NONE", dt.NONE), ("SDRX_DETECT_AM", dt.AM), ("SDRX_DETECT_FM", dt.FM)):
        assert f"#define {name} {v}\n" in hdr
    K = _lib.DetectCfgC
    assert C.sizeof(K) == 16 and [getattr(K, f).offset for f in ("kind", "reserved")] == [0, 4]
    assert "SDRX_NKERNELS 8" in hdr and _lib.NKERNELS == 8  # (the detector launches are booked with k_compress)
    assert C.sizeof(_lib.VfoDescC) == 56  # sdrx_vfo_desc does not change
    # the shared header holds the model's coefficients, digit for digit
    src = open(os.path.join(ROOT, "sdrreceiver_amd", "csrc", "sdrx_detect.h")).read()
    lits = [float.fromhex(m) for m in re.findall(r"(-?0x1\.[0-9a-f]+p-?\d+)f", src)]
    assert [np.float32(v) for v in lits] == list(dt.ANG_COEF[::-1])


def test_ang_accuracy():
    ang = np.concatenate([np.linspace(-np.pi, np.pi, 400001), np.arange(-8, 9) * np.pi / 8])
    worst = 0.0
    for m in (1e-30, 1e-12, 1e-3, 0.5, 1.0, 37.5, 1e10, 1e30):
        y, x = (m * np.sin(ang)).astype(np.float32), (m * np.cos(ang)).astype(np.float32)
        got = dt.ang(y, x).astype(np.float64) * np.pi
        d = np.abs(got - np.arctan2(y.astype(np.float64), x.astype(np.float64)))
        worst = max(worst, float(np.minimum(d, 2 * np.pi - d).max()))
    print(f"ANG: worst error {worst:.3e} rad against double atan2")
    assert worst < ANG_BOUND
    assert worst < 2 * ANG_WORST
    assert ANG_BOUND == pytest.approx(np.pi / 32768, rel=2e-3)


def test_ang_axes_diagonals_and_range():
    f = np.float32
    assert dt.ang(f(0), f(0)) == 0 and dt.ang(f(0), f(3)) == 0 and dt.ang(f(0), f(-3)) == 1 and dt.ang(f(-0.0), f(-3)) == 1
    assert dt.ang(f(2), f(0)) == 0.5 and dt.ang(f(-2), f(0)) == -0.5
    d = dt.ang(f(5), f(5))
    assert abs(float(d) - 0.25) < 1e-6 and dt.ang(f(5), f(-5)) == f(1) - d and dt.ang(f(-5), f(-5)) == -(f(1) - d) and dt.ang(f(-5), f(5)) == -d
    rng = np.random.default_rng(3)
    y, x = rng.standard_normal(20000).astype(f), rng.standard_normal(20000).astype(f)
    a = dt.ang(y, x)
    assert np.all(np.abs(a) <= 1) and np.array_equal(dt.ang(-y, x), -a)  # odd in y, whatever the rounding
    assert np.array_equal(dt.ang(y * f(1024), x * f(1024)), a)  # a power of two scales nothing


@pytest.mark.parametrize("wrong", dr.WRONG)
def test_every_wrong_device_changes_a_payload(wrong):
    kind = dr.WRONG_KIND[wrong]
    changed = {}
    for c in dr.crafted():
        want = [r["payload"] for r in dr.model_run(c, kind)]
        got = dr.wrong_run(c, wrong)
        changed[c.name] = sum(int(np.count_nonzero(a != b)) for a, b in zip(got, want))
    assert sum(changed.values()) > 0, changed
    assert len(dr.WRONG) >= 12


def test_signal_cases_are_signal():
    seen = set()
    for c in dr.crafted():
        for kind in c.signal:
            for f, r in enumerate(dr.model_run(c, kind)):
                assert np.count_nonzero(r["payload"]) >= 0.95 * r["payload"].size, (c.name, kind, f)
                assert r["clipped"] == 0, (c.name, kind, f)
            seen.add(kind)
    assert seen == {dt.AM, dt.FM}
    wrap = next(c for c in dr.crafted() if c.name == "wrap")
    assert all(r["clipped"] > 0 for k in (dt.AM, dt.FM) for r in dr.model_run(wrap, k)), "the int16 wraps"


def test_what_the_definition_promises():
    zeros = np.zeros(dr.N_CRAFT, np.complex64)
    assert not dt.am(zeros, 1.0).any() and not dt.fm(zeros, 1.0).any() and not dt.fm(zeros, 1.0, 1 + 1j).any()
    case = next(c for c in dr.crafted() if c.name == "carrier_step")
    # AM carries nothing between frames: a frame's payload is that of the frame alone
    runs = dr.model_run(case, dt.AM)
    for f, z in enumerate(case.frames):
        assert np.array_equal(runs[f]["payload"], dt.am(z, case.gain_am))
    # the carrier sum does not depend on the order or on the geometry
    z = case.frames[1]
    e = dt.envelope(z)
    assert dt.carrier_sum(e) == dt.carrier_sum(e[::-1]) == sum(dt.carrier_sum(e[k:k + 256]) for k in range(0, e.size, 256))
    # FM: z[-1] is the frame before's last sample; a fresh leaf's first value is ANG(0, 0) gain = 0
    fm = dr.model_run(case, dt.FM)
    assert fm[0]["payload"][0] == 0 and np.array_equal(fm[2]["payload"], dt.fm(case.frames[2], case.gain_fm, case.frames[1][-1]))
    both = dt.fm(np.concatenate(case.frames[:2]), case.gain_fm)
    assert np.array_equal(both, np.concatenate([fm[0]["payload"], fm[1]["payload"]])), "frames join without a seam"
    # a phase step of exactly pi is +1 half-turn: full scale wraps to -32768 at gain 1
    pi = next(c for c in dr.crafted() if c.name == "pi_step")
    assert set(np.unique(dr.model_run(pi, dt.FM)[1]["payload"]).tolist()) == {-32768}
    # the meter is the int16 leaves'
    r = runs[0]
    assert r["n_values"] == dr.N_CRAFT and r["sum_sq"] == int(np.sum(r["payload"].astype(np.int64) ** 2))
    with pytest.raises(ValueError):
        dt.run(dt.NONE, zeros, 1.0)


def test_the_trees_cover_the_leaf_frame_lengths():
    lengths = set()
    for key in dr.TREES:
        topo = dr.TREES[key]()
        for i in dr.detector_leaves(topo):
            assert topo.is_leaf(i) and not topo.vfos[i].demod_usb
            lengths.add((topo.vfos[i].detector, topo.vfos[i].n_stage_out, topo.vfos[i].parent < 0))
    n = {v[1] for v in lengths}
    assert {49, 1568, 2048, 3136, 4096, 6272, 8192, 12544} <= n  # < 1 block, exactly 1, 1 + a partial one, 2, 3 + 256, odd
    assert 12544 == 3 * dr.BLOCK + 256 and any(v[2] for v in lengths) and not all(v[2] for v in lengths)
    a = dr.tree_a()
    kinds = {(v.demod_usb, v.detector) for i, v in enumerate(a.vfos) if a.is_leaf(i)}
    assert kinds == {(True, 0), (False, 0), (False, dt.AM), (False, dt.FM)}
    assert max(len(a.children(i)) and 1 + max((len(a.children(j)) > 0) for j in a.children(i)) for i in a.roots()) == 2  # a main below a main


def _ini_with(extra_entries):
    """sdr_25E.ini (a copy, in memory) with more [vfos] entries"""
    text = open(os.path.join(SAMPLE_INI, "sdr_25E.ini")).read()
    kv = tp.parse_ini(text)
    n = int(kv["vfos/size"])
    lines = []
    for k, entry in enumerate(extra_entries, n + 1):
        lines += [f"{k}\\{key}={val}" for key, val in entry.items()]
    text = re.sub(r"(?m)^size=%d\s*$" % n, "size=%d" % (n + len(extra_entries)), text)
    assert f"size={n + len(extra_entries)}" in text
    head, sep, tail = text.partition("[vfos]")
    assert sep
    return head + sep + "\n" + "\n".join(lines) + "\n" + tail, n


def detector_ini():
    """(text, topology): sdr_25E.ini with an AM and an FM entry beside the last 48 kS/s sub"""
    plain = tp.topology_from_ini(open(os.path.join(SAMPLE_INI, "sdr_25E.ini")).read())
    sub = plain.vfos[-1]
    f = int(plain.center_frequency - plain.vfos[sub.parent].mixer_freq - sub.mixer_freq)
    text, _ = _ini_with([{"frequency": f + 5000, "gain": 50, "topic": "AIR01", "detector": "am"},
                         {"frequency": f - 5000, "gain": 100, "topic": "AIS01", "detector": "FM", "filter_bandwidth": 10000}])
    return text, tp.topology_from_ini(text)


def test_the_ini_key():
    plain = tp.topology_from_ini(open(os.path.join(SAMPLE_INI, "sdr_25E.ini")).read())
    assert all(v.detector == 0 for v in plain.vfos)
    sub = plain.vfos[-1]  # a 48 kS/s sub of main 2
    f = int(plain.center_frequency - plain.vfos[sub.parent].mixer_freq - sub.mixer_freq)
    text, n = _ini_with([{"frequency": f + 5000, "gain": 50, "topic": "AIR01", "detector": "am"},
                         {"frequency": f - 5000, "gain": 100, "topic": "AIS01", "detector": "FM", "filter_bandwidth": 10000}])
    topo = tp.topology_from_ini(text)
    assert len(topo.vfos) == len(plain.vfos) + 2 and topo.vfos[:len(plain.vfos)] == plain.vfos
    am, fm = topo.vfos[-2], topo.vfos[-1]
    assert (am.detector, fm.detector) == (dt.AM, dt.FM) and not am.demod_usb and not fm.demod_usb
    for v in (am, fm):  # placed as a 48 kS/s sub is
        assert (v.parent, v.fs, v.decimate_count, v.samples_per_buffer, v.late_decimate) == (sub.parent, sub.fs, sub.decimate_count, sub.samples_per_buffer, 0)
        assert v.output_rate == 48000 and v.filter_bw == 0
    assert am.topic == "AIR01" and am.gain == float(np.float32(0.5)) and am.mixer_freq == sub.mixer_freq - 5000
    with pytest.raises(ValueError, match="only am and fm"):
        tp.topology_from_ini(_ini_with([{"frequency": f, "detector": "usb"}])[0])
    # below a 240 kS/s main the placement needs the late decimation by 5: refused, with a message that says so
    text54 = open(os.path.join(SAMPLE_INI, "sdr_54W_all.ini")).read()
    t54 = tp.topology_from_ini(text54)
    s54 = t54.vfos[-1]
    assert s54.late_decimate == 5
    f54 = int(t54.center_frequency - t54.vfos[s54.parent].mixer_freq - s54.mixer_freq)
    n54 = int(tp.parse_ini(text54)["vfos/size"])
    bad = re.sub(r"(?m)^size=%d\s*$" % n54, "size=%d" % (n54 + 1), text54).replace("[vfos]", f"[vfos]\n{n54 + 1}\\frequency={f54}\n{n54 + 1}\\detector=am\n")
    with pytest.raises(ValueError, match="late decimation by 5"):
        tp.topology_from_ini(bad)


def test_the_ini_key_through_the_cpp_front_door(tmp_path):
    import json
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "sdrx_demo"], stdout=subprocess.DEVNULL)
    demo = os.path.join(ROOT, "host", "sdrx_demo")
    text, topo = detector_ini()
    p = tmp_path / "detect.ini"
    p.write_text(text)
    rows = [json.loads(l) for l in subprocess.check_output([demo, str(p), "--dump"], text=True).splitlines()]
    subs = {r["topic"]: r for r in rows if "sub_of" in r}
    assert rows[0]["n"] == len(topo.vfos) and len(subs) == sum(1 for v in topo.vfos if v.parent >= 0)
    for v in topo.vfos:
        if v.parent < 0:
            continue
        r = subs[v.topic]
        assert (r["sub_of"], r["fs"], r["d"], r["late"], r["mixer"], r["bw"], r["spb"], bool(r["usb"]), r["detector"]) == \
            (v.parent, v.fs, v.decimate_count, v.late_decimate, v.mixer_freq, v.filter_bw, v.samples_per_buffer, v.demod_usb, v.detector), v.topic
        assert np.float32(r["gain"]) == np.float32(v.gain)
    assert subs["AIR01"]["detector"] == dt.AM and subs["AIS01"]["detector"] == dt.FM
    for bad, what in ((text.replace("detector=am", "detector=usb"), "only am and fm"),):
        p.write_text(bad)
        r = subprocess.run([demo, str(p), "--dump"], capture_output=True, text=True)
        assert r.returncode == 1 and what in r.stderr, r.stderr
    text54 = open(os.path.join(SAMPLE_INI, "sdr_54W_all.ini")).read()
    n54 = int(tp.parse_ini(text54)["vfos/size"])
    t54 = tp.topology_from_ini(text54)
    s54 = t54.vfos[-1]
    f54 = int(t54.center_frequency - t54.vfos[s54.parent].mixer_freq - s54.mixer_freq)
    p.write_text(re.sub(r"(?m)^size=%d\s*$" % n54, "size=%d" % (n54 + 1), text54).replace("[vfos]", f"[vfos]\n{n54 + 1}\\frequency={f54}\n{n54 + 1}\\detector=fm\n"))
    r = subprocess.run([demo, str(p), "--dump"], capture_output=True, text=True)
    assert r.returncode == 1 and "late decimation by 5" in r.stderr, r.stderr


def test_refusals_that_need_no_device():
    L = _lib.lib()
    assert L.sdrx_set_detector(None, 0, None) == _lib.SDRX_EINVAL and L.sdrx_get_detector(None, 0, None) == _lib.SDRX_EINVAL
    assert dt.KINDS == {"none": 0, "am": 1, "fm": 2}
    # (sdrx_set_detector's own refusals and the group's need a context, hence a device: tests/test_gpu_detect.py)
