#!/usr/bin/env python3
"""tools/front_time.py [--rounds R] [--frames F] [--subs N] -- what the half-band front stage costs in the ingest group.

Three cases of 16-bit frames without DC removal, device-resident and queued back to back (process_device_fmt, one fetch a
round), with sdrx_enable_kernel_timing on; the figure is the ingest group of sdrx_get_kernel_times in microseconds per frame,
median and range over the rounds:
  "5 MS real -> 2.5 MS complex": 5 000 000 RS16 real samples through one real stage (K = 15) into a 2.5 MS/frame root; beside
      it the same root fed 2 500 000 CS16 samples (the conversion pass alone), the two receivers taking turns round by round;
  "5 MS real -> config 3": the same samples through the real stage, a second stage and the 192/625 resampler (T = 64) into
      config 3's tree (1.536 MS/s, 384 000 a frame); beside it config 3 fed 384 000 CS16 samples;
  "10 MS complex -> 6.144 MS/s root": the route without a front stage -- 2 500 000 CS16 samples through the 384/625 resampler
      (T = 32) into config 3's tree re-rooted at 6.144 MS/s (each main two half-bands deeper); its k_mix_levels time is printed
      too, since the deeper level 0 is where that route pays.
Beside them what the shapes say: bytes and multiply-adds a frame.  (One kernel alone: run this under rocprofv3 --kernel-trace
--output-format csv with --rounds 1 and read its rows.)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from sdrreceiver_amd import _lib, front as fr, ingest, topology as tp  # noqa: E402
from sdrreceiver_amd.receiver import Receiver  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--subs", type=int, default=1024)
args = ap.parse_args()
K = 15


def wide_root() -> tp.Topology:
    """One main at 10 MS/s, d = 1, with a compress sub, and a parent-less compress leaf: 2 500 000 samples a frame"""
    fs, n = 10000000, 2500000
    t = tp.Topology(fs=fs, frame=n, name="root10000")
    t.vfos.append(tp.VfoDesc(topic="MAIN0", parent=-1, fs=fs, decimate_count=1, mixer_freq=100000.0, demod_usb=False, cstyle=1, samples_per_buffer=n))
    t.vfos.append(tp.VfoDesc(topic="CMP01", parent=0, fs=fs // 2, decimate_count=0, mixer_freq=-50000.0, demod_usb=False, cstyle=1,
                             samples_per_buffer=n // 2))
    t.vfos.append(tp.VfoDesc(topic="RAW02", parent=-1, fs=fs, decimate_count=0, mixer_freq=-200000.0, demod_usb=False, cstyle=0, samples_per_buffer=n))
    return t


def config3_at_6144(subs) -> tp.Topology:
    """config 3 with its mains two half-bands deeper: a 6.144 MS/s root, 1 536 000 samples a frame"""
    t = tp.config3(subs)
    t.fs, t.frame, t.name = 4 * t.fs, 4 * t.frame, t.name + "-root6144"
    for d in t.vfos:
        if d.parent < 0:
            d.fs, d.samples_per_buffer, d.decimate_count = 4 * d.fs, 4 * d.samples_per_buffer, d.decimate_count + 2
    return t


def frames_of(n, real, count=2):
    rng = np.random.default_rng(n)
    host = [rng.integers(-2048, 2048, n if real else 2 * n).astype(np.int16) for _ in range(count)]
    dev = [torch.from_numpy(v).cuda() for v in host]
    torch.cuda.synchronize()
    return dev


def times_us(rx, dev, n, fmt, frames):
    rx.enable_kernel_timing(True)  # (zeroes the sums)
    for k in range(frames):
        rx.process_device_fmt(dev[k % len(dev)].data_ptr(), n, fmt)
    rx.fetch()
    t = rx.kernel_times()
    return {k: v["ms"] / frames * 1e3 for k, v in t.items() if v["launches"]}


def summary(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


N = fr.n_taps(K)
CASES = {
    "5 MS real -> 2.5 MS complex": {
        "on": (wide_root(), dict(front_stages=1, front_real=True, front_taps=K), 5000000, ingest.RS16),
        "off": (wide_root(), {}, 2500000, ingest.CS16),
        # the real stage reads 2 B a real sample and writes 8 B an output; the conversion pass reads 4 B and writes 8 B a sample
        "bytes_per_frame": {"on": 2 * 5000000 + 8 * 2500000, "off": 12 * 2500000},
        "multiply_adds_per_frame": {"on": (2 * K + 3) * 2500000},
    },
    "5 MS real -> config 3": {
        "on": (tp.config3(args.subs), dict(front_stages=2, front_real=True, front_taps=K, input_rate=5000000, resample_taps=64), 5000000, ingest.RS16),
        "off": (tp.config3(args.subs), {}, 384000, ingest.CS16),
        "bytes_per_frame": {"on": 2 * 5000000 + 8 * 2500000 + (8 * 2500000 + 8 * 1250000) + (8 * 1250000 + 8 * 384000 + 4 * 192 * 64), "off": 12 * 384000},
        "multiply_adds_per_frame": {"on": (2 * K + 3) * 2500000 + 2 * (2 * K + 3) * 1250000 + 2 * 64 * 384000},
    },
    "10 MS complex -> 6.144 MS/s root": {
        "on": (config3_at_6144(args.subs), dict(input_rate=10000000, resample_taps=32), 2500000, ingest.CS16),
        "off": (tp.config3(args.subs), {}, 384000, ingest.CS16),
        "bytes_per_frame": {"on": 12 * 2500000 + (8 * 2500000 + 8 * 1536000 + 4 * 384 * 32), "off": 12 * 384000},
        "multiply_adds_per_frame": {"on": 2 * 32 * 1536000},
    },
}

out = {"build_id": _lib.lib().sdrx_build_id().decode(), "rounds": args.rounds, "frames_per_round": args.frames, "K": K, "taps": N, "cases": {}}
for name, case in CASES.items():
    pair = {}
    for key in ("off", "on"):
        topo, kw, n, fmt = case[key]
        rx = Receiver.from_topology(topo, **kw)
        rx.set_publish(False)
        dev = frames_of(n, ingest.is_real(fmt))
        times_us(rx, dev, n, fmt, 4)  # warm-up
        pair[key] = (rx, dev, n, fmt)
    us = {"off": {}, "on": {}}
    for r in range(args.rounds):
        for key in (("off", "on") if r % 2 == 0 else ("on", "off")):
            for kind, v in times_us(*pair[key], args.frames).items():
                us[key].setdefault(kind, []).append(v)
    rx_on, rx_off = pair["on"][0], pair["off"][0]
    out["cases"][name] = {
        "in_frame": pair["on"][2], "tree_frame": pair["on"][0].root_frame(),
        "front": {k: v for k, v in (rx_on.front or {}).items() if k != "taps"} or None,
        "resampler": {k: v for k, v in (rx_on.resampler or {}).items() if k != "taps"} or None,
        "us_per_frame": {key: {kind: summary(v) for kind, v in us[key].items()} for key in us},
        "bytes_per_frame": case["bytes_per_frame"], "multiply_adds_per_frame": case["multiply_adds_per_frame"],
        "device_bytes": {"on": rx_on.stats()["device_bytes"], "off": rx_off.stats()["device_bytes"]}}
    for rx, *_ in pair.values():
        rx.close()
    del pair
    torch.cuda.empty_cache()
print(json.dumps(out))
