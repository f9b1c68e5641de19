#!/usr/bin/env python3
"""tools/resample_time.py [--rounds R] [--frames F] -- what the resampler costs in the ingest group.

Two cases of int16 frames without DC removal, device-resident and queued back to back (process_device_fmt, one fetch a round),
with sdrx_enable_kernel_timing on: 600 000 -> 384 000 samples (2.4 -> 1.536 MS/s, L/M = 16/25, T = 24) into config 3's tree,
and 1 500 000 -> 1 536 000 (6 -> 6.144 MS/s, 128/125, T = 32) into a 6.144 MS/s root.  Per case two receivers, the resampler on
(frames at the input rate) and off (frames at the tree's rate), taking turns round by round in one process; the figure is the
ingest group of sdrx_get_kernel_times -- the conversion pass alone without the resampler, conversion + k_resample with it --
in microseconds per frame, median and range over the rounds.  Beside it what the shapes say: bytes and multiply-adds a frame.
(k_resample alone: run this under rocprofv3 --kernel-trace --output-format csv with --rounds 1 and read its rows.)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from sdrreceiver_amd import _lib, ingest, resample as rs, topology as tp  # noqa: E402
from sdrreceiver_amd.receiver import Receiver  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--subs", type=int, default=1024)
args = ap.parse_args()


def wide_root() -> tp.Topology:
    """One main at 6.144 MS/s, d = 2, with four USB subs at d = 5 (48 kS/s)"""
    fs, n = 6144000, 1536000
    t = tp.Topology(fs=fs, frame=n, name="root6144")
    t.vfos.append(tp.VfoDesc(topic="MAIN0", parent=-1, fs=fs, decimate_count=2, mixer_freq=100000.0, demod_usb=False, cstyle=1, samples_per_buffer=n))
    for k in range(4):
        t.vfos.append(tp.VfoDesc(topic=f"USB{k:02d}", parent=0, fs=fs // 4, decimate_count=5, mixer_freq=50000.0 * (k + 1), filter_bw=0,
                                 gain=tp._g(0.05), samples_per_buffer=n // 4))
    return t


CASES = {"2.4 -> 1.536 MS/s into config 3": (tp.config3(args.subs), 2400000, 24),
         "6 -> 6.144 MS/s into a 6.144 MS/s root": (wide_root(), 6000000, 32)}


def frames_of(n, count=2):
    rng = np.random.default_rng(n)
    host = [(rng.integers(-2048, 2048, 2 * n)).astype(np.int16) for _ in range(count)]
    dev = [torch.from_numpy(v).cuda() for v in host]
    torch.cuda.synchronize()
    return dev


def ingest_us(rx, dev, n, frames):
    rx.enable_kernel_timing(True)  # (zeroes the sums)
    for k in range(frames):
        rx.process_device_fmt(dev[k % len(dev)].data_ptr(), n, ingest.CS16)
    rx.fetch()
    t = rx.kernel_times()["k_ingest"]
    return t["ms"] / t["launches"] * 1e3  # (one bracket a frame: the conversion, and k_resample inside it)


out = {"build_id": _lib.lib().sdrx_build_id().decode(), "rounds": args.rounds, "frames_per_round": args.frames, "cases": {}}
for name, (topo, fs_in, T) in CASES.items():
    L, M = rs.ratio(fs_in, topo.fs)
    n, n_in = topo.frame, rs.in_frame(fs_in, topo.fs, topo.frame)
    pair = {"off": (Receiver.from_topology(topo), frames_of(n), n),
            "on": (Receiver.from_topology(topo, input_rate=fs_in, resample_taps=T), frames_of(n_in), n_in)}
    for rx, dev, m in pair.values():
        rx.set_publish(False)
        ingest_us(rx, dev, m, 4)  # warm-up
    us = {"off": [], "on": []}
    for r in range(args.rounds):
        for key in (("off", "on") if r % 2 == 0 else ("on", "off")):
            rx, dev, m = pair[key]
            us[key].append(ingest_us(rx, dev, m, args.frames))
    info = pair["on"][0].resampler
    out["cases"][name] = {
        "L": L, "M": M, "taps_per_phase": T, "in_frame": n_in, "out_frame": n, "passband_hz": round(info["passband_hz"], 1),
        "ingest_us_per_frame": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in us.items()},
        # what the shapes say: the conversion reads 4 B and writes 8 B a sample; k_resample reads the staged frame and the taps
        # once and writes the tree's frame; two products and two sums a tap and output
        "bytes_per_frame": {"conversion_off": 12 * n, "conversion_on": 12 * n_in, "k_resample": 8 * n_in + 8 * n + 4 * L * T},
        "multiply_adds_per_frame": 2 * T * n,
        "device_bytes_grown": pair["on"][0].stats()["device_bytes"] - pair["off"][0].stats()["device_bytes"]}
    for rx, _, _ in pair.values():
        rx.close()
print(json.dumps(out))
