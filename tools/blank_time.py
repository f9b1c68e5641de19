#!/usr/bin/env python3
"""tools/blank_time.py [--rounds R] [--frames F] [--subs N] -- what the impulse blanker costs in the ingest group.

config 3's tree fed frames of 384 000 CS16 samples without DC removal, device-resident and queued back to back
(process_device_fmt, one fetch a round), with sdrx_enable_kernel_timing on; the figure is the ingest group of
sdrx_get_kernel_times in microseconds per frame, median and range over the rounds, for a receiver with the blanker (ratio 32, the
median, G = 8) and one without, taking turns round by round.  Two inputs, because the histogram's contention depends on what the
samples are:
  "uniform": int16 components uniform in -2048 .. 2047 (what tools/front_time.py feeds);
  "noise and pulses": Gaussian noise of sigma = 8 dongle LSB with five 4-sample pulses of +-25 000 codes a frame -- nearly every
      sample in some 20 bins of the histogram.
Beside them the record of the last frame (hits, blanked, runs) and what the stage holds on the device."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from sdrreceiver_amd import _lib, blank as bl, ingest, topology as tp  # noqa: E402
from sdrreceiver_amd.receiver import Receiver  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--subs", type=int, default=1024)
args = ap.parse_args()
N = 384000
CFG = bl.Cfg(32.0, 0.0, 32768, 8)


def uniform(rng):
    return rng.integers(-2048, 2048, 2 * N).astype(np.int16)


def noise_and_pulses(rng):
    v = np.clip(np.rint(rng.standard_normal(2 * N) * 8.0 * 256), -32768, 32767).astype(np.int16)
    for j in rng.choice(N // 128 - 2, 5, replace=False):
        v[2 * (128 * j + 64): 2 * (128 * j + 68)] = rng.choice([-25000, 25000], size=8)
    return v


def times_us(rx, dev, frames):
    rx.enable_kernel_timing(True)  # (zeroes the sums)
    for k in range(frames):
        rx.process_device_fmt(dev[k % len(dev)].data_ptr(), N, ingest.CS16)
    rx.fetch()
    return {k: v["ms"] / frames * 1e3 for k, v in rx.kernel_times().items() if v["launches"]}


def summary(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


out = {"build_id": _lib.lib().sdrx_build_id().decode(), "rounds": args.rounds, "frames_per_round": args.frames, "frame": N,
       "cfg": [CFG.ratio, CFG.floor, CFG.rank_q16, CFG.guard], "inputs": {}}
for name, make in (("uniform", uniform), ("noise and pulses", noise_and_pulses)):
    rng = np.random.default_rng(384)
    dev = [torch.from_numpy(make(rng)).cuda() for _ in range(2)]
    torch.cuda.synchronize()
    pair = {}
    for key, kw in (("off", {}), ("on", dict(blanker=CFG))):
        rx = Receiver.from_topology(tp.config3(args.subs), **kw)
        rx.set_publish(False)
        times_us(rx, dev, 4)  # warm-up
        pair[key] = rx
    us = {"off": {}, "on": {}}
    for r in range(args.rounds):
        for key in (("off", "on") if r % 2 == 0 else ("on", "off")):
            for kind, v in times_us(pair[key], dev, args.frames).items():
                us[key].setdefault(kind, []).append(v)
    rec = pair["on"].blanker
    out["inputs"][name] = {"us_per_frame": {key: {kind: summary(v) for kind, v in us[key].items()} for key in us},
                           "record": {k: rec[k] for k in ("thr_bits", "ref_bin", "next_ref_bin", "hits", "blanked", "runs", "carry_in")},
                           "device_bytes": {key: pair[key].stats()["device_bytes"] for key in pair}}
    for rx in pair.values():
        rx.close()
    del pair, dev
    torch.cuda.empty_cache()
print(json.dumps(out))
