#!/usr/bin/env python3
"""tools/shift_time.py [--rounds R] [--frames F] [--subs N] [--calls K] -- what the frequency shift costs in the ingest group, and what
one sdrx_set_shift call costs.

config 3's tree fed frames of 384 000 CS16 samples without DC removal, device-resident and queued back to back
(process_device_fmt, one fetch a round), with sdrx_enable_kernel_timing on; the figure is the ingest group of
sdrx_get_kernel_times in microseconds per frame, median and range over the rounds, for a receiver with the stage (a shift of
-1234.5 Hz) and one without, taking turns round by round.  The stage's arithmetic does not depend on the samples or on the
increment, so one input serves.
The setter: K sdrx_set_shift calls on the idle receiver (another increment each), wall clock per call without and with a
device synchronisation behind the last -- the call drains the pipeline and queues one one-thread launch.
Beside them the record of the last frame and what the stage holds on the device."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from sdrreceiver_amd import _lib, ingest, shift as sh, topology as tp  # noqa: E402
from sdrreceiver_amd.receiver import Receiver  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--subs", type=int, default=1024)
ap.add_argument("--calls", type=int, default=200)
args = ap.parse_args()
N = 384000
HZ = -1234.5


def frame(rng, k):
    j = np.arange(N, dtype=np.float64)
    ph = 2 * np.pi * (37 + k) * j / N
    v = np.empty(2 * N)
    v[0::2], v[1::2] = 40 * np.cos(ph) + 4 * rng.standard_normal(N), 40 * np.sin(ph) + 4 * rng.standard_normal(N)
    return np.clip(np.rint(v * 256), -32768, 32767).astype(np.int16)


def times_us(rx, dev, frames):
    rx.enable_kernel_timing(True)  # (zeroes the sums)
    for k in range(frames):
        rx.process_device_fmt(dev[k % len(dev)].data_ptr(), N, ingest.CS16)
    rx.fetch()
    return {k: v["ms"] / frames * 1e3 for k, v in rx.kernel_times().items() if v["launches"]}


def summary(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


rng = np.random.default_rng(384)
dev = [torch.from_numpy(frame(rng, k)).cuda() for k in range(2)]
torch.cuda.synchronize()
pair = {}
for key, kw in (("off", {}), ("on", dict(shift=HZ))):
    rx = Receiver.from_topology(tp.config3(args.subs), **kw)
    rx.set_publish(False)
    times_us(rx, dev, 4)  # warm-up
    pair[key] = rx
us = {"off": {}, "on": {}}
for r in range(args.rounds):
    for key in (("off", "on") if r % 2 == 0 else ("on", "off")):
        for kind, v in times_us(pair[key], dev, args.frames).items():
            us[key].setdefault(kind, []).append(v)
rec = pair["on"].shift
# the setter, on the idle receiver
rx = pair["on"]
rx.enable_kernel_timing(False)
calls = {"call_us": [], "call_and_sync_us": []}
for r in range(args.rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.calls):
        rx.set_shift(inc=1000 * r + k)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    calls["call_us"].append((t1 - t0) / args.calls * 1e6)
    calls["call_and_sync_us"].append((t2 - t0) / args.calls * 1e6)
rx.process_device_fmt(dev[0].data_ptr(), N, ingest.CS16)
rx.fetch()
last = rx.shift
assert last["inc"] == 1000 * (args.rounds - 1) + args.calls - 1 and last["phase"] == rec["next_phase"]  # the phase carried on
out = {"build_id": _lib.lib().sdrx_build_id().decode(), "rounds": args.rounds, "frames_per_round": args.frames, "frame": N, "hz": HZ,
       "us_per_frame": {key: {kind: summary(v) for kind, v in us[key].items()} for key in us},
       "set_shift": {"calls_per_round": args.calls, **{k: summary(v) for k, v in calls.items()}},
       "record": {k: rec[k] for k in sh.RECORD_FIELDS}, "device_bytes": {key: pair[key].stats()["device_bytes"] for key in pair}}
for rx in pair.values():
    rx.close()
print(json.dumps(out))
