#!/usr/bin/env python3
"""tools/notch_time.py [--rounds R] [--frames F] [--subs N] -- what the spur canceller costs in the ingest group.

config 3's tree fed frames of 384 000 CS16 samples without DC removal, device-resident and queued back to back
(process_device_fmt, one fetch a round), with sdrx_enable_kernel_timing on; the figure is the ingest group of
sdrx_get_kernel_times in microseconds per frame, median [min, max] over the rounds, for a receiver with one tone, one with eight
and one without the stage, taking turns round by round.  The input has a carrier 7 Hz beside the first tone: the stage's arithmetic
does not depend on the samples, but the record printed beside the figures shows it locked.  Beside them what the stage holds on the
device."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from sdrreceiver_amd import _lib, ingest, notch as nt, topology as tp  # noqa: E402
from sdrreceiver_amd.receiver import Receiver  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--subs", type=int, default=1024)
args = ap.parse_args()
N = 384000
HZ = [61234.5 + 37500.0 * k for k in range(8)]  # 100 bins apart
KW = dict(mu=0.25, afc_gain=1.0, min_coherence=0.5, max_pull_hz=100.0)


def frame(rng, k, fs):
    j = np.arange(k * N, (k + 1) * N, dtype=np.float64)
    ph = 2 * np.pi * (((HZ[0] + 7.0) / fs * j) % 1.0)
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


topo = tp.config3(args.subs)
fs = float(next(d.fs for d in topo.vfos if d.parent < 0))
rng = np.random.default_rng(384)
dev = [torch.from_numpy(frame(rng, k, fs)).cuda() for k in range(2)]
torch.cuda.synchronize()
pair = {}
for key, kw in (("off", {}), ("one", dict(notch=dict(hz=HZ[:1], **KW))), ("eight", dict(notch=dict(hz=HZ, **KW)))):
    rx = Receiver.from_topology(topo, **kw)
    rx.set_publish(False)
    times_us(rx, dev, 4)  # warm-up
    pair[key] = rx
us = {key: {} for key in pair}
order = list(pair)
for r in range(args.rounds):
    for key in order[r % 3:] + order[:r % 3]:
        for kind, v in times_us(pair[key], dev, args.frames).items():
            us[key].setdefault(kind, []).append(v)
rec = pair["one"].notch
out = {"build_id": _lib.lib().sdrx_build_id().decode(), "rounds": args.rounds, "frames_per_round": args.frames, "frame": N, "hz": HZ,
       "us_per_frame": {key: {kind: summary(v) for kind, v in us[key].items()} for key in us},
       "levels_one": rec["levels"], "blocks": rec["blocks"], "device_bytes": {key: pair[key].stats()["device_bytes"] for key in pair},
       "model_device_bytes": nt.device_bytes(N)}
for rx in pair.values():
    rx.close()
print(json.dumps(out))
