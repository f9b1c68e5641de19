#!/usr/bin/env python3
"""tools/iq_time.py [--rounds R] [--frames F] [--subs N] -- what the IQ balance correction costs in the ingest group.

config 3's tree fed frames of 384 000 CS16 samples without DC removal, device-resident and queued back to back
(process_device_fmt, one fetch a round), with sdrx_enable_kernel_timing on; the figure is the ingest group of
sdrx_get_kernel_times in microseconds per frame, median and range over the rounds, for a receiver with the stage (mu = 2^-4, no
power floor) and one without, taking turns round by round.  The input is a tone of amplitude 40 in noise of sigma 4 through a front
end with 5 % gain and 3 degrees phase error -- the stage's arithmetic does not depend on the samples, so one input serves.
Beside them the record of the last frame, the residual imbalance it shows (iqbal.levels), and what the stage holds on the device."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from sdrreceiver_amd import _lib, ingest, iqbal as iq, topology as tp  # noqa: E402
from sdrreceiver_amd.receiver import Receiver  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--subs", type=int, default=1024)
args = ap.parse_args()
N = 384000
CFG = iq.Cfg(2.0 ** -4, 0.0)


def frame(rng, k):
    j = np.arange(N, dtype=np.float64)
    ph = 2 * np.pi * (37 + k) * j / N
    i, q = 40 * np.cos(ph) + 4 * rng.standard_normal(N), 40 * np.sin(ph) + 4 * rng.standard_normal(N)
    a = np.deg2rad(3.0)
    v = np.empty(2 * N)
    v[0::2], v[1::2] = i + 0.7, 1.05 * (q * np.cos(a) + i * np.sin(a)) - 0.3
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
for key, kw in (("off", {}), ("on", dict(iq_balance=CFG))):
    rx = Receiver.from_topology(tp.config3(args.subs), **kw)
    rx.set_publish(False)
    times_us(rx, dev, 4)  # warm-up
    pair[key] = rx
us = {"off": {}, "on": {}}
for r in range(args.rounds):
    for key in (("off", "on") if r % 2 == 0 else ("on", "off")):
        for kind, v in times_us(pair[key], dev, args.frames).items():
            us[key].setdefault(kind, []).append(v)
rec = pair["on"].iq_balance
out = {"build_id": _lib.lib().sdrx_build_id().decode(), "rounds": args.rounds, "frames_per_round": args.frames, "frame": N,
       "cfg": [CFG.mu, CFG.min_power, CFG.c0, CFG.d0], "us_per_frame": {key: {kind: summary(v) for kind, v in us[key].items()} for key in us},
       "record": {k: rec[k] for k in iq.RECORD_FIELDS}, "pair": [iq.from_bits(rec["next_c_bits"]), iq.from_bits(rec["next_d_bits"])],
       "levels": iq.levels(rec), "device_bytes": {key: pair[key].stats()["device_bytes"] for key in pair}}
for rx in pair.values():
    rx.close()
print(json.dumps(out))
