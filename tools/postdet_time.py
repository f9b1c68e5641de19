#!/usr/bin/env python3
"""tools/postdet_time.py [--rounds R] [--frames F] [--subs N] -- what the post-detection filter costs on a detector leaf.

config 3's tree three times, all N subs as FM leaves (the same mixers, rates and gains; demod_usb off): without the filter (the
yardstick: k_detect), with T = 64 taps and R = 6 (a voice channel: 48 kS/s to 8 kS/s), and with T = 256 taps and R = 1 (the most
arithmetic the limits allow: about 3e9 multiply-add pairs a frame).  Device-resident cf32 frames queued back to back through
sdrx_process_device, one fetch a round; wall clock per frame with a device synchronisation behind the round, the three receivers
taking turns round by round.  Reported: median [min, max] ms per frame, the launches per frame of every bracketed kernel kind (the
filtered leaves' launches are booked with k_compress), the payload bytes per frame and the device bytes."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from sdrreceiver_amd import _lib, detect as dt, postdet as pd, synth, topology as tp  # noqa: E402
from sdrreceiver_amd.receiver import Receiver  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--subs", type=int, default=1024)
args = ap.parse_args()

VARIANTS = (("plain", 0, 1, 0.0), ("t64_r6", 64, 6, 3000.0), ("t256_r1", 256, 1, 3000.0))


def tree(T, R, cutoff):
    t = tp.config3(args.subs)
    out = []
    for v in t.vfos:
        if v.parent >= 0:
            v = dataclasses.replace(v, demod_usb=False, filter_bw=0, cstyle=0, detector=dt.FM)
            if T:
                v = dataclasses.replace(v, post_taps=tuple(pd.design(v.out_rate_stage, cutoff, T, 60.0)[0].tolist()), post_decim=R)
        out.append(v)
    t.vfos = out
    return t


def run(rx, dev, n, frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(frames):
        rx.process_device(dev[k % len(dev)].data_ptr(), n)
    rx.fetch()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / frames * 1e3


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


topo = tree(0, 1, 0.0)
lcg = synth.Lcg(1)
dev = [torch.from_numpy(synth.lcg_frame(topo.frame, lcg)).cuda() for _ in range(2)]
torch.cuda.synchronize()
rxs = {}
for key, T, R, cutoff in VARIANTS:
    rx = Receiver.from_topology(tree(T, R, cutoff))
    rx.set_publish(False)
    run(rx, dev, topo.frame, 4)  # warm-up
    rxs[key] = rx
ms = {key: [] for key in rxs}
order = list(rxs)
for r in range(args.rounds):
    for key in order[r % 3:] + order[:r % 3]:
        ms[key].append(run(rxs[key], dev, topo.frame, args.frames))
launches = {}
for key, rx in rxs.items():
    rx.enable_kernel_timing(True)
    run(rx, dev, topo.frame, args.frames)
    launches[key] = {k: round(v["launches"] / args.frames, 3) for k, v in rx.kernel_times().items()}
    rx.enable_kernel_timing(False)
out = {"build_id": _lib.lib().sdrx_build_id().decode(), "rounds": args.rounds, "frames_per_round": args.frames, "subs": args.subs,
       "ms_per_frame": {key: summary(v) for key, v in ms.items()}, "launches_per_frame": launches,
       "payload_bytes_per_frame": {key: int(sum(2 * d.n_detect_out for d in rx.descs if d.parent >= 0)) for key, rx in rxs.items()},
       "device_bytes": {key: rx.stats()["device_bytes"] for key, rx in rxs.items()}}
for rx in rxs.values():
    rx.close()
print(json.dumps(out))
