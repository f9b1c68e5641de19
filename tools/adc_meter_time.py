#!/usr/bin/env python3
"""tools/adc_meter_time.py [--rounds R] [--frames F] -- what option adc_meter costs.

Config 3's tree and its 384 000-sample frame through the ABI, pipelined (submit_fmt(f+1); wait() -> f), fed dongle bytes
without DC removal, int16 without it, and int16 with the exact DC-bias removal: two receivers per case, the option on and off,
taking turns round by round in one process, so that whatever drifts on the machine drifts under both.  Per case the median and
the range of the rounds' ms per frame for each, and what device_bytes grows by.  (The kernel's own length: run this under
rocprofv3 --kernel-trace --stats with --rounds 1 and read k_adc_meter's row.)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from sdrreceiver_amd import _lib, ingest, synth, topology as tp  # noqa: E402
from sdrreceiver_amd.receiver import Receiver  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--subs", type=int, default=1024)
args = ap.parse_args()

topo = tp.config3(args.subs)
cap = synth.capture_like_u8(4, topo.frame, topo.fs)
u8 = [np.minimum(cap[2 * topo.frame * f: 2 * topo.frame * (f + 1)], 254) for f in range(4)]  # (byte 255 has no signed image)
s16 = [((b.astype(np.int32) - 127) * 256).astype(np.int16) for b in u8]
CASES = {"cu8": (u8, False), "cs16": (s16, False), "cs16 + dc": (s16, True)}


def run(rx, feed, dc, frames):
    t0 = time.perf_counter()
    rx.submit_fmt(feed[0], correct_dc=dc)
    for k in range(1, frames):
        rx.submit_fmt(feed[k % len(feed)], correct_dc=dc)
        rx.wait()
    rx.wait()
    return (time.perf_counter() - t0) / frames * 1e3


out = {"build_id": _lib.lib().sdrx_build_id().decode(), "frame": topo.frame, "rounds": args.rounds, "frames_per_round": args.frames,
       "ms_per_frame": {}}
for name, (feed, dc) in CASES.items():
    pair = {"off": Receiver.from_topology(topo), "on": Receiver.from_topology(topo, adc_meter=True)}
    for rx in pair.values():
        rx.set_publish(False)
        run(rx, feed, dc, 16)  # warm-up: the DC estimate sits where it lives, every buffer exists
    ms = {"off": [], "on": []}
    for r in range(args.rounds):
        for key in (("off", "on") if r % 2 == 0 else ("on", "off")):
            ms[key].append(run(pair[key], feed, dc, args.frames))
    rec = pair["on"].adc_meter()
    assert rec["measured"] == 1 and rec["n_complex"] == topo.frame and rec["fmt"] == ingest.infer_format(feed[0])
    out["ms_per_frame"][name] = {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                                 for k, v in ms.items()}
    out["device_bytes_grown"] = pair["on"].stats()["device_bytes"] - pair["off"].stats()["device_bytes"]
    for rx in pair.values():
        rx.close()
print(json.dumps(out))
