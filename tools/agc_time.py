#!/usr/bin/env python3
"""tools/agc_time.py -- what option "agc" (the per-leaf gain step behind every frame) adds per frame over option "meter".

    python3 tools/agc_time.py [--steps K] [--warmup W] [--reps R] [--skip-10k] [--out FILE]

BASELINE config 3 (1 024 subs) and the north-star tree of 10 240 subs, frames through sdrx_process_device back to back on the
torch stream (the flagship path of bench.py: kernels only), with meter = 1 and with agc = 1 -- every USB leaf given a window, so
the step does all its work -- each with fuse_demod 0 and 1: on a fuse_demod tree "agc" also takes the planner rules of
"preroll" (no tail_in_levels).  The time of K frames is taken between device events after W warm-up frames; the receivers of
one tree are timed in turn (R rounds) and the median per-frame time is reported with min, max and the added ms per frame.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-10k", action="store_true")
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    from sdrreceiver_amd import synth, topology as tp
    from sdrreceiver_amd.receiver import Receiver

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    result = {}
    trees = [("config3", tp.config3(1024))]
    if not a.skip_10k:
        trees.append(("10k", tp.config3(10240)))
    for name, topo in trees:
        host = synth.lcg_frame(topo.frame, synth.Lcg(1))
        src = torch.from_numpy(np.ascontiguousarray(host, np.float32)).cuda()
        usb = [i for i in topo.leaves_in_publish_order() if topo.vfos[i].demod_usb]
        keys = [(fd, on) for fd in (False, True) for on in (False, True)]
        rxs = {}
        for fd, on in keys:
            rx = Receiver.from_topology(topo, device=0, meter=True, agc=on, fuse_demod=fd)
            rx.set_publish(False)
            rx.set_stream(stream.cuda_stream)
            if on:  # a window no frame leaves: the step folds, compares and writes its record for every leaf
                rx.set_agc(usb, 1, 1 << 30, 0, 0, 1.25, 0.5, 1e-6, 1e6)
            rxs[(fd, on)] = rx
        times = {k: [] for k in keys}
        for _ in range(a.reps):
            for k in keys:
                rx = rxs[k]
                for _ in range(a.warmup):
                    rx.process_device(src.data_ptr(), topo.frame)
                rx.sync()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.steps):
                    rx.process_device(src.data_ptr(), topo.frame)
                rx.sync()
                e1.record(stream)
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.steps)
        for fd in (False, True):
            base = statistics.median(times[(fd, False)])
            for on in (False, True):
                t = times[(fd, on)]
                med = statistics.median(t)
                result[f"{name}_fuse_demod{int(fd)}_{'agc' if on else 'meter'}"] = {
                    "ms_per_frame": round(med, 5), "min": round(min(t), 5), "max": round(max(t), 5),
                    "added_ms": round(med - base, 5), "added_pct": round(100.0 * (med - base) / base, 2),
                    "device_bytes": rxs[(fd, on)].stats()["device_bytes"]}
        for rx in rxs.values():
            rx.close()
        del rxs
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
