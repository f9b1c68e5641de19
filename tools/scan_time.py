#!/usr/bin/env python3
"""tools/scan_time.py -- what the band scan adds to a watched tree per frame.

    python3 tools/scan_time.py [--steps K] [--warmup W] [--rounds R] [--out FILE]

BASELINE config 3 (1 024 sub VFOs, two sources), option watch = 1 with every sub watched, frames through sdrx_process_device,
interleaved over R rounds:
  (a) no scan;
  (b) both sources scanned, cell_bins 4, frames 1 (an evaluation every frame), floor_permille 500, ratio 16;
  (c) (b) and a drift estimate with max_shift 64 on both sources.
(b) - (a) is what one k_watch_scan launch per source group adds.  The kernel is not bracketed by sdrx_enable_kernel_timing
(SDRX_NKERNELS stays 8): its own time beside k_watch_psd's and k_watch_drift's needs a kernel trace
(rocprofv3 --kernel-trace --stats -- python3 tools/scan_time.py --rounds 1).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_steps(rx, src, frame, steps, warmup):
    for _ in range(warmup):
        rx.process_device(src.data_ptr(), frame)
    rx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        rx.process_device(src.data_ptr(), frame)
    rx.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    from sdrreceiver_amd import _lib, synth, topology as tp
    from sdrreceiver_amd.receiver import Receiver

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    topo = tp.config3(1024)
    subs = [i for i, v in enumerate(topo.vfos) if v.parent >= 0]
    one_per_source = {}
    for i in subs:
        one_per_source.setdefault(topo.vfos[i].parent, i)
    src = torch.from_numpy(np.ascontiguousarray(synth.lcg_frame(topo.frame, synth.Lcg(1)), np.float32)).cuda()
    rxs = {}
    for case, scan_on, K in (("a_watched", False, 0), ("b_scan", True, 0), ("c_scan_drift_64", True, 64)):
        rx = Receiver.from_topology(topo, device=0, watch=True)
        rx.set_publish(False)
        rx.set_stream(stream.cuda_stream)
        rx.set_watch(subs, [1] * len(subs))
        for leaf in one_per_source.values():
            if scan_on:
                rx.set_scan(leaf, cell_bins=4, frames=1, floor_permille=500, ratio_q8=16 * 256)
            if K:
                rx.set_drift(leaf, None, K)
        rxs[case] = rx
    t = {case: [] for case in rxs}
    for _ in range(a.rounds):
        for case, rx in rxs.items():
            t[case].append(run_steps(rx, src, topo.frame, a.steps, a.warmup))
    res = {"build_id": _lib.lib().sdrx_build_id().decode(), "subs": len(subs), "sources": len(one_per_source),
           "device_bytes": {case: rx.stats()["device_bytes"] for case, rx in rxs.items()}}
    for case in rxs:
        res[case + "_ms"] = {"median": round(statistics.median(t[case]), 4), "min": round(min(t[case]), 4), "max": round(max(t[case]), 4)}
    med = {case: statistics.median(t[case]) for case in rxs}
    res["scan_adds_ms"] = round(med["b_scan"] - med["a_watched"], 4)
    for rx in rxs.values():
        rx.fetch()
    res["sample_records"] = [rxs["b_scan"].scan(leaf) for leaf in one_per_source.values()]
    for rx in rxs.values():
        rx.close()
    line = json.dumps({"scan_time": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
