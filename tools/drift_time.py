#!/usr/bin/env python3
"""tools/drift_time.py -- what the drift estimate adds to a watched tree per frame.

    python3 tools/drift_time.py [--steps K] [--warmup W] [--rounds R] [--out FILE]

BASELINE config 3 (1 024 sub VFOs, two sources), option watch = 1 with every sub watched, frames through sdrx_process_device,
interleaved over R rounds:
  (a) no drift estimate;
  (b) both sources with a captured template, max_shift 64;
  (c) both sources with a captured template, max_shift 1 024.
(b) - (a) and (c) - (a) are what one k_watch_drift launch per source group adds: 2 sources x (2K + 1) shifts x 8 192 double
multiply-adds, in 3 (K = 64) or 33 (K = 1 024) workgroups per source.  The kernel is not bracketed by sdrx_enable_kernel_timing
(SDRX_NKERNELS stays 8): its own time needs a kernel trace (rocprofv3 --kernel-trace --stats -- python3 tools/drift_time.py
--rounds 1).  Prints one JSON line.
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
    from sdrreceiver_amd import _lib, drift, synth, topology as tp
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
    for case, K in (("a_watched", 0), ("b_drift_64", 64), ("c_drift_1024", 1024)):
        rx = Receiver.from_topology(topo, device=0, watch=True)
        rx.set_publish(False)
        rx.set_stream(stream.cuda_stream)
        rx.set_watch(subs, [1] * len(subs))
        if K:
            for leaf in one_per_source.values():
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
    res["drift_64_adds_ms"] = round(med["b_drift_64"] - med["a_watched"], 4)
    res["drift_1024_adds_ms"] = round(med["c_drift_1024"] - med["a_watched"], 4)
    for rx in rxs.values():
        rx.fetch()
    res["sample_records"] = {case: [rxs[case].drift(leaf) for leaf in one_per_source.values()] for case in ("b_drift_64", "c_drift_1024")}
    res["sample_estimate_bins"] = [drift.estimate_bins(r) for r in res["sample_records"]["b_drift_64"]]
    for rx in rxs.values():
        rx.close()
    line = json.dumps({"drift_time": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
