#!/usr/bin/env python3
"""tools/watch_time.py -- what watching a parked tree costs, against what running it costs.

    python3 tools/watch_time.py [--steps K] [--warmup W] [--rounds R] [--skip-10k] [--out FILE]

On BASELINE config 3 (1 024 sub VFOs) and on the 10 240-sub tree, options park = 1 and watch = 1, frames through
sdrx_process_device, interleaved over R rounds:
  (a) every sub parked, none watched;
  (b) every sub parked, every sub watched;
  (c) every sub active, none watched.
(b) - (a) is what the watch adds per frame -- one k_watch_psd and one k_watch_bands launch per source group; the two kernels are
not bracketed by sdrx_enable_kernel_timing (SDRX_NKERNELS stays 8), so their split needs a kernel trace
(rocprofv3 --kernel-trace --stats -- python3 tools/watch_time.py --skip-10k --rounds 1).  The claim to check is
(b) - (a) << (c) - (a).  Prints one JSON line.
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
    ap.add_argument("--skip-10k", action="store_true")
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    from sdrreceiver_amd import _lib, synth, topology as tp
    from sdrreceiver_amd.receiver import Receiver

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    cases = [("config3_1024_subs", tp.config3(1024))]
    if not a.skip_10k:
        cases.append(("north_star_10240_subs", tp.config3(10240)))
    result = {"build_id": _lib.lib().sdrx_build_id().decode()}
    for name, topo in cases:
        subs = [i for i, v in enumerate(topo.vfos) if v.parent >= 0]
        src = torch.from_numpy(np.ascontiguousarray(synth.lcg_frame(topo.frame, synth.Lcg(1)), np.float32)).cuda()
        rxs = {}
        for case in ("a_parked", "b_parked_watched", "c_active"):
            rx = Receiver.from_topology(topo, device=0, park=True, watch=True)
            rx.set_publish(False)
            rx.set_stream(stream.cuda_stream)
            if case != "c_active":
                rx.set_active(subs, [0] * len(subs))
            if case == "b_parked_watched":
                rx.set_watch(subs, [1] * len(subs))
            rxs[case] = rx
        t = {case: [] for case in rxs}
        for _ in range(a.rounds):
            for case, rx in rxs.items():
                t[case].append(run_steps(rx, src, topo.frame, a.steps, a.warmup))
        res = {"subs": len(subs), "sources": len({topo.vfos[i].parent for i in subs}),
               "device_bytes": {case: rx.stats()["device_bytes"] for case, rx in rxs.items()}}
        for case in rxs:
            res[case + "_ms"] = {"median": round(statistics.median(t[case]), 4), "min": round(min(t[case]), 4), "max": round(max(t[case]), 4)}
        med = {case: statistics.median(t[case]) for case in rxs}
        res["watch_adds_ms"] = round(med["b_parked_watched"] - med["a_parked"], 4)
        res["running_adds_ms"] = round(med["c_active"] - med["a_parked"], 4)
        lv = rxs["b_parked_watched"].watch(subs[:4])
        res["sample_levels"] = {k: [float(x) for x in v] for k, v in lv.items()}
        for rx in rxs.values():
            rx.fetch()
            rx.close()
        result[name] = res
    line = json.dumps({"watch_time": result})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
