#!/usr/bin/env python3
"""tools/meter_time.py -- what option "meter" (per-leaf output meters) adds per frame.

    python3 tools/meter_time.py [--steps K] [--warmup W] [--reps R] [--skip-10k] [--out FILE]

BASELINE config 3 (1 024 subs) and the north-star tree of 10 240 subs (bench.py --workload 10k), each with meter off and on, in
two forms: frames through sdrx_process_device back to back on the torch stream (the flagship path of bench.py: kernels only)
and the streaming host's submit(f+1); wait() (kernels plus the payload copy, which carries the records).  The time of K frames
is taken between device events (device form) or on the host clock around work that ends in a wait (streaming form) after W
warm-up frames; the two receivers of one tree are timed in turn (R rounds) and the median per-frame time is reported with
the added ms per frame and the record bytes per frame.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
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
        rxs = {}
        for on in (False, True):
            rx = Receiver.from_topology(topo, device=0, meter=on)
            rx.set_publish(False)
            rx.set_stream(stream.cuda_stream)
            rxs[on] = rx
        times = {(form, on): [] for form in ("device", "stream") for on in (False, True)}
        for _ in range(a.reps):
            for on in (False, True):
                rx = rxs[on]
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
                times[("device", on)].append(e0.elapsed_time(e1) / a.steps)
                rx.submit(host)
                for _ in range(a.warmup):
                    rx.submit(host)
                    rx.wait()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    rx.submit(host)
                    rx.wait()
                times[("stream", on)].append((time.perf_counter() - t0) * 1e3 / a.steps)
                rx.wait()
        st = rxs[True].stats()
        for form in ("device", "stream"):
            base = statistics.median(times[(form, False)])
            for on in (False, True):
                med = statistics.median(times[(form, on)])
                result[f"{name}_{form}_meter{int(on)}"] = {"ms_per_frame": round(med, 5), "min": round(min(times[(form, on)]), 5),
                                                          "max": round(max(times[(form, on)]), 5),
                                                          "added_ms": round(med - base, 5),
                                                          "added_pct": round(100.0 * (med - base) / base, 2)}
        result[f"{name}_device_bytes"] = {"meter0": rxs[False].stats()["device_bytes"], "meter1": st["device_bytes"]}
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
