#!/usr/bin/env python3
"""tools/park_time.py -- what option "park" costs and what a parked leaf saves.

    python3 tools/park_time.py [--steps K] [--warmup W] [--rounds R] [--skip-10k] [--out FILE]

On BASELINE config 3 (1 024 sub VFOs) and on the 10 240-sub tree, frames through sdrx_process_device:
  * ms per step with park = 0 and with park = 1 and every leaf active, interleaved over R rounds (the cost of the flag test);
  * ms per step with park = 1 and 0, 1/2, 7/8 and all but one of the sub VFOs parked, and for each the k_mix_levels /
    k_usb_demod times of sdrx_enable_kernel_timing (a separate, shorter run: the event pairs cost launch overlap);
  * the wall and device time of one sdrx_set_active call that unparks 1, 64 and 1 024 leaves (each restarts an oscillator: a
    serial replay of the table per leaf, as in tools/retune_time.py).
Prints one JSON line.
"""
import argparse
import ctypes as C
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


def kernel_times(rx, src, frame, steps):
    from sdrreceiver_amd import _lib
    rx._chk(rx.L.sdrx_enable_kernel_timing(rx.h, 1))
    for _ in range(steps):
        rx.process_device(src.data_ptr(), frame)
    ms = (C.c_double * _lib.NKERNELS)()
    n = (C.c_int64 * _lib.NKERNELS)()
    rx._chk(rx.L.sdrx_get_kernel_times(rx.h, ms, n, None))
    out = {}
    for k in range(_lib.NKERNELS):
        if n[k]:
            out[rx.L.sdrx_kernel_name(k).decode()] = round(ms[k] / n[k] * 1e3, 2)  # us per launch
    rx._chk(rx.L.sdrx_enable_kernel_timing(rx.h, 0))
    return out


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
        for park in (0, 1):
            rx = Receiver.from_topology(topo, device=0, park=bool(park))
            rx.set_publish(False)
            rx.set_stream(stream.cuda_stream)
            rxs[park] = rx
        ab = {0: [], 1: []}
        for _ in range(a.rounds):  # interleaved: park = 0, park = 1 (all active), ...
            for park in (0, 1):
                ab[park].append(run_steps(rxs[park], src, topo.frame, a.steps, a.warmup))
        res = {"subs": len(subs)}
        for park in (0, 1):
            res[f"park{park}_all_active_ms"] = {"median": round(statistics.median(ab[park]), 4), "min": round(min(ab[park]), 4),
                                                "max": round(max(ab[park]), 4)}
        rxs[0].close()
        rx = rxs[1]
        shares = {}
        for label, n_parked in (("0", 0), ("1/2", len(subs) // 2), ("7/8", len(subs) * 7 // 8), ("all_but_one", len(subs) - 1)):
            rx.set_active(subs, [1] * len(subs))
            if n_parked:
                rx.set_active(subs[:n_parked], [0] * n_parked)
            t = [run_steps(rx, src, topo.frame, a.steps, a.warmup) for _ in range(max(1, a.rounds // 2))]
            shares[label] = {"parked": n_parked, "ms_per_step": round(statistics.median(t), 4),
                             "kernel_us": kernel_times(rx, src, topo.frame, min(a.steps, 50))}
        res["parked_share"] = shares
        calls = {}
        for n_un in (1, 64, 1024):
            if n_un > len(subs):
                continue
            dev_ms, wall_ms = [], []
            for r in range(4):
                rx.set_active(subs[:n_un], [0] * n_un)
                rx.process_device(src.data_ptr(), topo.frame)
                rx.sync()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                t0 = time.perf_counter()
                rx.set_active(subs[:n_un], [1] * n_un)
                t1 = time.perf_counter()
                e1.record(stream)
                e1.synchronize()
                if r:  # (the first call also allocates the job list)
                    dev_ms.append(e0.elapsed_time(e1))
                    wall_ms.append((t1 - t0) * 1e3)
            calls[str(n_un)] = {"device_ms": round(statistics.median(dev_ms), 3), "call_ms": round(statistics.median(wall_ms), 3)}
        res["unpark_call"] = calls
        rx.fetch()
        rx.close()
        result[name] = res
    line = json.dumps({"park_time": result})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
