#!/usr/bin/env python3
"""tools/wake_time.py -- what the device-side wake costs per frame, and what a wake frame costs against sdrx_set_active.

    python3 tools/wake_time.py [--steps K] [--warmup W] [--rounds R] [--skip-10k] [--out FILE]

On BASELINE config 3 (1 024 sub VFOs) and on the 10 240-sub tree, option wake = 1, every sub parked and watched, frames through
sdrx_process_device, interleaved over R rounds:
  (a) the watch alone: no sub under control;
  (b) every sub under wake control, nothing hot (min_band_pwr 1e300): (b) - (a) is what one k_watch_wake launch per source
      group adds per frame when nothing changes;
  (c) a WAKE FRAME: n = 1, 64 and all subs made hot (min_band_pwr 0) before one frame, which wakes them and runs them -- against
      one sdrx_set_active call that unparks the same leaves on the same build plus the frame that then runs them.  What differs
      is the host round trip and the oscillator replay of k_vfo_retune, which a wake does not pay.
k_watch_wake is not bracketed by sdrx_enable_kernel_timing (SDRX_NKERNELS stays 8): its own time needs a kernel trace.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLD, HOT = 1e300, 0.0


def run_steps(rx, src, frame, steps, warmup):
    for _ in range(warmup):
        rx.process_device(src.data_ptr(), frame)
    rx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        rx.process_device(src.data_ptr(), frame)
    rx.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def one_frame(rx, src, frame):
    t0 = time.perf_counter()
    rx.process_device(src.data_ptr(), frame)
    rx.sync()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


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
        for case in ("a_watched", "b_controlled_cold", "c_wake", "c_set_active"):
            rx = Receiver.from_topology(topo, device=0, wake=True)
            rx.set_publish(False)
            rx.set_stream(stream.cuda_stream)
            rx.set_active(subs, [0] * len(subs))
            rx.set_watch(subs, [1] * len(subs))
            if case in ("b_controlled_cold", "c_wake"):
                rx.set_wake(subs, COLD)
            rxs[case] = rx
        t = {"a_watched": [], "b_controlled_cold": []}
        for _ in range(a.rounds):
            for case in t:
                t[case].append(run_steps(rxs[case], src, topo.frame, a.steps, a.warmup))
        res = {"subs": len(subs), "sources": len({topo.vfos[i].parent for i in subs}),
               "device_bytes": {case: rx.stats()["device_bytes"] for case, rx in rxs.items()}}
        for case in t:
            res[case + "_ms"] = stats(t[case])
        res["wake_step_adds_ms"] = round(statistics.median(t["b_controlled_cold"]) - statistics.median(t["a_watched"]), 4)
        wk, sa = rxs["c_wake"], rxs["c_set_active"]
        for rx in (wk, sa):
            run_steps(rx, src, topo.frame, 1, a.warmup)
        res["wake_frame"] = {}
        for n in (1, 64, len(subs)):
            ids = subs[:n]
            wake_ms, call_ms, frame_ms = [], [], []
            for _ in range(a.rounds):
                wk.set_wake(ids, HOT)                   # (between frames: the settings only -- the leaves stay parked)
                wake_ms.append(one_frame(wk, src, topo.frame))  # the frame that wakes and runs them
                assert int(wk.active(ids[:1])["active"][0]) == 1
                wk.set_wake(ids, COLD)
                one_frame(wk, src, topo.frame)          # ... and the one that parks them again
                t0 = time.perf_counter()
                sa.set_active(ids, [1] * n)
                call_ms.append((time.perf_counter() - t0) * 1e3)
                frame_ms.append(one_frame(sa, src, topo.frame))
                sa.set_active(ids, [0] * n)
                one_frame(sa, src, topo.frame)
            res["wake_frame"][str(n)] = {"wake_frame_ms": stats(wake_ms), "set_active_call_ms": stats(call_ms),
                                         "frame_behind_set_active_ms": stats(frame_ms)}
        for rx in rxs.values():
            rx.fetch()
            rx.close()
        result[name] = res
    line = json.dumps({"wake_time": result})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
