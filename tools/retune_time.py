#!/usr/bin/env python3
"""tools/retune_time.py -- how long sdrx_set_mixer_freqs takes.

    python3 tools/retune_time.py [--reps R] [--skip-10k] [--out FILE]

Retunes one 1.536 MS/s main, one sub, all 1 024 subs of BASELINE config 3 and all 10 240 subs of the north-star tree (config
5's shape), each R times between frames that run through sdrx_process_device on the torch stream (the library's stream is set
to it, so device events recorded around the call bracket exactly its upload and its k_vfo_retune launch).  Reports the median
device time between the events and the median wall time of the call (which returns once the device has applied the retune).
A retune replays the new NCO table once, a serial chain of Fs recurrence steps per VFO in one lane: expect milliseconds.
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


def main():
    ap = argparse.ArgumentParser()
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
    cases = [("main_1536k", tp.config1(), [0]), ("sub_384k", tp.config1(), [1]), ("config3_1024_subs", tp.config3(1024), None)]
    if not a.skip_10k:
        cases.append(("north_star_10240_subs", tp.config3(10240), None))
    result = {}
    for name, topo, ids in cases:
        if ids is None:
            ids = [i for i, v in enumerate(topo.vfos) if v.parent >= 0]
        src = torch.from_numpy(np.ascontiguousarray(synth.lcg_frame(topo.frame, synth.Lcg(1)), np.float32)).cuda()
        rx = Receiver.from_topology(topo, device=0)
        rx.set_publish(False)
        rx.set_stream(stream.cuda_stream)
        base = np.array([topo.vfos[i].mixer_freq for i in ids])
        dev_ms, wall_ms = [], []
        for r in range(a.reps + 1):
            rx.process_device(src.data_ptr(), topo.frame)
            rx.process_device(src.data_ptr(), topo.frame)
            rx.sync()  # (the call would run these first: not part of the retune)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            rx.set_mixer_freqs(ids, base + 100.0 * (r + 1))
            t1 = time.perf_counter()
            e1.record(stream)
            e1.synchronize()
            if r:  # (the first call also allocates the job list)
                dev_ms.append(e0.elapsed_time(e1))
                wall_ms.append((t1 - t0) * 1e3)
        rx.fetch()
        result[name] = {"vfos": len(ids), "fs": sorted({topo.vfos[i].fs for i in ids}),
                        "device_ms": round(statistics.median(dev_ms), 3), "call_ms": round(statistics.median(wall_ms), 3)}
        rx.close()
    line = json.dumps({"retune_latency": result})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
