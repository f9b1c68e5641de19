#!/usr/bin/env python3
"""tools/spectrum_time.py -- what the device spectrum display adds per frame.

    python3 tools/spectrum_time.py [--steps K] [--warmup W] [--reps R] [--skip-10k] [--out FILE]

BASELINE config 3 (1 024 subs) with 0, 1 and 1 024 spectra, and the north-star tree of 10 240 subs (config 5's shape) with 0
and 10 240 spectra.  Frames go through sdrx_process_device back to back on the torch stream (the flagship path of bench.py);
the time of K frames is taken between device events after W warm-up frames, the receivers of one tree are timed in turn
(alternating with / without, R rounds), and the median per-frame time is reported with the added ms per frame.  The kernel's
own time comes from a separate `rocprofv3 --kernel-trace --stats` run over this script (k_spectrum's row); bytes per update
are 8 x n_in in, 64 KB of pwr read and written, 64 KB of bins written.  Prints one JSON line.
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
    trees = [("config3", tp.config3(1024), [0, 1, 1024])]
    if not a.skip_10k:
        trees.append(("10k", tp.config5(10240), [0, 10240]))
    for name, topo, counts in trees:
        src = torch.from_numpy(np.ascontiguousarray(synth.lcg_frame(topo.frame, synth.Lcg(1)), np.float32)).cuda()
        subs = list(range(2, len(topo.vfos)))
        rxs = {}
        for n in counts:
            rx = Receiver.from_topology(topo, device=0)
            rx.set_publish(False)
            for v in subs[:n]:
                rx.set_spectrum(v)
            rx.set_stream(stream.cuda_stream)
            rxs[n] = rx
        times = {n: [] for n in counts}
        for _ in range(a.reps):
            for n in counts:
                rx = rxs[n]
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
                times[n].append(e0.elapsed_time(e1) / a.steps)
        base = statistics.median(times[counts[0]])
        for n in counts:
            med = statistics.median(times[n])
            upd_bytes = sum(8 * min(topo.vfos[v].samples_per_buffer >> topo.vfos[v].decimate_count, 8192) + 3 * 65536
                            for v in subs[:n])
            result[f"{name}_{n}"] = {"ms_per_frame": round(med, 5), "min": round(min(times[n]), 5),
                                     "max": round(max(times[n]), 5), "added_ms": round(med - base, 5),
                                     "spectrum_bytes_per_frame": upd_bytes}
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
