#!/usr/bin/env python3
"""tools/catchup_time.py -- what an unpark with catch-up costs (option "catchup").

    python3 tools/catchup_time.py [--rounds R] [--skip-10k] [--catchup both|0|1] [--out FILE]

On BASELINE config 3 (1 024 sub VFOs) and on the 10 240-sub tree: the wall time of ONE sdrx_set_active call that unparks 1, 64
and 1 024 leaves which were parked in the frame before, with catchup = 1 and with catchup = 0 (park = 1, preroll = 1) on the
same build, interleaved over R rounds.  With 0 the call restarts the oscillators (a serial replay of the table per leaf, as in
tools/park_time.py); with 1 it also runs one frame of the woken leaves.  `--catchup 0` runs on a checkout that does not know
the option (the parent commit's build): alternate the two checkouts by hand for the comparison of 0 against 0.
Prints one JSON line.
"""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_call(rx, src, frame, ids):
    """park `ids`, run a frame with them parked, then time the unpark"""
    rx.set_active(ids, [0] * len(ids))
    rx.process_device(src.data_ptr(), frame)
    rx.sync()
    t0 = time.perf_counter()
    rx.set_active(ids, [1] * len(ids))
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-10k", action="store_true")
    ap.add_argument("--catchup", default="both", choices=["both", "0", "1"])
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    from sdrreceiver_amd import _lib, synth, topology as tp
    from sdrreceiver_amd.receiver import Receiver

    knows = "catchup" in inspect.signature(Receiver.__init__).parameters
    forms = [0, 1] if a.catchup == "both" else [int(a.catchup)]
    if not knows:
        forms = [f for f in forms if f == 0]
    cases = [("config3_1024_subs", tp.config3(1024))]
    if not a.skip_10k:
        cases.append(("north_star_10240_subs", tp.config3(10240)))
    result = {"build_id": _lib.lib().sdrx_build_id().decode()}
    for name, topo in cases:
        subs = [i for i, v in enumerate(topo.vfos) if v.parent >= 0]
        src = torch.from_numpy(np.ascontiguousarray(synth.lcg_frame(topo.frame, synth.Lcg(1)), np.float32)).cuda()
        rxs = {}
        for cu in forms:
            kw = dict(catchup=True) if cu else dict(park=True, preroll=True)
            rx = Receiver.from_topology(topo, device=0, **kw)
            rx.set_publish(False)
            rx.process_device(src.data_ptr(), topo.frame)
            rxs[cu] = rx
        res = {"subs": len(subs)}
        for n_un in (1, 64, 1024):
            if n_un > len(subs):
                continue
            t = {cu: [] for cu in forms}
            for r in range(a.rounds + 1):
                for cu in forms:  # interleaved
                    ms = one_call(rxs[cu], src, topo.frame, subs[:n_un])
                    if r:  # (the first call also allocates the job list)
                        t[cu].append(ms)
            res[str(n_un)] = {f"catchup{cu}_call_ms": {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                              for cu, v in t.items()}
        for rx in rxs.values():
            rx.fetch()
            rx.close()
        result[name] = res
    line = json.dumps({"catchup_time": result})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
