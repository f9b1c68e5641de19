#!/usr/bin/env python3
"""tools/squelch_time.py -- what squelch-gated egress costs and saves per streamed frame.

    python3 tools/squelch_time.py [--steps K] [--warmup W] [--reps R] [--skip-10k] [--parent-lib FILE] [--out FILE] [--auto]

BASELINE config 3 (1 024 subs) and the north-star tree of 10 240 subs in the streaming host's form submit(f+1); wait() (kernels
plus the payload copy), publish callback off.  Receivers, timed in turn (R rounds, the median per-frame time reported with
min and max): meter=1 squelch=0 (baseline b), and squelch=1 with 100 %, 50 %, 10 % and 1 % of the leaves open (threshold 0
for the open ones, 2^63 for the others, spread evenly over the tree).  --parent-lib FILE adds baseline (a): a library built
from the parent commit, loaded in a child process through SDRX_LIB (it lacks the squelch entry points, so the child asks for
none of them), plain options, timed in the same run.  Prints one JSON line.

Option preroll, at 10 % open: `preroll_10pct` is the `open_10pct` receiver's twin with preroll=1 and the same
static open set -- no leaf ever re-opens, so the difference to `open_10pct` is the gate's second form alone.  `rot_squelch_10pct`
and `rot_preroll_10pct` rotate the open set EVERY frame (set_squelch; submit; wait -- a set needs an empty queue, so these two
rows have no frame of look-ahead and compare with each other only): with preroll every open leaf is then pre-rolled and the
copy doubles.

--auto (option squelch_auto) times only the pair that isolates the scan's AUTO form: `squelch_10pct`, squelch=1
with the static 10 % open set, and `auto_10pct`, squelch_auto=1 with the same thresholds and ratio_q8 = 256, window 8 on EVERY
leaf.  The frame is the same each time, so every floor equals the leaf's sum_sq and a ratio of 1.0 gives thr_eff = max(thr, s):
the same leaves are open and the same bytes copied, while every lane does the whole floor arithmetic.  Run it under
`rocprofv3 --kernel-trace --stats` for the per-launch time of the two k_squelch_scan instantiations side by side.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW = ("sdrx_set_squelch", "sdrx_get_squelch", "sdrx_get_egress", "sdrx_group_set_squelch", "sdrx_group_get_squelch", "sdrx_group_get_egress",
       "sdrx_get_preroll", "sdrx_get_preroll_count", "sdrx_group_get_preroll", "sdrx_group_get_preroll_count",
       "sdrx_set_squelch_auto", "sdrx_get_squelch_auto", "sdrx_group_set_squelch_auto", "sdrx_group_get_squelch_auto")
FRACTIONS = (1.0, 0.5, 0.1, 0.01)


def timed(rx, host, steps, warmup):
    rx.submit(host)
    for _ in range(warmup):
        rx.submit(host)
        rx.wait()
    t0 = time.perf_counter()
    for _ in range(steps):
        rx.submit(host)
        rx.wait()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    rx.wait()
    return ms


def timed_rotating(rx, host, steps, warmup, lv, sets):
    def one(i):
        thr, hang = sets[i % len(sets)]
        rx.set_squelch(lv, thr, hang)
        rx.submit(host)
        rx.wait()
    for i in range(warmup):
        one(i)
    t0 = time.perf_counter()
    for i in range(steps):
        one(warmup + i)
    return (time.perf_counter() - t0) * 1e3 / steps


def summary(v):
    return {"ms_per_frame": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-10k", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--auto", action="store_true", help="only squelch=1 against squelch_auto=1 at the same 10 %% open set")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)  # tree name: time the loaded library once, plain options
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    from sdrreceiver_amd import _lib, synth, topology as tp
    if a.child:
        import ctypes
        probe = ctypes.CDLL(_lib.LIB_PATH)
        for name in NEW:
            if not hasattr(probe, name):
                _lib.SYMBOLS.pop(name, None)
    from sdrreceiver_amd.receiver import Receiver

    trees = {"config3": lambda: tp.config3(1024), "10k": lambda: tp.config3(10240)}
    if a.child:
        topo = trees[a.child]()
        host = synth.lcg_frame(topo.frame, synth.Lcg(1))
        rx = Receiver.from_topology(topo, device=0)
        rx.set_publish(False)
        print(json.dumps([timed(rx, host, a.steps, a.warmup) for _ in range(a.reps)]))
        rx.close()
        return
    result = {}
    for name in ["config3"] + ([] if a.skip_10k else ["10k"]):
        topo = trees[name]()
        lv = topo.leaves_in_publish_order()
        host = synth.lcg_frame(topo.frame, synth.Lcg(1))
        if a.auto:
            is_open = np.zeros(len(lv), bool)
            is_open[np.unique(np.linspace(0, len(lv) - 1, max(1, round(0.1 * len(lv)))).round().astype(int))] = True
            thr = [0 if x else 1 << 63 for x in is_open]
            pair = {"squelch_10pct": Receiver.from_topology(topo, device=0, squelch=True),
                    "auto_10pct": Receiver.from_topology(topo, device=0, squelch_auto=True)}
            for rx in pair.values():
                rx.set_publish(False)
                rx.set_squelch(lv, thr, [0] * len(lv))
            pair["auto_10pct"].set_squelch_auto(lv, [256] * len(lv), [8] * len(lv))
            times = {k: [] for k in pair}
            for r in range(a.reps):
                for k, rx in pair.items():
                    times[k].append(timed(rx, host, a.steps, a.warmup))
            for k, rx in pair.items():
                eg = rx.egress()
                result[f"{name}_{k}"] = dict(summary(times[k]), n_open=eg["n_open"], payload_bytes_copied=eg["payload_bytes_copied"],
                                             device_bytes=rx.stats()["device_bytes"])
            au = pair["auto_10pct"].squelch_auto(lv)
            result[f"{name}_auto_10pct"].update(floor_valid=int(au["floor_valid"].sum()), lifted=int((au["thr_eff_sum_sq"] > 0).sum()))
            for rx in pair.values():
                rx.close()
            continue
        rxs = {"meter1_squelch0": Receiver.from_topology(topo, device=0, meter=True)}
        for frac in FRACTIONS:
            rx = Receiver.from_topology(topo, device=0, squelch=True)
            n_open = max(1, round(frac * len(lv)))
            is_open = np.zeros(len(lv), bool)
            is_open[np.unique(np.linspace(0, len(lv) - 1, n_open).round().astype(int))] = True
            rx.set_squelch(lv, [0 if x else 1 << 63 for x in is_open], [0] * len(lv))
            rxs[f"open_{round(100 * frac)}pct"] = rx
        static10 = np.zeros(len(lv), bool)
        static10[np.unique(np.linspace(0, len(lv) - 1, max(1, round(0.1 * len(lv)))).round().astype(int))] = True
        rxs["preroll_10pct"] = Receiver.from_topology(topo, device=0, preroll=True)
        rxs["preroll_10pct"].set_squelch(lv, [0 if x else 1 << 63 for x in static10], [0] * len(lv))
        rot = {"rot_squelch_10pct": Receiver.from_topology(topo, device=0, squelch=True),
               "rot_preroll_10pct": Receiver.from_topology(topo, device=0, preroll=True)}
        hang0 = np.zeros(len(lv), np.uint32)
        sets = [(np.where(np.arange(len(lv)) % 10 == j, np.uint64(0), np.uint64(1 << 63)), hang0) for j in range(10)]  # disjoint tenths
        for rx in list(rxs.values()) + list(rot.values()):
            rx.set_publish(False)
        times = {k: [] for k in list(rxs) + list(rot)}
        parent = []
        for r in range(a.reps):
            for k, rx in rxs.items():
                times[k].append(timed(rx, host, a.steps, a.warmup))
            for k, rx in rot.items():
                times[k].append(timed_rotating(rx, host, a.steps, a.warmup, lv, sets))
            if a.parent_lib:  # one round of the parent's library between ours, in a process of its own
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(a.steps), "--warmup",
                                      str(a.warmup), "--reps", "1"], env={**os.environ, "SDRX_LIB": os.path.abspath(a.parent_lib)},
                                     capture_output=True, text=True, check=True, timeout=300)
                parent += json.loads(out.stdout.strip().splitlines()[-1])
        for k, v in times.items():
            result[f"{name}_{k}"] = summary(v)
            if k != "meter1_squelch0":
                eg = {**rxs, **rot}[k].egress()
                result[f"{name}_{k}"].update(n_open=eg["n_open"], payload_bytes_copied=eg["payload_bytes_copied"])
            if "preroll" in k:
                result[f"{name}_{k}"].update({**rxs, **rot}[k].preroll_count())
        if parent:
            result[f"{name}_parent_lib"] = summary(parent)
        result[f"{name}_device_bytes"] = {"meter1_squelch0": rxs["meter1_squelch0"].stats()["device_bytes"],
                                          "squelch1": rxs["open_100pct"].stats()["device_bytes"],
                                          "preroll1": rxs["preroll_10pct"].stats()["device_bytes"]}
        for rx in list(rxs.values()) + list(rot.values()):
            rx.close()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
