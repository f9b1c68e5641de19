#!/usr/bin/env python3
"""tools/ingest_time.py [frames] -- what the integer sample formats cost (sdrx_*_fmt, DESIGN.md "Integer sample formats").

1. The event-timed ingest group (sdrx_get_kernel_times, k_ingest) per 384 000-sample frame of config 1's tree fed CU8, CS8
   and CS16, without and with the exact DC-bias removal: the capture-like stream (offsets +1.3 / -0.7 LSB, the same sample
   values in every format), 16 frames of warm-up so that the estimate sits where it lives.
2. Config 3 through the ABI, pipelined (submit(f+1); wait() -> f), fed cf32 and fed CS16 without DC removal: ms per frame."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from sdrreceiver_amd import ingest, synth, topology as tp  # noqa: E402
from sdrreceiver_amd.receiver import Receiver  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 24
topo = tp.config1()
cap = synth.capture_like_u8(8, topo.frame, topo.fs)
cap = [np.minimum(cap[2 * topo.frame * f: 2 * topo.frame * (f + 1)], 254) for f in range(8)]  # (byte 255 has no signed image)
as_fmt = {ingest.CU8: lambda b: b, ingest.CS8: lambda b: (b.astype(np.int16) - 127).astype(np.int8),
          ingest.CS16: lambda b: ((b.astype(np.int32) - 127) * 256).astype(np.int16)}
out = {"ingest_ms_per_frame": {}, "config3_pipelined_ms_per_frame": {}}
for name, fmt in ingest.NAMES.items():
    feed = [as_fmt[fmt](b) for b in cap]
    for dc in (False, True):
        rx = Receiver.from_topology(topo)
        rx.set_publish(False)
        for k in range(16):
            rx.process_fmt(feed[k % 8], correct_dc=dc)
        rx.enable_kernel_timing(True)
        for k in range(frames):
            rx.process_fmt(feed[k % 8], correct_dc=dc)
        t = rx.kernel_times().get("k_ingest")  # (dongle bytes without DC removal go to level 0 as they lie: no ingest launch)
        out["ingest_ms_per_frame"][f"{name}{' + dc' if dc else ''}"] = round(t["ms"] / frames, 4) if t else None
        rx.close()

topo = tp.config3(1024)
lcg = synth.Lcg(1)
f32 = [synth.lcg_frame(topo.frame, lcg) for _ in range(4)]
s16 = [(x * 256).astype(np.int16) for x in f32]  # the same sample values
for name, submit, feed in (("cf32", "submit", f32), ("cs16", "submit_fmt", s16)):
    rx = Receiver.from_topology(topo)
    rx.set_publish(False)
    go = getattr(rx, submit)
    best = []
    for rep in range(3):
        t0 = time.perf_counter()
        go(feed[0])
        for k in range(1, frames):
            go(feed[k % 4])
            rx.wait()
        rx.wait()
        best.append((time.perf_counter() - t0) / frames * 1e3)
    out["config3_pipelined_ms_per_frame"][name] = [round(b, 4) for b in best]
    rx.close()
print(json.dumps(out))
