"""Crafted schedules for option "agc" (test infrastructure; no GPU): frames, settings and gains designed so that the gain step
meets its thresholds, its clamp and more than one block -- what the closed loop of tests/agc_ref.py, whose windows lie far
from every meter, never shows the device.  tests/test_agc_crafted_model.py asserts every condition named here on the model,
tests/test_gpu_agc_crafted.py holds the device to the same records bit for bit.

A schedule is ``sched[f]`` = the calls made before frame f, in order: ``("gain", ids, gains)`` is one sdrx_set_gains call,
``("agc", ids, cfgs)`` one sdrx_set_agc call (which restarts the named leaves' quiet_run).  :func:`run` plays it on
agc_ref.AgcTree -- live_ref.ModelTree, pinned to the oracle by tests/test_live_model.py, with sdrreceiver_amd.agc.step behind
every frame -- and that run is the expectation: nothing here predicts a meter without the model confirming it.

* :func:`boundary` -- on ``lat-late-deep`` and ``rnd-24``, with ``up = down = 1`` so that the step takes every decision and the
  gain never moves: a USB leaf's pre-gain stream does not depend on its gain, so ONE plain model run at unit gain
  (:func:`usb_streams`) gives every leaf's stream of every frame, a seeded search over gains (:func:`_search`) finds the gain at
  which a frame's ``sum_sq`` is a multiple of ``n_values``, and the thresholds are then built from the meter of the very frame
  that follows.  Frames 0-2 are all-zero input (``s == 0``), 3-8 carry one threshold case per leaf and frame -- ``s == T n``,
  ``T n + r`` and ``T n - r`` for T = hi_ms, lo_ms, silent_ms, and ``silent_ms == lo_ms`` -- and, on the leaves with more than
  1024 outputs, exactly one wrapped sample past the first meter record with ``hi_ms = 2^30``; 9-16 run
  cold, cold, silent, cold, in-window, cold, hot, cold under ONE setting per leaf with ``hold_frames`` 0, 1 and 2^32 - 1, steered
  by sdrx_set_gains alone (which leaves quiet_run alone).
* :func:`clamp` -- the one fp32 multiply and the clamp: seven all-zero frames on which every leaf is cold (``silent_ms = 0,
  lo_ms = 1``) and raises by its own ``up``, then seven loud ones on which ``hi_ms = 1`` makes it hot and it lowers by its own
  ``down``; steps with full mantissas, limits out of reach (seven multiplies in a row) and within it, a product that overflows
  to +inf, host-set gains outside the limits.
* :func:`wide` -- one /4 inner node on 1.536 MS/s with 520 USB leaves (d = 3 and d = 5 alternately: 480 and 120 values per
  frame of 15 360): three blocks of k_agc_step, the last partly filled, nine of k_agc_set.  Settings and gains depend on the
  slot; the sdrx_set_agc calls name 1, 63, 64, 65, 256, 257 and all leaves in shuffled order.
* :func:`mutants` -- wrong rules, each a small variant of agc.step (:func:`rule`); :func:`exposure` counts the scheduled
  (leaf, frame) pairs on which a mutant's record differs from the rule's.

Not reachable, hence not here: ``quiet_run`` saturating at 2^32 - 1 (no call can set the word; agc.step's own saturation is
asserted in tests/test_agc_model.py), and a NaN product (sdrx_set_gains refuses a gain that is not finite, so
``fl(g * up)`` is finite or an infinity)."""
from __future__ import annotations

import functools

import numpy as np

import agc_ref as ar
import lattice
import live_ref as lr
import retune_ref as rr
from sdrreceiver_amd import agc
from sdrreceiver_amd.topology import Topology, VfoDesc

FULL = agc.FULL_SCALE_MS
HOLD_MAX = (1 << 32) - 1
FLT_MAX = float(np.finfo(np.float32).max)
TREES = ("lat-late-deep", "rnd-24")
THRESHOLDS = ("hi_ms", "lo_ms", "silent_ms")
TILE = 1024  # values per meter record


def f32(x) -> float:
    return float(np.float32(x))


# ---- frames ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loud(name, n):
    """(topo, n loud frames) of one of agc_ref's trees, with as many frames as the schedule needs"""
    kind, key = name.split("-", 1)
    if kind == "rnd":
        topo = lr.topology_of(int(key))
        return topo, tuple(lr.frames_of(topo, int(key), n))
    return lattice.trees()[key], lattice.frames(key, n)


def _frames(topo, n_zero, loud):
    z = np.zeros(2 * topo.frame, np.float32)
    z.setflags(write=False)
    return (z,) * n_zero + tuple(loud)


def usb_leaves(topo) -> list:
    return [i for i in topo.leaves_in_publish_order() if topo.vfos[i].demod_usb]


def slot_order(topo) -> list:
    """The USB leaves in node order: the device's slots (sdrx_finalize's AGC table)"""
    return sorted(usb_leaves(topo))


def usb_streams(topo, frames) -> dict:
    """u[leaf][f]: the float32 stream in front of the gain (``pre = fl(u g) * 32768``), from one model run at unit gain"""
    model = lr.ModelTree(topo)
    usb = usb_leaves(topo)
    for i in usb:
        model.set_gain(i, 1.0)
    out = {i: [] for i in usb}
    for iq in frames:
        model.process(iq)
        for i in usb:
            out[i].append((model.nodes[i].pre / 32768.0).astype(np.float32))
    return out


def meter_at(u, g) -> tuple:
    """(sum_sq, n_values, clipped) of the stream `u` at gain `g`: retune_ref.Node.payload's last two lines and the meter"""
    pre = (u * np.float32(g)).astype(np.float64) * 32768.0
    v = rr.to_short(pre).astype(np.int64)
    p = pre.astype(np.float32)
    return int(np.sum(v * v)), int(u.size), int(np.count_nonzero(~((p > -32769.0) & (p < 32768.0))))


def _head(payload, pre) -> dict:
    """The meter without the payload's last 1024-value tile (the last record of a leaf with several)"""
    n = payload.size
    cut = ((n - 1) // TILE) * TILE if n else 0
    v = payload[:cut].astype(np.int64)
    p = np.asarray(pre[:cut], np.float32)
    return {"sum_sq": int(np.sum(v * v)), "n_values": n, "clipped": int(np.count_nonzero(~((p > -32769.0) & (p < 32768.0))))}


# ---- the model run ----------------------------------------------------------------------------------------------------------------
def _apply(model, calls):
    for kind, ids, vals in calls:
        for i, v in zip(ids, vals):
            model.apply([(kind, i, v)])


def run(topo, frames, sched) -> tuple:
    """want[f] = agc_ref.AgcTree.process of frame f under `sched` (without the streams), plus per USB leaf ``before`` =
    (settings, quiet_run) in front of the frame, ``head`` = :func:`_head` and ``wrapped`` = the indices of the wrapped samples
    (at most a few are kept)."""
    model = ar.AgcTree(topo)
    want = []
    for f, iq in enumerate(frames):
        _apply(model, sched[f])
        before = {i: (model.cfg[i], model.quiet[i]) for i in model.usb}
        w = model.process(iq)
        w["streams"] = w["published"] = None
        w["before"] = before
        w["head"], w["wrapped"] = {}, {}
        for i in model.usb:
            pre = model.nodes[i].pre.astype(np.float32)
            w["head"][i] = _head(w["payload"][i], pre)
            w["wrapped"][i] = tuple(np.nonzero(~((pre > -32769.0) & (pre < 32768.0)))[0][:4].tolist())
        want.append(w)
    return tuple(want)


def cases(ref) -> list:
    """Every (USB leaf, frame) of a schedule with an observation, as a dict: tree, leaf, frame, cfg, q (quiet_run in front of
    the frame), g (gain_used), meter, head, wrapped, rec (the rule's record), fresh (an sdrx_set_agc named the leaf before
    this frame)."""
    out = []
    for f, w in enumerate(ref["want"]):
        named = {i for kind, ids, _ in ref["sched"][f] if kind == "agc" for i in ids}
        for i, (cfg, q) in w["before"].items():
            if cfg.hi_ms == 0 or w["meters"][i]["n_values"] == 0:
                continue
            out.append(dict(tree=ref["name"], leaf=i, frame=f, cfg=cfg, q=q, g=w["agc"][i]["gain_used"], meter=w["meters"][i],
                            head=w["head"][i], wrapped=w["wrapped"][i], rec=w["agc"][i], fresh=i in named))
    return out


def kind_of(c) -> str:
    """hot / silent / cold / window of one case, by the rule"""
    s, n, cfg = c["meter"]["sum_sq"], c["meter"]["n_values"], c["cfg"]
    if c["meter"]["clipped"] > 0 or s > cfg.hi_ms * n:
        return "hot"
    if s < cfg.silent_ms * n:
        return "silent"
    return "cold" if s < cfg.lo_ms * n else "window"


def relation(c, name) -> str | None:
    """"eq", "+r" or "-r" when the case's sum_sq lies within one unit of the threshold `name` (s == T n, T n + r, T n - r with
    0 < r < n; s > 0, nothing wrapped), else None"""
    s, n, T = c["meter"]["sum_sq"], c["meter"]["n_values"], getattr(c["cfg"], name)
    if s <= 0 or c["meter"]["clipped"]:
        return None
    d = s - T * n
    return "eq" if d == 0 else "+r" if 0 < d < n else "-r" if -n < d < 0 else None


# ---- a. the boundary schedule -----------------------------------------------------------------------------------------------------
B_ZERO, B_CASE, B_HOLD = 3, 6, 8          # frames 0-2, 3-8, 9-16
B_CLIP = (B_ZERO + 4, B_ZERO + 5)         # the two case frames in which a leaf with several records wraps once / just does not
HOLD_PATTERN = ("cold", "cold", "silent", "cold", "window", "cold", "hot", "cold")
HOLD_QUIET = (1, 2, 2, 3, 0, 1, 0, 1)
CASE_KINDS = tuple((t, r) for t in THRESHOLDS for r in ("eq", "+r", "-r")) + (("both", "eq"), ("both", "-r"))
_FROZEN = dict(up=1.0, down=1.0, gain_min=1e-30, gain_max=1e30)  # (every gain of the schedule lies inside: the clamp is idle)


def _search(u, rng, want_eq):
    """A float32 gain at which `u` wraps nowhere and has s > 0, s // n >= 1 and (s % n == 0) == want_eq, with its (s, n), or None:
    a seeded loop over the model's own arithmetic"""
    pk = float(np.abs(u).max()) * 32768.0
    if not pk > 0.0:
        return None
    tries = min(3 * u.size + 200, 8000) if want_eq else 50
    for _ in range(tries):
        g = f32(32767.0 / pk * rng.uniform(0.35, 0.95))
        s, n, clipped = meter_at(u, g)
        if clipped == 0 and s >= n and (s % n == 0) == want_eq:
            return g, s, n
    return None


def _case_cfg(which, rel, s, n, hold, top):
    """The setting that puts threshold `which` at distance `rel` of s; `top`: hi_ms = 2^30 where it is free"""
    T = s // n + (1 if rel == "-r" else 0)
    if which == "hi_ms":
        lo, hi, silent = T // 2, T, T // 4
    elif which == "lo_ms":
        lo, hi, silent = T, FULL if top else min(FULL, 4 * T), T // 2
    elif which == "silent_ms":
        lo, hi, silent = min(FULL, 2 * T + 1), FULL if top else min(FULL, 8 * T + 8), T
    else:  # silent_ms == lo_ms
        lo, hi, silent = T, FULL if top else min(FULL, 4 * T), T
    return agc.Cfg(lo, hi, silent, hold, **_FROZEN)


ZERO_CFGS = (agc.Cfg(0, 1, 0, 0, **_FROZEN),   # s == 0 is in the window
             agc.Cfg(1, 1, 0, 1, **_FROZEN),   # cold
             agc.Cfg(1, 1, 1, 0, **_FROZEN))   # silent


def _gain_for_ms(u, ms):
    m = float(np.mean((u.astype(np.float64) * 32768.0) ** 2))
    return f32(np.sqrt(ms / m)) if m > 0 else None


@functools.lru_cache(maxsize=None)
def boundary(name) -> dict:
    """name, topo, frames, sched, want of the frozen-gain schedule on one of :data:`TREES`.  Shared; read-only."""
    topo, loud = _loud(name, B_CASE + B_HOLD)
    frames = _frames(topo, B_ZERO, loud)
    usb = usb_leaves(topo)
    u = usb_streams(topo, frames)
    rng = np.random.default_rng(81000 + TREES.index(name))
    sched = [[] for _ in frames]

    def put(f, gains, cfgs):
        if gains:
            sched[f].append(("gain", list(gains), [gains[i] for i in gains]))
        if cfgs:
            sched[f].append(("agc", list(cfgs), [cfgs[i] for i in cfgs]))

    # frames 0 - 2: all-zero input.  Frame 1 follows without a call: the cold leaves count on, the others stay.
    put(0, {}, {i: ZERO_CFGS[k % 3] for k, i in enumerate(usb)})
    put(2, {}, {i: ZERO_CFGS[(k + 1) % 3] for k, i in enumerate(usb)})
    # frames 3 - 8: one threshold case per leaf and frame
    for f in range(B_ZERO, B_ZERO + B_CASE):
        gains, cfgs = {}, {}
        for k, i in enumerate(usb):
            x = u[i][f]
            if x.size > TILE and f in B_CLIP:
                a = np.sort(np.abs(x.astype(np.float64)))[-2:] * 32768.0
                clip_here = int(np.argmax(np.abs(x))) >= TILE and a[1] > a[0] > 0
                other = B_CLIP[1 - B_CLIP.index(f)]
                clip_other = int(np.argmax(np.abs(u[i][other]))) >= TILE
                if clip_here and (f == B_CLIP[0] or not clip_other):
                    g = f32(2.0 * 32768.0 / (a[0] + a[1]))  # between the two largest: exactly one sample wraps
                    if meter_at(x, g)[2] == 1:
                        gains[i], cfgs[i] = g, agc.Cfg(1, FULL, 0, k % 2, **_FROZEN)
                        continue
                elif clip_other and a[1] > 0:
                    g = f32(32767.0 / a[1])               # one notch lower: the largest sample just does not wrap
                    if meter_at(x, g)[2] == 0:
                        gains[i], cfgs[i] = g, agc.Cfg(1, FULL, 0, k % 2, **_FROZEN)
                        continue
            which, rel = CASE_KINDS[(k + 5 * f) % len(CASE_KINDS)]
            found = _search(x, rng, rel == "eq")
            if found is None and rel == "eq":
                rel = "+r"
                found = _search(x, rng, False)
            if found is None:
                continue  # (a frame of zeros: the leaf keeps what it has)
            g, s, n = found
            gains[i] = g
            cfgs[i] = _case_cfg(which, rel, s, n, hold=(k + f) % 2, top=(k + f) % 3 == 0)
        put(f, gains, cfgs)
    # frames 9 - 16: one setting per leaf, the classes steered by the gain alone
    f0 = B_ZERO + B_CASE
    plan = {}
    for k, i in enumerate(usb):
        xs = u[i][f0:f0 + B_HOLD]
        pk = [float(np.abs(x).max()) * 32768.0 for x in xs]
        if not all(p > 0 for p in pk):
            continue
        w = HOLD_PATTERN.index("window")
        g_win = f32(0.9 * 32767.0 / pk[w])
        s, n, _ = meter_at(xs[w], g_win)
        lo = (s // n) // 4
        if lo < 64:
            continue
        cfg = agc.Cfg(lo, FULL, lo // 16, (0, 1, HOLD_MAX)[k % 3], **_FROZEN)
        gs = []
        for j, cls in enumerate(HOLD_PATTERN):
            g = {"window": g_win, "hot": f32(2.0 * 32768.0 / pk[j]), "cold": _gain_for_ms(xs[j], lo / 4.0),
                 "silent": _gain_for_ms(xs[j], lo / 64.0)}[cls]
            gs.append(g)
        got = [kind_of(dict(meter=dict(zip(("sum_sq", "n_values", "clipped"), meter_at(x, g))), cfg=cfg)) for x, g in zip(xs, gs)]
        if tuple(got) == HOLD_PATTERN:
            plan[i] = (cfg, gs)
    off = agc.Cfg(0, 0, 0, 0, 1.0, 1.0, 1.0, 1.0)
    put(f0, {i: plan[i][1][0] for i in plan}, {i: plan[i][0] if i in plan else off for i in usb})
    for j in range(1, B_HOLD):
        put(f0 + j, {i: plan[i][1][j] for i in plan}, {})
    ref = dict(name=name, topo=topo, frames=frames, sched=tuple(tuple(s) for s in sched), hold_leaves=tuple(plan))
    ref["want"] = run(topo, frames, sched)
    return ref


# ---- b. the multiply-and-clamp schedule ------------------------------------------------------------------------------------------
C_ZERO = C_LOUD = 7
COLD_ALWAYS = dict(lo_ms=1, hi_ms=1, silent_ms=0, hold_frames=0)  # s == 0 is cold; a payload with s > n is hot


@functools.lru_cache(maxsize=None)
def clamp(name) -> dict:
    """name, topo, frames, sched, want, roles ({leaf: (role on the zero frames, role on the loud ones)}): every USB leaf raises
    by its own `up` over seven all-zero frames and lowers by its own `down` over seven loud ones.  `up` and `down` are doubles
    with full mantissas (the library and the rule round them to float32 once).  The "free" leaves -- every leaf with several
    meter records among them -- have their limits out of reach: their gain is one float32 multiply further in each of the
    seven frames of a half.  The "compound" ones reach a limit at the fourth or fifth step and stay on it."""
    topo, loud = _loud(name, C_LOUD)
    frames = _frames(topo, C_ZERO, loud)
    usb = usb_leaves(topo)
    u = usb_streams(topo, frames)
    rng = np.random.default_rng(82000 + TREES.index(name))
    gains0, cfgs0, gains1, cfgs1, roles = {}, {}, {}, {}, {}
    for k, i in enumerate(usb):
        up, down = float(rng.uniform(1.0, 3.0)), 1.0 - float(rng.uniform(0.0, 0.8))  # [1, 3) and (0.2, 1]
        g0 = f32(rng.uniform(0.01, 2.0))
        big = topo.vfos[i].n_out > TILE  # several meter records: such a leaf compounds freely in both halves
        role = "free" if big else ("overflow", "above_max_cold", "outside_window", "pinned", "compound", "free")[k % 6]
        if role == "overflow":      # three raises, then fl(g up) = +inf, clamped to FLT_MAX
            g0, c = f32(FLT_MAX / up ** 3.5), agc.Cfg(up=up, down=down, gain_min=1e-3, gain_max=FLT_MAX, **COLD_ALWAYS)
        elif role == "above_max_cold":  # a host-set gain above gain_max: the raise moves it DOWN
            g0, c = f32(rng.uniform(40.0, 60.0)), agc.Cfg(up=up, down=down, gain_min=0.1, gain_max=f32(rng.uniform(2.0, 4.0)), **COLD_ALWAYS)
        elif role == "outside_window":  # in the window (lo_ms 0): a gain outside the limits stays, above and below
            g0 = f32(rng.uniform(40.0, 60.0)) if k % 12 < 6 else f32(rng.uniform(1e-4, 2e-4))
            c = agc.Cfg(0, 1, 0, 0, up, down, 0.01, 4.0)
        elif role == "pinned":          # gain_min == gain_max
            lim = f32(rng.uniform(0.5, 1.5))
            c = agc.Cfg(up=up, down=down, gain_min=lim, gain_max=lim, **COLD_ALWAYS)
        elif role == "compound":        # a ceiling within reach of the fifth raise
            c = agc.Cfg(up=up, down=down, gain_min=1e-6, gain_max=f32(g0 * up ** 4.3), **COLD_ALWAYS)
        else:                           # free: seven raises, one float32 multiply each, the limits out of reach (g0 3^7 < 1e4)
            c = agc.Cfg(up=up, down=down, gain_min=1e-6, gain_max=1e30, **COLD_ALWAYS)
        gains0[i], cfgs0[i] = g0, c
        # the loud half: gains from the leaf's own level at the first loud frame (an RMS near 3000 LSB)
        g_ref = _gain_for_ms(u[i][C_ZERO], 9.0e6) or 1.0
        role1 = "free" if big else ("below_min_hot", "pinned", "compound", "free")[k % 4]
        if role1 == "below_min_hot":    # a host-set gain below gain_min: the lowering moves it UP
            g1, c1 = g_ref, agc.Cfg(up=up, down=down, gain_min=f32(3.0 * g_ref), gain_max=f32(10.0 * g_ref), **COLD_ALWAYS)
        elif role1 == "pinned":
            g1, c1 = g_ref, agc.Cfg(up=up, down=down, gain_min=f32(1.7 * g_ref), gain_max=f32(1.7 * g_ref), **COLD_ALWAYS)
        elif role1 == "compound":       # a floor within reach of the fourth lowering
            g1 = f32(g_ref * rng.uniform(1.0, 8.0))
            c1 = agc.Cfg(up=up, down=down, gain_min=f32(g1 * down ** 3.4), gain_max=f32(1e6 * g_ref), **COLD_ALWAYS)
        else:                           # free: seven lowerings with the floor out of reach.  It starts 30 times too loud (hot by
            g1 = f32(30.0 * g_ref)      # `clipped` at first), so that after six steps of 0.2 the RMS is still several LSB: hot
            c1 = agc.Cfg(up=up, down=down, gain_min=f32(1e-9 * g_ref), gain_max=f32(1e6 * g_ref), **COLD_ALWAYS)
        gains1[i], cfgs1[i] = g1, c1
        roles[i] = (role, role1)
    sched = [[] for _ in frames]
    sched[0] = [("gain", list(gains0), list(gains0.values())), ("agc", list(cfgs0), list(cfgs0.values()))]
    sched[C_ZERO] = [("gain", list(gains1), list(gains1.values())), ("agc", list(cfgs1), list(cfgs1.values()))]
    ref = dict(name=name, topo=topo, frames=frames, sched=tuple(tuple(s) for s in sched), roles=roles)
    ref["want"] = run(topo, frames, sched)
    return ref


# ---- c. the wide tree -------------------------------------------------------------------------------------------------------------
W_LEAVES = 520                       # three blocks of k_agc_step's 256 threads, the last with 8; nine of k_agc_set's 64, the last with 8
W_FRAME, W_FS = 15360, 1536000
W_SIZES = (1, 63, 64, 65, 256, 257, W_LEAVES)
W_TARGET = 2000 * 2000


@functools.lru_cache(maxsize=None)
def wide_tree() -> Topology:
    t = Topology(fs=W_FS, frame=W_FRAME, name="agc-wide")
    t.vfos.append(VfoDesc(parent=-1, fs=W_FS, decimate_count=2, mixer_freq=12345.0, demod_usb=False, cstyle=1, samples_per_buffer=W_FRAME))
    fs, n = W_FS >> 2, W_FRAME >> 2
    for k in range(W_LEAVES):
        mixer = float(int(round((k + 0.5 - W_LEAVES / 2) * 0.6 * fs / W_LEAVES)) + 37)
        t.vfos.append(VfoDesc(topic=f"W{k:04d}", parent=0, fs=fs, decimate_count=3 if k % 2 == 0 else 5, mixer_freq=mixer,
                              gain=0.01, cstyle=1, samples_per_buffer=n))
    return t


def wide_cfg(k: int, version: int = 0) -> agc.Cfg:
    """The setting of slot k: no field repeats at k + 1 or at k +- 256.  `version` > 0: the provisional settings of the
    earlier sdrx_set_agc calls -- cold on an all-zero frame, never raising."""
    up, down = 1.0 + ((k * 37) % 509) / 512.0, 1.0 - ((k * 53) % 487) / 1024.0
    gmin, gmax = 1e-4 * (1.0 + k / 1000.0), 10.0 * (1.0 + k / 1000.0)
    if version:
        return agc.Cfg(1 + k, 1 + k + version, 0, HOLD_MAX - k - 1000 * version, up, down, gmin, gmax)
    lo = W_TARGET // 3 + 7 * k
    return agc.Cfg(lo, 9 * lo + k, (lo if k % 5 == 4 else 3 + k), k % 3, up, down, gmin, gmax)


@functools.lru_cache(maxsize=None)
def wide() -> dict:
    """name, topo, frames, sched, want, calls.  Frames 0, 1, 2 and 6 are all-zero input, 3, 4 and 5 loud: four frames follow
    the last call.  Before frame 1:
    provisional settings for shuffled lists of 1, 63 and 64 leaves; before frame 2: for 65 and 256 (a leaf named before frame 1
    alone has counted two cold frames after it, one named again has counted one); before frame 3: 257, then all 520 with
    :func:`wide_cfg` and slot-dependent gains -- every fourth slot 40 times the gain that puts it on the target (hot), every
    fourth a tenth of it (cold), and so on."""
    topo = wide_tree()
    loud = lr.frames_of(topo, 91, 3)
    z = np.zeros(2 * topo.frame, np.float32)
    frames = (z, z, z, loud[0], loud[1], loud[2], z)
    slots = slot_order(topo)
    u = usb_streams(topo, frames)
    rng = np.random.default_rng(83000)
    lists = [[slots[int(j)] for j in rng.permutation(W_LEAVES)[:n]] for n in W_SIZES]
    slot_of = {i: k for k, i in enumerate(slots)}
    sched = [[] for _ in frames]
    for f, which in ((1, (0, 1, 2)), (2, (3, 4)), (3, (5,))):
        for v in which:
            sched[f].append(("agc", lists[v], [wide_cfg(slot_of[i], version=v + 1) for i in lists[v]]))
    gains = []
    for i in lists[6]:
        k = slot_of[i]
        g_in = _gain_for_ms(u[i][3], float(W_TARGET)) or 1.0
        gains.append(f32(g_in * (40.0, 0.1, 1.0, 0.003)[k % 4] * (1.0 + k / 4096.0)))
    sched[3].append(("gain", lists[6], gains))
    sched[3].append(("agc", lists[6], [wide_cfg(slot_of[i]) for i in lists[6]]))
    ref = dict(name="wide", topo=topo, frames=frames, sched=tuple(tuple(s) for s in sched), slots=tuple(slots))
    ref["want"] = run(topo, frames, sched)
    return ref


def settings_after(ref) -> list:
    """expect[f][c] = {leaf: (Cfg, named)} after call c of sched[f] -- the settings of EVERY USB leaf as sdrx_get_agc must read
    them back (all zero before the first call that names the leaf)"""
    cur = {i: agc.Cfg(0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0) for i in usb_leaves(ref["topo"])}
    out = []
    for calls in ref["sched"]:
        row = []
        for kind, ids, vals in calls:
            if kind == "agc":
                cur.update(zip(ids, vals))
            row.append(dict(cur))
        out.append(row)
    return out


# ---- d. mutants -------------------------------------------------------------------------------------------------------------------
def rule(c, flaw=None) -> tuple:
    """(gain_next bits, quiet_run, action) of one case by agc.step's rule, restated so that `flaw` can bend ONE thing"""
    cfg, q, g = c["cfg"], c["q"], np.float32(c["g"])
    m = c["meter"]
    s, n, clipped = m["sum_sq"], m["n_values"], m["clipped"]
    if flaw == "sum_without_last_tile":
        s = c["head"]["sum_sq"]
    if flaw == "clipped_without_last_tile":
        clipped = c["head"]["clipped"]
    if flaw == "clipped_ignored":
        clipped = 0
    prod = (lambda t: (t * n) & 0xFFFFFFFF) if flaw == "products_mod_2_32" else (lambda t: t * n)
    hot = clipped > 0 or (s >= prod(cfg.hi_ms) if flaw == "hi_ge" else s > prod(cfg.hi_ms))
    below_silent = s <= prod(cfg.silent_ms) if flaw == "silent_le" else s < prod(cfg.silent_ms)
    below_lo = s <= prod(cfg.lo_ms) if flaw == "lo_le" else s < prod(cfg.lo_ms)
    if flaw == "silent_after_cold":
        cold = not hot and below_lo
        silent = not hot and not cold and below_silent
    else:
        silent = not hot and below_silent
        cold = not hot and not silent and below_lo

    def clamp_(x):
        if flaw == "clamp_max_of_min":
            return np.float32(np.fmax(np.fmin(np.float32(x), np.float32(cfg.gain_max)), np.float32(cfg.gain_min)))
        return agc.clamp(x, cfg)

    def mul(step):
        with np.errstate(over="ignore"):
            if flaw == "double_rounded_multiply":
                return np.float32(np.float64(g) * np.float64(step))
            return g * np.float32(step)

    g2, action = g, 0
    if hot:
        g2, action = clamp_(mul(cfg.down)), -1
        if flaw != "quiet_kept_by_hot":
            q = 0
    elif silent:
        pass
    elif cold:
        q = min(q + 1, agc.QUIET_MAX)
        if q >= cfg.hold_frames if flaw == "hold_ge" else q > cfg.hold_frames:
            g2, action = clamp_(mul(cfg.up)), 1
    elif flaw != "quiet_kept_in_window":
        q = 0
    if flaw == "clamp_without_action" and action == 0:
        g2 = clamp_(g)
    return int(np.float32(g2).view(np.uint32)), int(q), int(action)


def mutants() -> tuple:
    return ("hi_ge", "lo_le", "silent_le", "products_mod_2_32", "clipped_ignored", "silent_after_cold", "quiet_kept_by_hot",
            "quiet_kept_in_window", "hold_ge", "clamp_max_of_min", "clamp_without_action", "double_rounded_multiply",
            "sum_without_last_tile", "clipped_without_last_tile")


# fminf(fmaxf(x, lo), hi) and fmaxf(fminf(x, hi), lo) differ only for a NaN x (or lo > hi, which sdrx_set_agc refuses), and no
# call can make fl(g * step) a NaN: sdrx_set_gains refuses a gain that is not finite, the steps are finite and positive.  The
# mutant stays in the list -- tests/test_agc_crafted_model.py shows where it WOULD differ -- but no schedule can expose it.
UNREACHABLE = ("clamp_max_of_min",)


@functools.lru_cache(maxsize=None)
def all_cases() -> tuple:
    out = []
    for name in TREES:
        out += cases(boundary(name)) + cases(clamp(name))
    return tuple(out + cases(wide()))


def exposure(flaw) -> int:
    """The scheduled (leaf, frame) pairs whose record under `flaw` differs from the rule's"""
    return sum(rule(c, flaw) != rule(c) for c in all_cases())
