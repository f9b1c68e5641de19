"""The ADC meter (option adc_meter, include/sdrx.h sdrx_adc_meter) as a numpy model, and the frames the device is held to.

`model` is the definition: np.int64 sums of the integer codes and a plain Python run scan.  `device_like` computes the same
record the way k_adc_meter is laid out -- per-thread sums, one element per workgroup, the workgroups' elements merged in
order -- so that the ways such a kernel goes wrong can be written down (FLAWS) and shown to change the record on the crafted
frames below.  The geometry is the kernel's, named here so the crafted frames can be placed on its boundaries.
"""
from __future__ import annotations

import functools

import numpy as np

from sdrreceiver_amd import ingest

CU8, CS8, CS16 = ingest.CU8, ingest.CS8, ingest.CS16
FORMATS = (CU8, CS8, CS16)
NAME = {CU8: "cu8", CS8: "cs8", CS16: "cs16"}

# ---- the kernel's geometry, in complex samples (adcmeter.hip) -------------------------------------------------------------------
LOAD = {CU8: 8, CS8: 8, CS16: 4}  # per 16-byte load
THREAD = 16
WAVE = 64 * THREAD
WG = 4 * WAVE
BINS = 17


def samples_of(codes, fmt) -> np.ndarray:
    """integer codes (interleaved I,Q) -> the samples of format `fmt` that carry them"""
    c = np.asarray(codes, np.int64)
    assert c.min() >= ingest.LOWEST[fmt] and c.max() <= ingest.HIGHEST[fmt]
    return (c + 127).astype(np.uint8) if fmt == CU8 else c.astype(ingest.FORMATS[fmt])


def longest_run(mask) -> int:
    """the longest run of consecutive True: a plain scan over the positions that are set"""
    best = cur = 0
    last = -2
    for k in np.flatnonzero(np.asarray(mask, bool)).tolist():
        cur = cur + 1 if k == last + 1 else 1
        best = max(best, cur)
        last = k
    return best


def runs_of(mask) -> list:
    """[(start, length)] of every run of consecutive True"""
    out = []
    for k in np.flatnonzero(np.asarray(mask, bool)).tolist():
        if out and out[-1][0] + out[-1][1] == k:
            out[-1][1] += 1
        else:
            out.append([k, 1])
    return [tuple(r) for r in out]


def bit_lengths(v) -> np.ndarray:
    """bit_length(|v|) of every code: 0 for 0, 16 for -32768"""
    a = np.abs(np.asarray(v, np.int64))
    return np.where(a > 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1, 0)


def _arm(v, fmt) -> dict:
    lo, hi = v == ingest.LOWEST[fmt], v == ingest.HIGHEST[fmt]
    return {"sum": int(v.sum(dtype=np.int64)), "sum_sq": int((v * v).sum(dtype=np.int64)), "min": int(v.min()), "max": int(v.max()),
            "at_lo": int(lo.sum()), "at_hi": int(hi.sum()), "longest_rail_run": longest_run(lo | hi)}


def model(samples, fmt, frame=0) -> dict:
    """The record of one frame of integer samples (interleaved I,Q) of format `fmt`: the definition."""
    c = ingest.codes(samples, fmt)
    vi, vq = c[0::2], c[1::2]
    bits = np.bincount(bit_lengths(c), minlength=BINS)
    assert bits.size == BINS and int(bits.sum()) == c.size
    return {"frame": int(frame), "n_complex": int(vi.size), "fmt": int(fmt), "measured": 1, "i": _arm(vi, fmt), "q": _arm(vq, fmt),
            "sum_iq": int((vi * vq).sum(dtype=np.int64)), "bits": [int(b) for b in bits]}


def unmeasured(frame) -> dict:
    z = {"sum": 0, "sum_sq": 0, "min": 0, "max": 0, "at_lo": 0, "at_hi": 0, "longest_rail_run": 0}
    return {"frame": int(frame), "n_complex": 0, "fmt": -1, "measured": 0, "i": dict(z), "q": dict(z), "sum_iq": 0, "bits": [0] * BINS}


# ---- the same record the way the kernel is laid out, with the ways it can go wrong ---------------------------------------------
FLAWS = ("sum32", "pad_zero", "pad_rail", "no_wg_merge", "swap_pre_suf", "b_minus_128", "bin15", "iq_unsigned")


def _element(v, rail) -> dict:
    """the associative element of a stretch of one arm: (length, prefix run, suffix run, best)"""
    n = int(rail.size)
    off = np.flatnonzero(~rail)
    pre = n if off.size == 0 else int(off[0])
    suf = n if off.size == 0 else n - 1 - int(off[-1])
    return {"len": n, "pre": pre, "suf": suf, "best": longest_run(rail)}


def _merge(a, b, flaw) -> dict:
    if flaw == "swap_pre_suf":
        return {"len": a["len"] + b["len"], "best": max(a["best"], b["best"], a["pre"] + b["suf"]),
                "pre": a["len"] + b["pre"] if a["pre"] == a["len"] else a["pre"],
                "suf": b["len"] + a["suf"] if b["suf"] == b["len"] else b["suf"]}
    best = max(a["best"], b["best"]) if flaw == "no_wg_merge" else max(a["best"], b["best"], a["suf"] + b["pre"])
    return {"len": a["len"] + b["len"], "best": best, "pre": a["len"] + b["pre"] if a["pre"] == a["len"] else a["pre"],
            "suf": b["len"] + a["suf"] if b["suf"] == b["len"] else b["suf"]}


def device_like(samples, fmt, frame=0, flaw=None) -> dict:
    """`model`'s record computed per thread and per workgroup and merged in order; `flaw`: one of FLAWS, built in."""
    assert flaw is None or flaw in FLAWS
    a, fmt = ingest.as_samples(samples, fmt)
    c = ingest.codes(a, fmt)
    if flaw == "b_minus_128" and fmt == CU8:
        c = a.astype(np.int64) - 128
    n = c.size // 2
    lo_code, hi_code = ingest.LOWEST[fmt], ingest.HIGHEST[fmt]
    if flaw in ("pad_zero", "pad_rail"):  # the threads behind the frame's end count as samples
        pad = (-n) % WG
        c = np.concatenate([c, np.full(2 * pad, 0 if flaw == "pad_zero" else lo_code, np.int64)])
    vi, vq = c[0::2], c[1::2]
    rec = {"frame": int(frame), "n_complex": n, "fmt": int(fmt), "measured": 1}
    for key, v in (("i", vi), ("q", vq)):
        sq = (v * v)[:n] if flaw == "pad_rail" else v * v
        if flaw == "sum32":  # a thread's sum of squares in 32 bits
            per = np.add.reduceat(sq, np.arange(0, v.size, THREAD)) & 0xFFFFFFFF
            sum_sq = int(per.sum(dtype=np.int64))
        else:
            sum_sq = int(sq.sum(dtype=np.int64))
        rail = (v == lo_code) | (v == hi_code)
        if flaw == "pad_zero":
            rail[n:] = False
        e = None
        for w in range(0, v.size, WG):
            el = _element(v[w:w + WG], rail[w:w + WG])
            e = el if e is None else _merge(e, el, flaw)
        lo, hi = v == lo_code, v == hi_code
        real = slice(0, None) if flaw == "pad_zero" else slice(0, n)  # (pad_rail: the rails and runs count, the values do not)
        rec[key] = {"sum": int(v[:n].sum(dtype=np.int64)), "sum_sq": sum_sq, "min": int(v[real].min()), "max": int(v[real].max()),
                    "at_lo": int(lo.sum()), "at_hi": int(hi.sum()), "longest_rail_run": e["best"]}
    if flaw == "iq_unsigned":
        u = a.astype(np.int64) & (0xFFFF if fmt == CS16 else 0xFF)
        rec["sum_iq"] = int((u[0::2] * u[1::2]).sum(dtype=np.int64))
    else:
        rec["sum_iq"] = int((vi[:n] * vq[:n]).sum(dtype=np.int64))
    k = bit_lengths(c if flaw == "pad_zero" else c[:2 * n])
    if flaw == "bin15":
        k = np.minimum(k, 15)
    rec["bits"] = [int(b) for b in np.bincount(k, minlength=BINS)]
    return rec


# ---- the crafted frames ------------------------------------------------------------------------------------------------------
CRAFT_N = 16368  # 3 whole workgroups and 4080 samples: the last workgroup ends one thread short of a wave
SMALL_N = 1296   # one wave and 17 threads


def _background(rng, fmt, n) -> np.ndarray:
    """codes well inside the range, no rail anywhere"""
    span = 100 if fmt != CS16 else 20000
    return rng.integers(-span, span + 1, 2 * n).astype(np.int64)


def boundary_runs(fmt, n=CRAFT_N) -> dict:
    """Where the rail runs of the boundary frame lie, per arm: {name: (start, length)}.  I: one run for every kind of boundary,
    one over a whole workgroup that begins and ends mid-thread, one at sample 0 and one at sample n - 1.  Q: two runs of one
    length, the longest of that arm, where I has none."""
    assert n >= 3 * WG + 2 * THREAD
    L = LOAD[fmt]
    i = {
        "at_0": (0, 3),
        "inside_load": (5 * THREAD + 1, 2),
        "across_loads": (9 * THREAD + L - 1, 2),
        "across_threads": (20 * THREAD - 1, 3),
        "across_waves": (WAVE - 2, 5),
        "across_workgroups": (WG - 3, 5),
        "whole_workgroup": (2 * WG - 103, WG + 103 + 37),
        "at_end": (n - 2, 2),
    }
    q = {"first_longest": (WG + 3 * THREAD - 20, 40), "second_longest": (WG + WAVE + 7 * THREAD - 20, 40), "short": (40, 7)}
    return {"i": i, "q": q}


def boundary_frame(fmt, n=CRAFT_N, seed=5) -> np.ndarray:
    rng = np.random.default_rng(seed + fmt)
    c = _background(rng, fmt, n)
    lo, hi = ingest.LOWEST[fmt], ingest.HIGHEST[fmt]
    for arm, runs in boundary_runs(fmt, n).items():
        for start, length in runs.values():
            k = np.arange(start, start + length)
            c[2 * k + (arm == "q")] = np.where(k % 3 == 0, hi, lo)  # either rail counts
    return samples_of(c, fmt)


def one_lowest(fmt, n, at) -> np.ndarray:
    """one sample whose components are both the lowest code, among zeros"""
    c = np.zeros(2 * n, np.int64)
    c[2 * at] = c[2 * at + 1] = ingest.LOWEST[fmt]
    return samples_of(c, fmt)


@functools.lru_cache(maxsize=None)
def crafted(fmt, n=CRAFT_N) -> dict:
    """name -> samples: every crafted frame of format `fmt` at `n` samples"""
    lo, hi = ingest.LOWEST[fmt], ingest.HIGHEST[fmt]
    alt = np.empty(2 * n, np.int64)
    alt[0::4], alt[1::4], alt[2::4], alt[3::4] = lo, hi, hi, lo  # every arm alternates: mean about 0, power full scale
    out = {
        "all_lowest": samples_of(np.full(2 * n, lo, np.int64), fmt),
        "all_highest": samples_of(np.full(2 * n, hi, np.int64), fmt),
        "alternating": samples_of(alt, fmt),
        "zeros": samples_of(np.zeros(2 * n, np.int64), fmt),
    }
    if n >= 3 * WG + 2 * THREAD:
        out["boundaries"] = boundary_frame(fmt, n)
    if fmt == CU8:
        for b in (0, 127, 128, 255):
            out[f"bytes_{b}"] = np.full(2 * n, b, np.uint8)
    for at in (0, 15, 16, n - 1):
        out[f"lowest_at_{at}"] = one_lowest(fmt, n, at)
    for v in out.values():
        v.setflags(write=False)
    return out


def full_range(fmt, n, seed) -> np.ndarray:
    """full-range random samples of `fmt`, both rails forced in"""
    info = np.iinfo(ingest.FORMATS[fmt])
    rng = np.random.default_rng(seed)
    v = rng.integers(info.min, info.max + 1, 2 * n, dtype=ingest.FORMATS[fmt])
    v[[0, 3, -1]] = info.min
    v[[1, 2, -2]] = info.max
    return v


def from_bytes(b, fmt) -> np.ndarray:
    """dongle bytes as the samples of `fmt` with the same value: CU8 as they are, CS8 b - 127 "to int8", CS16 that times 256
    (bytes <= 254)"""
    b = np.asarray(b, np.uint8)
    if fmt == CU8:
        return b
    assert int(b.max()) <= 254
    v = b.astype(np.int32) - 127
    return v.astype(np.int8) if fmt == CS8 else (v * 256).astype(np.int16)
