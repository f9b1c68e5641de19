"""The integer sample formats of the ``*_fmt`` calls (include/sdrx.h, SDRX_FMT_*) and their one host definition.

Every format maps to the reference's units, "dongle LSB, |x| <= 128" -- the units the shipped INI gains and every squelch,
AGC and watch threshold live in, and the bound the device's DC-bias removal is proved bit-exact for.  The scale is fixed:

    constant   memory                    sample value x (float32, exact)   range
    CU8 = 0    uint8 I,Q                 b - 127                           [-127, 128]
    CS8 = 1    int8 I,Q                  float(v)                          [-128, 127]
    CS16 = 2   native-endian int16 I,Q   float(v) * 2**-8                  [-128, 128)

Two formats of REAL samples, taken only by a receiver whose front stage has ``front_real`` (sdrreceiver_amd.front; include/sdrx.h
"Front stage"), whose first half-band turns them into I/Q on the device:

    RS16 = 3   native-endian int16       float(v) * 2**-8                  [-128, 128)
    RU12 = 4   uint16, 12-bit offset     float((v & 4095) - 2048) * 2**-4  [-128, 128)

An array's dtype never stands for a real format: int16 is CS16 to :func:`infer_format` and uint16 nothing, so `fmt` must be told.
"""
from __future__ import annotations

import numpy as np

CU8, CS8, CS16 = 0, 1, 2  # SDRX_FMT_CU8, SDRX_FMT_CS8, SDRX_FMT_CS16
RS16, RU12 = 3, 4  # SDRX_FMT_RS16, SDRX_FMT_RU12: real samples
FORMATS = {CU8: np.dtype(np.uint8), CS8: np.dtype(np.int8), CS16: np.dtype(np.int16)}
REAL_FORMATS = {RS16: np.dtype(np.int16), RU12: np.dtype(np.uint16)}
NAMES = {"cu8": CU8, "cs8": CS8, "cs16": CS16, "rs16": RS16, "ru12": RU12}


def is_real(fmt) -> bool:
    return fmt in REAL_FORMATS


def infer_format(a) -> int:
    """The format an array's dtype stands for (uint8 / int8 / int16); TypeError for any other."""
    dt = np.asarray(a).dtype
    for fmt, want in FORMATS.items():
        if dt == want:
            return fmt
    raise TypeError(f"no sample format for dtype {dt}: uint8 (CU8), int8 (CS8) or int16 (CS16)")


def as_samples(a, fmt=None) -> tuple[np.ndarray, int]:
    """`a` as the flat contiguous array of format `fmt` (None: the one its dtype stands for), and that format."""
    if fmt is None:
        fmt = infer_format(a)
    if fmt not in FORMATS and fmt not in REAL_FORMATS:
        raise ValueError(f"fmt {fmt!r}: CU8 (0), CS8 (1), CS16 (2), or the real RS16 (3) or RU12 (4)")
    a = np.asarray(a)
    if fmt in REAL_FORMATS and a.dtype != REAL_FORMATS[fmt]:  # (a value problem: the real formats are named, never inferred)
        raise ValueError(f"the real format {fmt} takes {REAL_FORMATS[fmt]} samples, not {a.dtype}")
    if fmt in FORMATS and a.dtype != FORMATS[fmt]:
        raise TypeError(f"format {fmt} takes {FORMATS[fmt]}, not {a.dtype}")
    return np.ascontiguousarray(a).reshape(-1), int(fmt)


def to_float(a, fmt=None) -> np.ndarray:
    """The float32 samples the library computes from the integer samples `a`: the table above, exactly."""
    a, fmt = as_samples(a, fmt)
    if fmt == CU8:
        return (a.astype(np.int32) - 127).astype(np.float32)
    if fmt == CS8:
        return a.astype(np.float32)
    if fmt == RU12:
        return ((a.astype(np.int32) & 4095) - 2048).astype(np.float32) * np.float32(2.0 ** -4)
    return a.astype(np.float32) * np.float32(2.0 ** -8)


# ---- ADC meter (option ``adc_meter``; include/sdrx.h sdrx_adc_meter): the record, and the figures a front-end loop wants --------
# The integer code v of a component: CU8 b - 127, CS8 the int8, CS16 the int16 itself.  LOWEST / HIGHEST: the rails per format.
# A real frame is recorded as the same memory read as pairs -- even samples in arm I, odd samples in arm Q --: RS16 the int16,
# RU12 (v & 4095) - 2048.
LOWEST = {CU8: -127, CS8: -128, CS16: -32768}
HIGHEST = {CU8: 128, CS8: 127, CS16: 32767}
REAL_LOWEST = {RS16: -32768, RU12: -2048}
REAL_HIGHEST = {RS16: 32767, RU12: 2047}


def rails(fmt) -> tuple[int, int]:
    """(lowest, highest) code of a format, complex or real"""
    return (REAL_LOWEST[fmt], REAL_HIGHEST[fmt]) if fmt in REAL_FORMATS else (LOWEST[fmt], HIGHEST[fmt])
FULL_SCALE = 128.0  # the largest |code| of every format in the chain's units, "dongle LSB" (CS16 codes times 2**-8)
ADC_BINS = 17


def codes(a, fmt=None) -> np.ndarray:
    """The integer codes (int64, interleaved I,Q) the ADC meter counts: the table above."""
    a, fmt = as_samples(a, fmt)
    if fmt == RU12:
        return (a.astype(np.int64) & 4095) - 2048
    return a.astype(np.int64) - 127 if fmt == CU8 else a.astype(np.int64)


def _arm_dict(a) -> dict:
    return {"sum": int(a.sum), "sum_sq": int(a.sum_sq), "min": int(a.min), "max": int(a.max), "at_lo": int(a.at_lo),
            "at_hi": int(a.at_hi), "longest_rail_run": int(a.longest_rail_run)}


def adc_dict(r) -> dict:
    """One ``sdrx_adc_meter`` record as a dict of Python ints: ``frame``, ``n_complex``, ``fmt``, ``measured``, the arms ``i`` and
    ``q`` (dicts: ``sum``, ``sum_sq``, ``min``, ``max``, ``at_lo``, ``at_hi``, ``longest_rail_run``), ``sum_iq`` and ``bits``
    (a list of 17 counts)."""
    return {"frame": int(r.frame), "n_complex": int(r.n_complex), "fmt": int(r.fmt), "measured": int(r.measured),
            "i": _arm_dict(r.i), "q": _arm_dict(r.q), "sum_iq": int(r.sum_iq), "bits": [int(b) for b in r.bits]}


def adc_levels(rec: dict) -> dict:
    """What the record says about the front end, in the chain's units (CS16 codes times 2**-8, the 8-bit codes as they are):

    ``dc_i``, ``dc_q`` (means), ``rms`` (of the components, I and Q together, DC included), ``peak`` (largest ``|code|``),
    ``headroom_db = 20 log10(FULL_SCALE / peak)`` (inf for an all-zero frame), ``clip_share`` (components at a rail / 2n),
    ``longest_rail_run`` (the longer of the arms'), ``bits_used`` (the highest non-empty bin of ``bits``),
    ``gain_imbalance = sqrt(var_i / var_q)`` and ``phase_error = asin(cov_iq / sqrt(var_i var_q))`` in radians (nan when an
    arm is constant).  Variances and the covariance come from exact integers: ``var_i = (n sum_sq_i - sum_i**2) / n**2`` and
    ``cov_iq = (n sum_iq - sum_i sum_q) / n**2``, each numerator converted to float64 once.  ValueError for a record that was
    not measured.

    A record of REAL samples (``fmt`` RS16 or RU12: the arms are the even and the odd samples) is merged into one arm first:
    sums, sums of squares and rail counts add up, min / max are taken over both; ``dc`` (the mean), ``rms``, ``peak``,
    ``headroom_db``, ``clip_share`` (of 2 n real samples), ``bits_used`` and ``longest_rail_run`` -- the larger of the two arms',
    a LOWER BOUND: a run of consecutive real samples alternates between the arms, so it is up to twice that plus one.  No IQ
    balance: ``dc_i`` = ``dc_q`` = ``dc`` and ``gain_imbalance`` and ``phase_error`` are nan."""
    if not rec["measured"]:
        raise ValueError("the frame was not measured: it did not arrive as integer samples")
    n = int(rec["n_complex"])
    s = 2.0 ** -8 if rec["fmt"] in (CS16, RS16) else 2.0 ** -4 if rec["fmt"] == RU12 else 1.0
    i, q = rec["i"], rec["q"]
    if is_real(rec["fmt"]):
        total, total_sq = i["sum"] + q["sum"], i["sum_sq"] + q["sum_sq"]
        peak = float(max(abs(min(i["min"], q["min"])), abs(max(i["max"], q["max"])))) * s
        used = [k for k, b in enumerate(rec["bits"]) if b]
        dc = float(total) / (2.0 * float(n)) * s
        return {
            "dc": dc, "dc_i": dc, "dc_q": dc,
            "rms": float(np.sqrt(float(total_sq) / (2.0 * float(n)))) * s,
            "peak": peak,
            "headroom_db": float(20.0 * np.log10(FULL_SCALE / peak)) if peak > 0.0 else float("inf"),
            "clip_share": float(i["at_lo"] + i["at_hi"] + q["at_lo"] + q["at_hi"]) / (2.0 * float(n)),
            "longest_rail_run": max(i["longest_rail_run"], q["longest_rail_run"]),
            "longest_rail_run_is_lower_bound": True,
            "bits_used": used[-1] if used else 0,
            "gain_imbalance": float("nan"),
            "phase_error": float("nan"),
        }
    nn = float(n) * float(n)
    var_i = float(n * i["sum_sq"] - i["sum"] ** 2) / nn * s * s
    var_q = float(n * q["sum_sq"] - q["sum"] ** 2) / nn * s * s
    cov = float(n * rec["sum_iq"] - i["sum"] * q["sum"]) / nn * s * s
    peak = float(max(abs(i["min"]), abs(i["max"]), abs(q["min"]), abs(q["max"]))) * s
    used = [k for k, b in enumerate(rec["bits"]) if b]
    ok = var_i > 0.0 and var_q > 0.0
    return {
        "dc_i": float(i["sum"]) / float(n) * s,
        "dc_q": float(q["sum"]) / float(n) * s,
        "rms": float(np.sqrt(float(i["sum_sq"] + q["sum_sq"]) / (2.0 * float(n)))) * s,
        "peak": peak,
        "headroom_db": float(20.0 * np.log10(FULL_SCALE / peak)) if peak > 0.0 else float("inf"),
        "clip_share": float(i["at_lo"] + i["at_hi"] + q["at_lo"] + q["at_hi"]) / (2.0 * float(n)),
        "longest_rail_run": max(i["longest_rail_run"], q["longest_rail_run"]),
        "bits_used": used[-1] if used else 0,
        "gain_imbalance": float(np.sqrt(var_i / var_q)) if ok else float("nan"),
        "phase_error": float(np.arcsin(min(1.0, max(-1.0, cov / float(np.sqrt(var_i * var_q)))))) if ok else float("nan"),
    }


def suggest_tuner_gain(rec: dict, gains, current, headroom_db: float, unit_db: float = 0.1):
    """The entry of the front end's gain list to set next, from one ADC record: the counterpart of
    :func:`sdrreceiver_amd.meter.suggest_gains` for the gain in FRONT of the ADC.

    `gains` is the caller's list of tuner gains, sorted ascending, in steps of `unit_db` dB (librtlsdr's lists are tenths of a
    dB: 496 is 49.6 dB); `current` is the entry the frame was received with.  A change of g units moves the peak by
    ``g * unit_db`` dB, so the answer is the largest entry whose predicted headroom ``headroom_now - (entry - current) *
    unit_db`` still reaches `headroom_db` -- the peak closest to the asked headroom without going under it -- or the lowest
    entry if none does.  A record whose ``longest_rail_run`` is 2 or more saw the converter saturate: its peak is a lower bound
    only, and the answer is at most the entry below `current` (a step down at once, whatever the headroom says).  A frame
    that was not measured or is all zeros says nothing: `current` comes back.

    There is deliberately no default headroom, as there is none for squelch, AGC or scan: how far below full scale the
    strongest signal of YOUR band may come is the caller's to choose."""
    g = sorted(gains)
    if not g:
        raise ValueError("an empty gain list")
    if not rec["measured"]:
        return current
    lv = adc_levels(rec)
    if lv["peak"] <= 0.0:
        return current
    fits = [x for x in g if lv["headroom_db"] - (x - current) * float(unit_db) >= float(headroom_db)]
    pick = fits[-1] if fits else g[0]
    if lv["longest_rail_run"] >= 2:
        lower = [x for x in g if x < current]
        pick = min(pick, lower[-1] if lower else g[0])
    return pick
