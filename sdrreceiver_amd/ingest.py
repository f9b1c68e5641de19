"""The integer sample formats of the ``*_fmt`` calls (include/sdrx.h, SDRX_FMT_*) and their one host definition.

Every format maps to the reference's units, "dongle LSB, |x| <= 128" -- the units the shipped INI gains and every squelch,
AGC and watch threshold live in, and the bound the device's DC-bias removal is proved bit-exact for.  The scale is fixed:

    constant   memory                    sample value x (float32, exact)   range
    CU8 = 0    uint8 I,Q                 b - 127                           [-127, 128]
    CS8 = 1    int8 I,Q                  float(v)                          [-128, 127]
    CS16 = 2   native-endian int16 I,Q   float(v) * 2**-8                  [-128, 128)
"""
from __future__ import annotations

import numpy as np

CU8, CS8, CS16 = 0, 1, 2  # SDRX_FMT_CU8, SDRX_FMT_CS8, SDRX_FMT_CS16
FORMATS = {CU8: np.dtype(np.uint8), CS8: np.dtype(np.int8), CS16: np.dtype(np.int16)}
NAMES = {"cu8": CU8, "cs8": CS8, "cs16": CS16}


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
    if fmt not in FORMATS:
        raise ValueError(f"fmt {fmt!r}: CU8 (0), CS8 (1) or CS16 (2)")
    a = np.asarray(a)
    if a.dtype != FORMATS[fmt]:
        raise TypeError(f"format {fmt} takes {FORMATS[fmt]}, not {a.dtype}")
    return np.ascontiguousarray(a).reshape(-1), int(fmt)


def to_float(a, fmt=None) -> np.ndarray:
    """The float32 samples the library computes from the integer samples `a`: the table above, exactly."""
    a, fmt = as_samples(a, fmt)
    if fmt == CU8:
        return (a.astype(np.int32) - 127).astype(np.float32)
    if fmt == CS8:
        return a.astype(np.float32)
    return a.astype(np.float32) * np.float32(2.0 ** -8)
