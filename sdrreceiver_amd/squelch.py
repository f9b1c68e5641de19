"""Squelch-gated egress (option ``squelch``): the definition the device is held to, and a threshold helper.

Per leaf: a threshold ``thr`` in units of the meter's ``sum_sq`` (0 = always open, the default), a hang time
``hang_frames`` and a state ``hang_left`` (0 after finalize, and after every ``set_squelch`` that names the leaf).
For every frame, with ``s`` the leaf's meter ``sum_sq`` of that frame (:mod:`sdrreceiver_amd.meter`)::

    if   s >= thr:        open = 1; hang_left = hang_frames
    elif hang_left > 0:   open = 1; hang_left -= 1
    else:                 open = 0

Integers only, so the decision is exact.  The library decides on the device (``k_squelch_scan``), packs the open
leaves' payloads and copies only those to the host; :func:`decide` restates the rule for the tests.

Option ``preroll`` adds one bit of state per leaf, ``prev_open``: 1 after finalize (frame 0 has no predecessor), and after
every frame that frame's ``open``; ``set_squelch`` does not touch it.  With ``open(f)`` as above::

    pre(f) = open(f) and not prev_open;   prev_open = open(f)

A frame with ``pre(f) = 1`` for a leaf is delivered with the leaf's payload of frame ``f-1`` ahead of that of ``f``
(:func:`preroll_flags`).  One frame and no more: it is what the device still holds.

There is deliberately no default threshold: what level separates a live channel from an idle one on a real front end
has not been measured.  Read ``meters()`` of the closed leaves (they are always reported) and choose.
"""
from __future__ import annotations

import math

import numpy as np

NEVER_OPEN = 1 << 63  # no int16 / int8 frame reaches it


def align64(n: int) -> int:
    """Payloads are packed in 64-byte units."""
    return (int(n) + 63) // 64 * 64


def decide(sum_sq_per_frame, thr, hang_frames, hang_left: int = 0, return_state: bool = False):
    """The open flag of one leaf for each frame of `sum_sq_per_frame` (python ints, exact), starting from
    `hang_left`.  With `return_state` also the ``hang_left`` after every frame."""
    thr, hang_frames, left = int(thr), int(hang_frames), int(hang_left)
    flags, lefts = [], []
    for s in sum_sq_per_frame:
        if int(s) >= thr:
            is_open, left = 1, hang_frames
        elif left > 0:
            is_open, left = 1, left - 1
        else:
            is_open = 0
        flags.append(is_open)
        lefts.append(left)
    flags = np.array(flags, np.int32).reshape(len(flags))
    if return_state:
        return flags, np.array(lefts, np.int64).reshape(len(lefts))
    return flags


def preroll_flags(open_flags, prev_open: int = 1):
    """The pre-roll flag of one leaf for each frame of `open_flags` (what :func:`decide` returns), starting from
    `prev_open` (1 after finalize)."""
    prev, out = int(bool(prev_open)), []
    for o in open_flags:
        o = int(bool(o))
        out.append(int(o and not prev))
        prev = o
    return np.array(out, np.int32).reshape(len(out))


def threshold(rms_dbfs: float, n_values: int, full_scale: float) -> int:
    """The ``sum_sq`` of `n_values` values whose RMS is `rms_dbfs` below `full_scale` (32768 for a USB leaf's int16,
    128 for a compress() leaf's int8 components): ``ceil((10**(rms_dbfs/20) * full_scale)**2 * n_values)``."""
    rms = 10.0 ** (float(rms_dbfs) / 20.0) * float(full_scale)
    return int(math.ceil(rms * rms * int(n_values)))


def squelch_dict(records) -> dict:
    """``sdrx_squelch_state`` records (in the order asked for) as arrays."""
    n = len(records)
    return {
        "frame": np.array([r.frame for r in records], np.int64).reshape(n),
        "thr_sum_sq": np.array([r.thr_sum_sq for r in records], np.uint64).reshape(n),
        "hang_frames": np.array([r.hang_frames for r in records], np.int64).reshape(n),
        "hang_left": np.array([r.hang_left for r in records], np.int64).reshape(n),
        "open": np.array([r.open for r in records], np.int32).reshape(n),
    }
