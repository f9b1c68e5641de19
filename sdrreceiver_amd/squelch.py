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

Option ``squelch_auto`` makes the threshold relative to the leaf's own noise floor, so that nobody has to choose an
absolute level per leaf and the gate follows gain changes, retunes and the front end.  Two more settings per leaf,
``ratio_q8`` (a power ratio times 256; 0 = off for the leaf, the default; :func:`ratio_q8_from_db`) and ``window_frames``
(at least 1 where ``ratio_q8 > 0``), and three more words of state: ``cur_min``, ``prev_min`` (:data:`NONE` = 2^64 - 1 is "no
observation") and ``age``; ``cur_min = prev_min = NONE, age = 0`` after finalize and after every ``set_squelch_auto`` that
names the leaf.  For every frame (:func:`decide_auto`)::

    floor   = min(cur_min, prev_min)                       # from the frames BEFORE this one
    auto    = 0 if ratio_q8 == 0 or floor == NONE else min(2^64 - 1, (floor * ratio_q8) >> 8)
    thr_eff = max(thr, auto)                               # the manual threshold stays a lower bound
    open / hang_left: the rule above with thr_eff in place of thr
    cur_min = min(cur_min, s);  age += 1
    if age == window_frames:  prev_min = cur_min;  cur_min = NONE;  age = 0

Minimum statistics over a sliding window of ``window_frames`` to ``2 * window_frames - 1`` frames.  What follows:

* the first frame after finalize or a restart decides with ``thr`` alone (open, with the defaults);
* a frame of zeros makes the floor 0, so ``thr_eff = thr``: a gap fails open, for at most ``2 * window_frames - 1`` frames;
* a burst never lifts its own threshold (the floor excludes the current frame), but a transmission longer than
  ``2 * window_frames - 1`` frames becomes the floor and, with ``ratio_q8 > 256``, closes: ``window_frames`` is chosen above
  the longest transmission, and continuous channels keep ``ratio_q8 = 0``;
* ``set_squelch`` does not touch the floor state; ``set_squelch_auto`` does not touch ``thr``, ``hang_frames``,
  ``hang_left`` or ``prev_open``; pre-roll follows ``open`` as before.

There is still no default, neither an absolute threshold nor a ratio or window: what separates a live channel from an idle
one on a real front end has not been measured.  But a ratio over the leaf's own floor needs no measurement of the floor:
for an absolute level read ``meters()`` of the closed leaves (they are always reported) and choose; otherwise pick a ratio
(a few dB) and a window longer than the longest transmission.
"""
from __future__ import annotations

import math

import numpy as np

NEVER_OPEN = 1 << 63  # no int16 / int8 frame reaches it
NONE = (1 << 64) - 1  # squelch_auto: no observation


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


def decide_auto(sum_sq_per_frame, thr, hang_frames, ratio_q8, window_frames, hang_left: int = 0, cur_min: int = NONE,
                prev_min: int = NONE, age: int = 0, return_state: bool = False):
    """The auto-squelch rule for one leaf over the frames of `sum_sq_per_frame` (python ints, exact), from the starting
    state `hang_left`, `cur_min`, `prev_min`, `age` (the defaults: after finalize or a restart).  A dict of per-frame
    arrays: ``open`` and ``hang_left`` (after the frame) as :func:`decide` gives them, ``thr_eff``, ``floor`` (uint64; 0
    where ``floor_valid`` is 0) and ``floor_valid`` -- the values that decided the frame.  With `return_state` also
    ``state``: ``(hang_left, cur_min, prev_min, age)`` after the last frame, to carry on from."""
    thr, hang_frames, left = int(thr), int(hang_frames), int(hang_left)
    ratio, window = int(ratio_q8), int(window_frames)
    cur, prev, age = int(cur_min), int(prev_min), int(age)
    if ratio > 0 and window < 1:
        raise ValueError("window_frames must be at least 1 where ratio_q8 > 0")
    flags, lefts, effs, floors, valid = [], [], [], [], []
    for s in sum_sq_per_frame:
        s = int(s)
        floor = min(cur, prev)
        auto = 0 if ratio == 0 or floor == NONE else min(NONE, (floor * ratio) >> 8)
        eff = max(thr, auto)
        if s >= eff:
            is_open, left = 1, hang_frames
        elif left > 0:
            is_open, left = 1, left - 1
        else:
            is_open = 0
        cur = min(cur, s)
        age += 1
        if age == window:
            prev, cur, age = cur, NONE, 0
        flags.append(is_open)
        lefts.append(left)
        effs.append(eff)
        floors.append(0 if floor == NONE else floor)
        valid.append(int(floor != NONE))
    n = len(flags)
    out = {
        "open": np.array(flags, np.int32).reshape(n),
        "hang_left": np.array(lefts, np.int64).reshape(n),
        "thr_eff": np.array(effs, np.uint64).reshape(n),
        "floor": np.array(floors, np.uint64).reshape(n),
        "floor_valid": np.array(valid, np.int32).reshape(n),
    }
    if return_state:
        out["state"] = (left, cur, prev, age)
    return out


def ratio_q8_from_db(db: float) -> int:
    """``ratio_q8`` of a power ratio of `db` decibels: ``round(256 * 10**(db/10))``.  A result of 0 would switch the leaf's
    auto-squelch off by accident and is refused, as is one beyond uint32."""
    q = int(round(256.0 * 10.0 ** (float(db) / 10.0)))
    if q <= 0 or q > 0xFFFFFFFF:
        raise ValueError(f"{db} dB gives ratio_q8 = {q}: outside 1 .. 2^32 - 1 (0 means off)")
    return q


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


def squelch_auto_dict(records) -> dict:
    """``sdrx_squelch_auto_state`` records (in the order asked for) as arrays."""
    n = len(records)
    return {
        "frame": np.array([r.frame for r in records], np.int64).reshape(n),
        "floor_sum_sq": np.array([r.floor_sum_sq for r in records], np.uint64).reshape(n),
        "thr_eff_sum_sq": np.array([r.thr_eff_sum_sq for r in records], np.uint64).reshape(n),
        "ratio_q8": np.array([r.ratio_q8 for r in records], np.uint32).reshape(n),
        "window_frames": np.array([r.window_frames for r in records], np.uint32).reshape(n),
        "floor_valid": np.array([r.floor_valid for r in records], np.int32).reshape(n),
    }
