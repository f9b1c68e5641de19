"""Device-side wake (option ``wake``): the watch parks and unparks leaves itself, inside the frame.  include/sdrx.h ("Device-side
wake") has the definition; this module has the settings of a leaf, the rule on the host -- :func:`step`, in numpy doubles, bit
for bit what the device decides from the figures :meth:`Receiver.watch` reports -- and the records as arrays.

No default threshold, contrast or hold time is offered: what a real front end needs has not been measured (the stance of the
squelch, the AGC and the scan).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

BINS = 8192  # SDRX_SPECTRUM_BINS


@dataclass(frozen=True)
class Cfg:
    """``sdrx_wake_cfg``: a leaf is hot in a frame when its ``band_pwr`` reaches `min_band_pwr` and -- `contrast_q8` > 0 -- the
    power density inside its band is at least ``contrast_q8 / 256`` times the density outside; it stays active `hold_frames`
    frames after the last hot one.  `on` 1 puts the leaf under the device's control, 0 releases it."""
    min_band_pwr: float
    contrast_q8: int = 0
    hold_frames: int = 0
    on: int = 1
    reserved: tuple = (0, 0, 0)


def invalid(cfg: Cfg) -> str | None:
    """What ``sdrx_set_wake`` refuses about the setting itself (the leaf's own conditions -- watched, no enabled spectrum --
    come first there), or None."""
    if cfg.on not in (0, 1):
        return "on must be 0 or 1"
    b = float(cfg.min_band_pwr)
    if not math.isfinite(b) or not b >= 0.0:
        return "min_band_pwr must be finite and not negative"
    if any(int(r) != 0 for r in cfg.reserved):
        return "a reserved field is not 0"
    return None


def step(cfg: Cfg, hold_left: int, band_pwr, total_pwr, n_bins: int) -> tuple[int, int, int]:
    """The rule for one leaf and frame: ``(active, hot, hold_left)`` from the leaf's watch record (``band_pwr``, ``total_pwr``,
    ``n_bins``) and the ``hold_left`` the frame before left.  IEEE double, one rounding per operation; both integer factors are
    exact in double; a NaN is not hot."""
    b, t = np.float64(band_pwr), np.float64(total_pwr)
    n, q = int(n_bins), int(cfg.contrast_q8)
    c_ok = q == 0
    if not c_ok and n < BINS:
        with np.errstate(all="ignore"):
            lhs = b * np.float64(256 * (BINS - n))
            rhs = (t - b) * np.float64(q * n)
        c_ok = bool(lhs >= rhs)
    hot = bool(b >= np.float64(cfg.min_band_pwr)) and c_ok
    if hot:
        return 1, 1, int(cfg.hold_frames)
    if hold_left > 0:
        return 1, 0, int(hold_left) - 1
    return 0, 0, 0


def wake_dict(recs) -> dict:
    """``sdrx_wake_state`` records -> arrays: ``frame``, ``since_frame``, ``active``, ``hot``, ``hold_left``, ``controlled``."""
    return {"frame": np.array([r.frame for r in recs], dtype=np.int64),
            "since_frame": np.array([r.since_frame for r in recs], dtype=np.int64),
            "active": np.array([r.active for r in recs], dtype=np.int32),
            "hot": np.array([r.hot for r in recs], dtype=np.int32),
            "hold_left": np.array([r.hold_left for r in recs], dtype=np.uint32),
            "controlled": np.array([r.controlled for r in recs], dtype=np.int32)}
