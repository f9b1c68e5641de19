"""Device-side AGC (option ``agc``): the rule the device is held to, and a helper for choosing the window.

After every frame ``k_agc_step`` moves the gain of each USB leaf from that frame's output meter, for the NEXT frame -- the
reference's own ``vfo::setGain`` between two ``vfo::process`` calls, so every frame stays bit for bit what the reference
produces with the gain that frame had.  The reference has no AGC: its README tells the user to move the VFO gain until
JAERO's volume light is green.

Settings per leaf (:class:`Cfg` = ``sdrx_agc_cfg``; all zero after finalize: off) and one word of state, ``quiet_run`` (0
after finalize, after every ``set_agc`` that names the leaf and after an unpark).  With ``s`` the leaf's meter ``sum_sq`` of
the frame, ``n`` its ``n_values``, ``clipped`` as :mod:`sdrreceiver_amd.meter` defines them and ``g`` the gain the frame was
computed with (:func:`step`)::

    parked in f, or n == 0, or hi_ms == 0:   g' = g, action 0, quiet_run unchanged
    hot    = clipped > 0 or s > hi_ms * n
    silent = not hot and s < silent_ms * n
    cold   = not hot and not silent and s < lo_ms * n
    hot:     g' = clamp(fl(g * down)); quiet_run = 0; action -1
    silent:  g' = g; action 0; quiet_run unchanged
    cold:    quiet_run = min(quiet_run + 1, 2^32 - 1)
             if quiet_run > hold_frames: g' = clamp(fl(g * up)), action +1   else g' = g, action 0
    else:    g' = g; quiet_run = 0; action 0
    clamp(x) = fminf(fmaxf(x, gain_min), gain_max)

Integers (the products fit uint64) and one float32 multiply: exact on both sides.  ``hot`` wins because a wrapped payload's
``sum_sq`` is that of the wrapped values -- the rule :func:`sdrreceiver_amd.meter.suggest_gains` follows too.  The clamp acts
only when the AGC moves the gain: a gain the host set outside the limits stays while the leaf is in its window.

Choosing the window: the output scales with ``g``, its mean square with ``g^2``, so a steady input never alternates between
the two steps when ``hi_ms >= lo_ms * max(up^2, 1 / down^2)`` (:func:`window_is_stable`; the library does not check it).
There is no default window or step: what JAERO's green light corresponds to has not been measured.
:func:`window_from_dbfs` turns a pair of RMS levels in dBFS into ``lo_ms`` / ``hi_ms``.

The host loop (:func:`sdrreceiver_amd.meter.suggest_gains` + ``set_gains``) is still the right tool for a proportional
one-frame correction on a host that is synchronous anyway; it cannot serve frames in flight or queued on the device.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

FULL_SCALE_MS = 1 << 30  # 32768^2: the largest mean square of an int16 payload, and the largest hi_ms
QUIET_MAX = (1 << 32) - 1


@dataclasses.dataclass(frozen=True)
class Cfg:
    """``sdrx_agc_cfg``"""
    lo_ms: int = 0
    hi_ms: int = 0
    silent_ms: int = 0
    hold_frames: int = 0
    up: float = 1.0
    down: float = 1.0
    gain_min: float = 1.0
    gain_max: float = 1.0


def invalid(cfg: Cfg, usb: bool = True) -> str | None:
    """What ``sdrx_set_agc`` refuses about `cfg` for a leaf that does (`usb`) or does not demodulate USB; None: accepted."""
    if cfg.hi_ms == 0:
        return None
    if not (0 <= cfg.silent_ms <= cfg.lo_ms <= cfg.hi_ms <= FULL_SCALE_MS):
        return "the window needs silent_ms <= lo_ms <= hi_ms <= 2^30"
    f = [np.float32(cfg.up), np.float32(cfg.down), np.float32(cfg.gain_min), np.float32(cfg.gain_max)]
    if not all(np.isfinite(v) for v in f):
        return "up, down, gain_min and gain_max must be finite"
    if not (f[0] >= 1 and 0 < f[1] <= 1):
        return "the steps need up >= 1 and 0 < down <= 1"
    if not (0 < f[2] <= f[3]):
        return "the limits need 0 < gain_min <= gain_max"
    if not usb:
        return "the leaf does not demodulate USB"
    return None


def clamp(x, cfg: Cfg) -> np.float32:
    """``fminf(fmaxf(x, gain_min), gain_max)``: +inf clamps to ``gain_max``, a NaN to ``gain_min``."""
    return np.float32(np.fmin(np.fmax(np.float32(x), np.float32(cfg.gain_min)), np.float32(cfg.gain_max)))


def step(cfg: Cfg, quiet_run: int, gain, meter: dict, parked: bool = False) -> tuple[np.float32, int, int]:
    """One leaf, one frame: ``(gain_next, quiet_run, action)`` from the settings, the state in front of the frame, the gain
    the frame was computed with and the frame's meter (``sum_sq``, ``n_values``, ``clipped``: Python integers)."""
    g = np.float32(gain)
    q = int(quiet_run)
    s, n, clipped = int(meter["sum_sq"]), int(meter["n_values"]), int(meter["clipped"])
    if parked or n == 0 or int(cfg.hi_ms) == 0:
        return g, q, 0
    hot = clipped > 0 or s > int(cfg.hi_ms) * n
    silent = not hot and s < int(cfg.silent_ms) * n
    cold = not hot and not silent and s < int(cfg.lo_ms) * n
    with np.errstate(over="ignore"):
        if hot:
            return clamp(g * np.float32(cfg.down), cfg), 0, -1
        if silent:
            return g, q, 0
        if cold:
            q = min(q + 1, QUIET_MAX)
            if q > int(cfg.hold_frames):
                return clamp(g * np.float32(cfg.up), cfg), q, 1
            return g, q, 0
    return g, 0, 0


def ms_from_dbfs(rms_dbfs: float) -> int:
    """The mean square in LSB^2 of an int16 payload whose RMS is `rms_dbfs` (0 dBFS = 32768 LSB), rounded to an integer
    and held inside 0 .. 2^30."""
    return max(0, min(FULL_SCALE_MS, int(round(FULL_SCALE_MS * 10.0 ** (float(rms_dbfs) / 10.0)))))


def window_from_dbfs(lo_rms_dbfs: float, hi_rms_dbfs: float) -> tuple[int, int]:
    """``(lo_ms, hi_ms)`` for a window between two RMS levels in dBFS; ``hi_ms`` is at least 1 (0 would switch the AGC off)
    and at least ``lo_ms``."""
    lo = ms_from_dbfs(lo_rms_dbfs)
    hi = max(ms_from_dbfs(hi_rms_dbfs), lo, 1)
    return lo, hi


def window_is_stable(cfg: Cfg) -> bool:
    """``hi_ms >= lo_ms * max(up^2, 1 / down^2)``: a steady input never alternates between the two steps."""
    up, down = float(np.float32(cfg.up)), float(np.float32(cfg.down))
    return cfg.hi_ms >= cfg.lo_ms * max(up * up, 1.0 / (down * down) if down > 0 else math.inf)


def agc_dict(records) -> dict:
    """``sdrx_agc_state`` records (in the order asked for) as arrays."""
    n = len(records)
    d = {
        "frame": np.array([r.frame for r in records], np.int64).reshape(n),
        "gain_used": np.array([r.gain_used for r in records], np.float32).reshape(n),
        "gain_next": np.array([r.gain_next for r in records], np.float32).reshape(n),
        "action": np.array([r.action for r in records], np.int32).reshape(n),
        "quiet_run": np.array([r.quiet_run for r in records], np.int64).reshape(n),
    }
    for name, dt in (("lo_ms", np.int64), ("hi_ms", np.int64), ("silent_ms", np.int64), ("hold_frames", np.int64),
                     ("up", np.float32), ("down", np.float32), ("gain_min", np.float32), ("gain_max", np.float32)):
        d[name] = np.array([getattr(r.cfg, name) for r in records], dt).reshape(n)
    return d
