"""Drift estimate (part of option ``watch``): by how many Hz the band of a watched source has moved since its template was taken.
include/sdrx.h ("Drift estimate") has the definition -- the device correlates the source's power spectrum with a template over
the shifts ``-K .. K`` and reports the first maximum with its neighbours; this module has what a host does with the record:

    rx.set_drift(leaf, max_shift=64)                  # capture: the next frame's spectrum is the template
    ...
    hz = drift.estimate_hz(rx.drift(leaf), topo.vfos[leaf].fs)
    ids, freqs = topology.mix_offset_retune(topo, ini_text, drift.new_mix_offset(offset_at_capture, hz))
    rx.set_mixer_freqs(ids, freqs)

The estimate is absolute since the template was taken (retuning the subs does not change the source's spectrum), so there is
no loop gain to choose.  Nothing is applied automatically, and no default ``max_shift`` or template is offered.
"""
from __future__ import annotations

import numpy as np

from . import watch as _watch

BINS = _watch.BINS    # SDRX_SPECTRUM_BINS
MAX_SHIFT = 1024      # SDRX_DRIFT_MAX_SHIFT


def drift_dict(rec) -> dict:
    """An ``sdrx_drift_level`` record as a dict: ``frame``, ``peak``, ``left``, ``right``, ``zero``, ``shift``, ``max_shift``,
    ``measured``, ``captured``."""
    return {"frame": int(rec.frame), "peak": float(rec.peak), "left": float(rec.left), "right": float(rec.right),
            "zero": float(rec.zero), "shift": int(rec.shift), "max_shift": int(rec.max_shift), "measured": int(rec.measured),
            "captured": int(rec.captured)}


def estimate_bins(level: dict) -> float:
    """The shift in bins with the parabola through the peak and its neighbours: ``shift + 0.5 (left - right) / (left - 2 peak +
    right)``; plain ``shift`` at the edge of the window (``shift = +-max_shift``) or when the denominator is 0."""
    shift, k = int(level["shift"]), int(level["max_shift"])
    left, peak, right = float(level["left"]), float(level["peak"]), float(level["right"])
    den = left - 2.0 * peak + right
    if abs(shift) >= k or den == 0.0:
        return float(shift)
    return shift + 0.5 * (left - right) / den


def estimate_hz(level: dict, fs_source: float) -> float:
    """The drift in Hz: :func:`estimate_bins` times the source's bin width ``fs_source / 8192`` (`fs_source`: the ``fs`` of a leaf
    of the source).  Positive: the band appears higher in the source than when the template was taken."""
    return estimate_bins(level) * float(fs_source) / BINS


def mask_template(topo, leaf_ids) -> np.ndarray:
    """A template without a capture, for plans whose signals fill their bands: per bin the number of the leaves `leaf_ids` (all
    of one source) whose band (:func:`sdrreceiver_amd.watch.band`) covers it.  8192 float64."""
    parents = {topo.vfos[i].parent for i in leaf_ids}
    if len(parents) > 1:
        raise ValueError(f"the leaves {list(leaf_ids)} have different sources: {sorted(parents)}")
    t = np.zeros(BINS, np.float64)
    for i in leaf_ids:
        first, n = _watch.band(topo.vfos[i])
        np.add.at(t, (first + np.arange(n)) % BINS, 1.0)
    return t


def new_mix_offset(offset_at_capture: int, hz: float) -> int:
    """The INI's ``mix_offset`` that takes a drift of `hz` out again, for :func:`sdrreceiver_amd.topology.mix_offset_retune`: the
    offset the tree had when the template was taken plus the estimate, rounded to the INI's integer Hz."""
    return int(offset_at_capture) + int(round(float(hz)))
