"""Band scan (part of option ``watch``): the carriers in a watched source's spectrum, found on the device.  include/sdrx.h
("Band scan") has the definition -- the source's power spectrum integrated over M frames, folded into cells of w bins, a
floor taken as a rank statistic of the cells, every run of cells above ``ratio_q8 / 256`` times the floor reported as a hit;
this module has what a host does with a hit:

    rx.set_scan(leaf, cell_bins=4, frames=3, floor_permille=500, ratio_q8=16 * 256)
    ... frames ...
    if rx.scan(leaf)["complete"]:
        hits, frame = rx.scan_hits(leaf)
        bands = [scan.leaf_band_hz(topo.vfos[i]) for i in active_leaves]
        for hit in scan.unassigned(hits, 4, fs_source, bands):
            rx.set_mixer_freqs([spare], [scan.mixer_for(topo.vfos[spare], scan.hit_hz(hit, 4, fs_source)[2])])
            rx.set_active([spare], [1])          # with option catchup: the leaf hears the frame the scan completed on

No default ``ratio_q8``, ``floor_permille`` or cell width is offered: what a real front end needs has not been measured (the
stance of the squelch and AGC windows).
"""
from __future__ import annotations

from . import watch as _watch

BINS = _watch.BINS    # SDRX_SPECTRUM_BINS
MAX_HITS = 512        # SDRX_SCAN_MAX_HITS


def scan_dict(rec) -> dict:
    """An ``sdrx_scan_level`` record as a dict: ``frame``, ``floor``, ``thr``, ``n_hits``, ``n_stored``, ``n_hot``, ``integrated``,
    ``frames``, ``cell_bins``, ``measured``, ``complete``."""
    return {"frame": int(rec.frame), "floor": float(rec.floor), "thr": float(rec.thr), "n_hits": int(rec.n_hits),
            "n_stored": int(rec.n_stored), "n_hot": int(rec.n_hot), "integrated": int(rec.integrated), "frames": int(rec.frames),
            "cell_bins": int(rec.cell_bins), "measured": int(rec.measured), "complete": int(rec.complete)}


def hit_dict(hit) -> dict:
    """An ``sdrx_scan_hit`` as a dict: ``first_cell``, ``n_cells``, ``peak_cell``, ``peak_pwr``."""
    return {"first_cell": int(hit.first_cell), "n_cells": int(hit.n_cells), "peak_cell": int(hit.peak_cell),
            "peak_pwr": float(hit.peak_pwr)}


def hit_hz(hit: dict, cell_bins: int, fs: float) -> tuple[float, float, float]:
    """``(lo, hi, peak)`` of a hit in Hz of the source (`fs`: the source's rate, the ``fs`` of a leaf of it): the centres of its
    first and last bin, and the middle of its peak cell."""
    w, half, hz = int(cell_bins), BINS // 2, float(fs) / BINS
    lo = (hit["first_cell"] * w - half) * hz
    hi = ((hit["first_cell"] + hit["n_cells"]) * w - 1 - half) * hz
    peak = (hit["peak_cell"] * w + (w - 1) / 2.0 - half) * hz
    return lo, hi, peak


def leaf_band_hz(desc) -> tuple[float, float]:
    """``[lo, hi]`` in Hz of the source that the leaf `desc` hears, as the watch defines it: a USB leaf ``[-f, -f + B]``, a compress
    leaf ``[-f - R/2, -f + R/2]``."""
    f, r = float(desc.mixer_freq), float(desc.fs) / float(1 << desc.decimate_count)
    if not desc.demod_usb:
        return -f - r / 2, -f + r / 2
    return -f, -f + _usb_width(desc)


def _usb_width(desc) -> float:
    r = float(desc.fs) / float(1 << desc.decimate_count)
    r_out = r / float(desc.late_decimate) if desc.late_decimate in (5, 6) else r
    b = float(desc.filter_bw) if desc.filter_bw > 0 else r_out / 2
    return min(b, r_out / 2)


def mixer_for(desc, hz: float) -> int:
    """The integer mixer frequency that puts `hz` (Hz of the source) in the middle of the watch band of the leaf `desc`: a USB leaf
    hears ``[-f, -f + B]``, so ``f = rint(B/2 - hz)``; a compress leaf hears ``-f +- R/2``, so ``f = rint(-hz)``."""
    if desc.demod_usb:
        return int(round(_usb_width(desc) / 2 - float(hz)))
    return int(round(-float(hz)))


def unassigned(hits, cell_bins: int, fs: float, bands) -> list:
    """The hits whose ``[lo, hi]`` (:func:`hit_hz`) overlaps none of `bands` -- ``(lo, hi)`` pairs in Hz of the source
    (:func:`leaf_band_hz`), closed intervals."""
    out = []
    for h in hits:
        lo, hi, _ = hit_hz(h, cell_bins, fs)
        if not any(lo <= b_hi and b_lo <= hi for b_lo, b_hi in bands):
            out.append(h)
    return out
