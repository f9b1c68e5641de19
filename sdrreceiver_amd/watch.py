"""Channel watch (option ``watch``): the power inside a leaf's passband, measured on the stream the leaf is fed -- its parent's
``decimate[d]`` or the raw frame -- whether the leaf runs or is parked.  include/sdrx.h ("Channel watch") has the definition;
this module has the band of a leaf on the host and what a host does with the figures: ``watch -> wake_list -> set_mixer_freqs /
set_active``.

No default contrast is offered: what a real front end needs has not been measured (the stance of
:func:`sdrreceiver_amd.meter.suggest_gains` and of the auto-squelch).
"""
from __future__ import annotations

import math

import numpy as np

BINS = 8192          # SDRX_SPECTRUM_BINS
MAX_SEGMENTS = 16    # SDRX_WATCH_MAX_SEGMENTS


def band(desc) -> tuple[int, int]:
    """``(first_bin, n_bins)`` of the leaf `desc` (a :class:`sdrreceiver_amd.topology.VfoDesc`) in the 8192-point spectrum of
    its source.  The mixer multiplies by ``exp(+j 2 pi f t)``: a component at g in the source lands at g + f in the leaf, so a
    USB leaf hears ``[-f, -f + B]`` and a compress leaf ``[-f - R/2, -f + R/2]``."""
    f, fs = float(desc.mixer_freq), float(desc.fs)
    r = fs / float(1 << desc.decimate_count)
    if desc.demod_usb:
        r_out = r / float(desc.late_decimate) if desc.late_decimate in (5, 6) else r
        b = float(desc.filter_bw) if desc.filter_bw > 0 else r_out / 2
        b = min(b, r_out / 2)
        lo, hi = -f, -f + b
    else:
        lo, hi = -f - r / 2, -f + r / 2
    k_lo, k_hi = math.ceil(lo * 8192.0 / fs), math.floor(hi * 8192.0 / fs)
    return k_lo % BINS, min(max(k_hi - k_lo + 1, 1), BINS)


def watch_dict(recs) -> dict:
    """``sdrx_watch_level`` records -> arrays: ``frame``, ``band_pwr``, ``total_pwr``, ``first_bin``, ``n_bins``, ``segments``,
    ``watched``."""
    return {"frame": np.array([r.frame for r in recs], dtype=np.int64),
            "band_pwr": np.array([r.band_pwr for r in recs], dtype=np.float64),
            "total_pwr": np.array([r.total_pwr for r in recs], dtype=np.float64),
            "first_bin": np.array([r.first_bin for r in recs], dtype=np.int32),
            "n_bins": np.array([r.n_bins for r in recs], dtype=np.int32),
            "segments": np.array([r.segments for r in recs], dtype=np.int32),
            "watched": np.array([r.watched for r in recs], dtype=np.int32)}


def contrast(levels: dict) -> np.ndarray:
    """Power density inside the band over the density outside it,
    ``(band_pwr / n_bins) / ((total_pwr - band_pwr) / (8192 - n_bins))``; NaN where the band is the whole spectrum."""
    band_pwr = np.asarray(levels["band_pwr"], dtype=np.float64)
    total = np.asarray(levels["total_pwr"], dtype=np.float64)
    n = np.asarray(levels["n_bins"], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (band_pwr / n) / ((total - band_pwr) / (BINS - n))
    return np.where(n >= BINS, np.nan, out)


def wake_list(vids, levels: dict, min_contrast: float) -> list[int]:
    """The leaves of `vids` (in the order of `levels`) that were watched and whose contrast reached `min_contrast`: the ones
    to retune and unpark."""
    c = contrast(levels)
    watched = np.asarray(levels["watched"]) != 0
    return [int(v) for v, ck, w in zip(np.asarray(vids).reshape(-1).tolist(), c.tolist(), watched.tolist()) if w and ck >= min_contrast]
