"""numpy model of the channel watch (option "watch", include/sdrx.h "Channel watch") for the tests: the yardstick, since the
reference has no counterpart.

* :func:`segments`, :func:`psd` -- S segments of min(8192, n) samples, each through spectrum_ref's Hann window and kiss_fft
  (pinned to the real kiss_fft by tests/golden/spectrum.npz), fp32 power ``fl(fl(im*im) + fl(re*re))``, summed over the
  segments in ascending order in float64.
* :func:`band` -- a leaf's bins, written on its own (not the product's sdrreceiver_amd.watch.band).
* :func:`levels` -- band and total power with ``math.fsum`` (the exact sum, correctly rounded).
* :func:`watch_tree`, :func:`tone_for` -- the small two-level tree of the sign-and-placement test and of the GPU tests.
"""
from __future__ import annotations

import math

import numpy as np

import spectrum_ref as sr
from sdrreceiver_amd.topology import Topology, VfoDesc

N = sr.N
MAX_SEGMENTS = 16


def segments(n: int) -> tuple[int, list[int]]:
    """(S, [start of segment s])"""
    S = min(max(n // N, 1), MAX_SEGMENTS)
    return S, [s * (n // S) for s in range(S)]


def segment_power(seg: np.ndarray) -> np.ndarray:
    """P_s of one segment of at most 8192 samples (zero-padded by the window step), float32."""
    out = sr.kiss_fft(sr.windowed(seg))
    re, im = out.real.astype(np.float32), out.imag.astype(np.float32)
    return (im * im + re * re).astype(np.float32)


def psd(stream: np.ndarray) -> np.ndarray:
    x = np.asarray(stream, np.complex64).reshape(-1)
    S, starts = segments(x.size)
    take = min(N, x.size)
    acc = np.zeros(N, np.float64)
    for st in starts:
        acc = acc + segment_power(x[st:st + take]).astype(np.float64)
    return acc


def band(desc) -> tuple[int, int]:
    """(first_bin, n_bins) of a leaf descriptor, in float64 as the definition says."""
    f = np.float64(desc.mixer_freq)
    fs = np.float64(desc.fs)
    R = fs / np.float64(2 ** desc.decimate_count)
    if desc.demod_usb:
        R_out = R / np.float64(desc.late_decimate) if desc.late_decimate in (5, 6) else R
        half = R_out / np.float64(2.0)
        B = np.float64(desc.filter_bw) if desc.filter_bw > 0 else half
        if B > half:
            B = half
        lo, hi = -f, -f + B
    else:
        lo, hi = -f - R / np.float64(2.0), -f + R / np.float64(2.0)
    k_lo = int(np.ceil(lo * np.float64(8192.0) / fs))
    k_hi = int(np.floor(hi * np.float64(8192.0) / fs))
    n_bins = k_hi - k_lo + 1
    n_bins = 1 if n_bins < 1 else N if n_bins > N else n_bins
    first = k_lo
    while first < 0:
        first += N
    while first >= N:
        first -= N
    return first, n_bins


def bins_of(first_bin: int, n_bins: int) -> np.ndarray:
    return (first_bin + np.arange(n_bins)) % N


def levels(p: np.ndarray, first_bin: int, n_bins: int) -> tuple[float, float]:
    """(band_pwr, total_pwr): exact sums"""
    return math.fsum(p[bins_of(first_bin, n_bins)].tolist()), math.fsum(p.tolist())


def contrast(band_pwr: float, total_pwr: float, n_bins: int) -> float:
    return (band_pwr / n_bins) / ((total_pwr - band_pwr) / (N - n_bins))


# ---- the small two-level tree -------------------------------------------------------------------------------------------
WT_FS, WT_FRAME = 245760, 61440          # the main: 3 half-band stages -> 30 720 S/s, 7 680 samples per frame (zero-padded)
WT_MAIN_MIXER = 21000.0
WT_USB_MIXERS = [-9000.0 + 2300.0 * k for k in range(8)]  # bands [-f, -f + B] 2 300 Hz apart, B <= 960: none overlaps, and a tone
#                                                            mid-band of one sub lies in the stop band of its neighbours' last half-band stage
WT_LATE = 5                              # USB sub 5 decimates by 5 behind its stages: B = 192
WT_GAIN = 0.003                          # (no int16 wraps: asserted by the test)
WT_COMPRESS_MIXER = 12500.0              # band [-14 420, -10 580]: below every USB band


def watch_tree() -> Topology:
    """Node 0: the main.  1..8: USB subs at d = 4 (1 920 S/s; node 6 with late_decimate 5).  9: a compress sub."""
    t = Topology(fs=WT_FS, frame=WT_FRAME, name="watch")
    t.vfos.append(VfoDesc(parent=-1, fs=WT_FS, decimate_count=3, mixer_freq=WT_MAIN_MIXER, demod_usb=False, cstyle=1,
                          samples_per_buffer=WT_FRAME))
    for k, f in enumerate(WT_USB_MIXERS):
        t.vfos.append(VfoDesc(topic=f"W{k:02d}", parent=0, fs=WT_FS // 8, decimate_count=4, mixer_freq=f,
                              late_decimate=WT_LATE if k == 5 else 0, gain=float(np.float32(WT_GAIN)), cstyle=1,
                              samples_per_buffer=WT_FRAME // 8))
    t.vfos.append(VfoDesc(topic="WIQ", parent=0, fs=WT_FS // 8, decimate_count=3, mixer_freq=WT_COMPRESS_MIXER, demod_usb=False,
                          cstyle=1, scalecomp=1, samples_per_buffer=WT_FRAME // 8))
    return t


def band_hz(desc) -> tuple[float, float]:
    """[lo, hi] of a leaf in Hz of its source (for placing a tone and for the overlap rule of the tests)"""
    R = desc.fs / 2 ** desc.decimate_count
    if not desc.demod_usb:
        return -desc.mixer_freq - R / 2, -desc.mixer_freq + R / 2
    R_out = R / desc.late_decimate if desc.late_decimate in (5, 6) else R
    B = min(desc.filter_bw if desc.filter_bw > 0 else R_out / 2, R_out / 2)
    return -desc.mixer_freq, -desc.mixer_freq + B


def tone_for(topo: Topology, leaf: int) -> float:
    """The raw frequency that lands mid-passband of `leaf` (a sub of node 0): its place in the parent's stream, less the
    main's mixer."""
    lo, hi = band_hz(topo.vfos[leaf])
    return (lo + hi) / 2 - topo.vfos[0].mixer_freq


def tone_frame(topo: Topology, raw_hz: float, seed: int, start: int = 0) -> np.ndarray:
    """+-1 LSB of noise plus one tone of amplitude 50"""
    from sdrreceiver_amd import synth
    rng = np.random.default_rng(seed)
    return synth.tone_frame(topo.frame, topo.fs, [(raw_hz, 50.0)], start) + rng.integers(-1, 2, 2 * topo.frame).astype(np.float32)
