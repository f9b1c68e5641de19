"""The channel watch without a GPU: the ABI additions, the band of a leaf (product against model), the segment rule, and the
sign and placement of the band pinned to the oracle -- the tone that the oracle's sub k hears is the tone the model finds in
sub k's band of the parent's spectrum."""
import ctypes as C
import dataclasses
import glob
import os
import re

import numpy as np
import pytest

import lattice
import watch_ref as wr
from helpers import SAMPLE_INI
from sdrreceiver_amd import _lib, topology as tp, watch
from sdrreceiver_amd.topology import VfoDesc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sdrx_set_watch", "sdrx_get_watch", "sdrx_get_watch_psd", "sdrx_group_set_watch", "sdrx_group_get_watch",
               "sdrx_group_get_watch_psd"]


def test_abi_additions():
    hdr = open(os.path.join(ROOT, "include", "sdrx.h")).read()
    declared = set(re.findall(r"\b(sdrx_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
    assert L.sdrx_abi_version() == 5
    assert "SDRX_WATCH_MAX_SEGMENTS 16" in hdr
    assert C.sizeof(_lib.WatchLevelC) == 48
    assert _lib.WatchLevelC.band_pwr.offset == 8 and _lib.WatchLevelC.first_bin.offset == 24 and _lib.WatchLevelC.watched.offset == 36


def _leaves(topo):
    return [i for i in range(len(topo.vfos)) if not topo.children(i)]


def test_band_lattice_trees():
    n = 0
    for name, topo in lattice.trees().items():
        for i in _leaves(topo):
            assert watch.band(topo.vfos[i]) == wr.band(topo.vfos[i]), (name, i, topo.vfos[i])
            n += 1
    assert n > 100


def test_band_sample_inis():
    files = sorted(glob.glob(os.path.join(SAMPLE_INI, "*.ini")))
    assert len(files) >= 5
    for path in files:
        topo = tp.topology_from_ini(open(path).read(), name=os.path.basename(path))
        for i in _leaves(topo):
            fb, nb = watch.band(topo.vfos[i])
            assert (fb, nb) == wr.band(topo.vfos[i]), (path, i)
            assert 0 <= fb < 8192 and 1 <= nb <= 8192


def _usb(fs, d, f, bw=0, late=0):
    return VfoDesc(parent=0, fs=fs, decimate_count=d, mixer_freq=f, filter_bw=bw, late_decimate=late, samples_per_buffer=fs // 4)


EDGE = {
    # a band that wraps bin 8191 -> 0: [-f, -f + B] = [-100, 1820] at 7.5 Hz per bin: bins -13 .. 242
    "wrap": (_usb(61440, 4, 100.0), (8192 - 13, 256)),
    # 57 Hz on a 1.536 MS/s parent (187.5 Hz per bin): ceil(0) = 0, floor(0.304) = 0
    "one_bin": (_usb(1536000, 5, 0.0, bw=57), (0, 1)),
    # 57 Hz between two bins: k_hi < k_lo, clamped to one bin
    "one_bin_clamped": (_usb(1536000, 5, -20.0, bw=57), (1, 1)),
    # a compress leaf at d = 0 hears its whole source
    "all_bins": (VfoDesc(parent=0, fs=61440, decimate_count=0, mixer_freq=3000.0, demod_usb=False, samples_per_buffer=15360), None),
    # a mixer beyond fs/2 aliases: f = fs/2 + 4 321 is the band of f - fs
    "beyond_nyquist": (_usb(61440, 3, 61440 // 2 + 4321.0), None),
    "non_integer": (_usb(61440, 2, 1234.625, bw=2000), None),
    "late6": (_usb(288000, 0, 54578.0, bw=10000, late=6), None),
    "late5_cap": (_usb(240000, 2, -74731.0, bw=30000, late=5), None),  # the filter is wider than R_out / 2: capped
}


@pytest.mark.parametrize("case", sorted(EDGE))
def test_band_edge_cases(case):
    d, want = EDGE[case]
    got = watch.band(d)
    assert got == wr.band(d), (case, got, wr.band(d))
    if want is not None:
        assert got == want, (case, got)
    if case == "all_bins":
        assert got[1] == 8192
        lv = {"band_pwr": [5.0], "total_pwr": [5.0], "n_bins": [8192], "watched": [1]}
        assert np.isnan(watch.contrast(lv)[0])
    if case == "beyond_nyquist":
        assert got == watch.band(dataclasses.replace(d, mixer_freq=d.mixer_freq - d.fs))
    if case == "late5_cap":
        assert got[1] == wr.band(dataclasses.replace(d, filter_bw=0))[1]


SEG_N = [256, 8191, 8192, 8193, 3 * 8192 + 5, 16 * 8192, 17 * 8192 + 1]


@pytest.mark.parametrize("n", SEG_N)
def test_segments(n):
    S, starts = wr.segments(n)
    assert S == {256: 1, 8191: 1, 8192: 1, 8193: 1, 3 * 8192 + 5: 3, 16 * 8192: 16, 17 * 8192 + 1: 16}[n]
    assert starts == [s * (n // S) for s in range(S)] and starts[0] == 0
    assert starts[-1] + min(8192, n) <= n  # the last segment ends inside the frame
    rng = np.random.default_rng(n)
    x = (rng.integers(-8, 9, n) + 1j * rng.integers(-8, 9, n)).astype(np.complex64)
    p = wr.psd(x)
    assert p.dtype == np.float64 and p.shape == (8192,) and (p >= 0).all()
    if n < 8192:  # the zero-padded case equals an explicit pad
        padded = np.zeros(8192, np.complex64)
        padded[:n] = x
        assert np.array_equal(p, wr.psd(padded))
    want = np.zeros(8192, np.float64)
    for st in starts:  # the sequential double sum, written out
        want += wr.segment_power(x[st:st + min(8192, n)]).astype(np.float64)
    assert np.array_equal(p, want)


def test_wake_list_and_contrast():
    lv = {"band_pwr": np.array([90.0, 1.0, 90.0]), "total_pwr": np.array([100.0, 100.0, 100.0]), "n_bins": np.array([8, 8, 8]),
          "watched": np.array([1, 1, 0])}
    c = watch.contrast(lv)
    assert c[0] == (90.0 / 8) / (10.0 / 8184) and c[1] == (1.0 / 8) / (99.0 / 8184)
    assert watch.wake_list([7, 8, 9], lv, 100.0) == [7]  # 9 reaches the contrast but was not watched


def test_sign_and_placement_against_the_oracle():
    """One tone of amplitude 50 over +-1 LSB of noise, at the raw frequency that lands mid-passband of sub k of
    watch_ref.watch_tree (8 USB subs, node 6 with late_decimate 5, and a compress sub): the oracle's sub with the largest audio
    sum_sq is k, the model's band_pwr on the ORACLE's parent stream is largest for k, and k's contrast is at least 100 x that
    of every sub whose band does not overlap k's.  Measured here: the oracle's sum_sq of sub k is >= 5 700 x the next sub's,
    the model's contrast of sub k >= 3.5e9 x the next one's (the compress sub included) -- room to spare over 100."""
    from oracle import binding as ob
    topo = wr.watch_tree()
    subs = list(range(1, 10))
    bands = {i: watch.band(topo.vfos[i]) for i in subs}
    hz = {i: wr.band_hz(topo.vfos[i]) for i in subs}
    for k in range(1, 9):
        nodes, roots = ob.build_tree("port", topo)
        ob.process_roots(roots, wr.tone_frame(topo, wr.tone_for(topo, k), seed=40 + k))
        audio = {i: nodes[i].usb() for i in range(1, 9)}
        assert max(int(np.abs(a.astype(np.int32)).max()) for a in audio.values()) < 32000  # (no int16 wrapped)
        sum_sq = {i: int((a.astype(np.int64) ** 2).sum()) for i, a in audio.items()}
        assert max(sum_sq, key=sum_sq.get) == k, (k, sum_sq)
        p = wr.psd(nodes[0].stream().view(np.complex64))
        lv = {i: wr.levels(p, *bands[i]) for i in subs}
        assert max(subs, key=lambda i: lv[i][0]) == k, (k, lv)
        con = {i: wr.contrast(lv[i][0], lv[i][1], bands[i][1]) for i in subs}
        for i in subs:
            if i != k and (hz[i][1] < hz[k][0] or hz[i][0] > hz[k][1]):
                assert con[k] >= 100 * con[i], (k, i, con)
        # the product's helper agrees with the model's formula
        d = {"band_pwr": [lv[k][0]], "total_pwr": [lv[k][1]], "n_bins": [bands[k][1]], "watched": [1]}
        assert watch.contrast(d)[0] == con[k]
