"""The spectrum display's restatement (tests/spectrum_ref.py) pinned to the REAL kiss_fft and to a C++ restatement of
fftHandlerSlot's power step (tests/golden/spectrum.npz, written by tests/golden/make_spectrum_golden.py), and the C ABI of
sdrx_set_spectrum / sdrx_get_spectrum / sdrx_get_spectrum_levels.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spectrum_ref as sr
from sdrreceiver_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "spectrum.npz"))


def test_fixture_records_its_provenance(g):
    p = str(g["provenance"])
    assert "kiss_fft.c sha256" in p and "gcc -O2" in p
    assert list(g["case_names"]) == ["noise", "tone", "carrier", "zeros", "short"]


def test_hann_table_is_bit_exact(g):
    assert np.array_equal(sr.hann().view(np.uint32), g["hann"].view(np.uint32))


@pytest.fixture(scope="module")
def inputs():
    return sr.fixture_cases()


@pytest.mark.parametrize("case", ["noise", "tone", "carrier", "zeros", "short"])
def test_windowed_input_and_fft_equal_the_real_kiss_fft(g, inputs, case):
    x = inputs[case]
    assert x.size == int(g[f"{case}_len"]) and sr.sha256(x) == str(g[f"{case}_x_sha256"]), "input generator drifted"
    inr = sr.windowed(x)
    assert sr.sha256(inr) == str(g[f"{case}_inr_sha256"])
    out = sr.kiss_fft(inr)
    assert np.array_equal(out[::64].copy().view(np.uint32), g[f"{case}_out_every64"].view(np.uint32)), case
    assert sr.sha256(out) == str(g[f"{case}_out_sha256"]), case


def test_digit_reversed_positions_are_a_permutation():
    pos = sr.digit_reversed_positions()
    assert np.array_equal(np.sort(pos), np.arange(sr.N))
    assert pos[1] == 2048 and pos[4096] == 1 and pos[4] == 512


def test_power_step_over_eight_updates(g):
    seq = sr.fixture_sequence()
    assert sr.sha256(seq) == str(g["seq_x_sha256"]), "input generator drifted"
    d = sr.Display()
    for f in range(8):
        d.update(seq[f])
        assert np.abs(d.pwr[f::8] - g["seq_pwr"][f]).max() <= 1e-9, f
        assert np.abs(d.smooth[f::8][:1022] - g["seq_smooth"][f]).max() <= 1e-9, f
        assert abs(d.maxval - g["seq_maxval"][f]) <= 1e-9 and abs(d.aveval - g["seq_aveval"][f]) <= 1e-9, f
    assert np.abs(d.pwr - g["seq_pwr_last"]).max() <= 1e-9
    assert d.updates == 8


def test_raw_cadence_matches_the_real_sdrj():
    dc = np.load(os.path.join(GOLDEN, "dc_reference.npz"))
    rids = [k[: -len("_fft_calls")] for k in dc.files if k.endswith("_fft_calls")]
    assert len(rids) >= 10
    for rid in rids:
        assert sr.raw_update_calls(int(dc[f"{rid}_frames"])) == [int(c) for c in dc[f"{rid}_fft_calls"]], rid
    assert sr.raw_update_calls(13) == [5, 9, 13]


def test_library_exports_the_spectrum_abi():
    L = _lib.lib()
    for name in ("sdrx_set_spectrum", "sdrx_get_spectrum", "sdrx_get_spectrum_levels"):
        assert hasattr(L, name) and name in _lib.SYMBOLS, name
    hdr = open(os.path.join(ROOT, "include", "sdrx.h")).read()
    assert int(re.search(r"#define SDRX_SPECTRUM_BINS (\d+)", hdr).group(1)) == _lib.SPECTRUM_BINS == sr.N
    assert int(re.search(r"#define SDRX_SPECTRUM_RAW \((-\d+)\)", hdr).group(1)) == _lib.SPECTRUM_RAW
    assert L.sdrx_abi_version() == 5


def test_spectrum_info_layout_matches_header():
    S = _lib.SpectrumInfoC
    assert C.sizeof(S) == 32
    assert (S.updates.offset, S.n_in.offset, S.reserved.offset, S.maxval.offset, S.aveval.offset) == (0, 8, 12, 16, 24)


def test_spectrum_calls_reject_a_null_context():
    L = _lib.lib()
    info = _lib.SpectrumInfoC()
    assert L.sdrx_set_spectrum(None, 0, 1) == _lib.SDRX_EINVAL
    assert L.sdrx_get_spectrum(None, 0, C.byref(info), None, None, None) == _lib.SDRX_EINVAL
    assert L.sdrx_get_spectrum_levels(None, None, 0, None, None, None) == _lib.SDRX_EINVAL
