"""The output-meter definition (sdrreceiver_amd/meter.py) on hand-built cases, suggest_gains, and the C ABI of
sdrx_get_meters / sdrx_group_get_meters.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sdrreceiver_amd import meter
from sdrreceiver_amd.topology import VfoDesc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USB = VfoDesc(demod_usb=True)


def _usb(pre):
    pre = np.asarray(pre, np.float32)
    return meter.meters_from_payload(USB, meter.wrap_int16(pre), pre)


def test_int16_wrap_boundary():
    pre = np.array([32767.9, 32768.0, -32768.9, -32769.0], np.float32)
    v = meter.wrap_int16(pre)
    assert v.tolist() == [32767, -32768, -32768, 32767]  # the last two: -32768 in range, -32769 wraps to +32767
    for p, clipped in zip(pre, [0, 1, 0, 1]):
        assert _usb([p])["clipped"] == clipped, p
    m = _usb(pre)
    assert m["clipped"] == 2 and m["n_values"] == 4
    assert m["peak"] == np.float32(32769.0)
    assert m["sum_sq"] == 32767 ** 2 * 2 + 32768 ** 2 * 2


def test_far_out_of_range_and_nan():
    pre = np.array([1e12, -1e12, np.inf, -np.inf, 65536.0 * 32768.0], np.float32)
    m = _usb(pre)
    assert m["clipped"] == 5 and m["peak"] == np.inf
    assert meter.wrap_int16(pre).tolist() == [0, 0, 0, 0, 0]  # INT32_MIN's low 16 bits
    m = _usb(np.array([1.0, np.nan, -3.0], np.float32))
    assert m["clipped"] == 1 and np.isnan(m["peak"])
    assert m["sum_sq"] == 1 + 0 + 9


def test_sum_is_exact_past_32_bits():
    pre = np.full(100000, -32768.0, np.float32)
    m = _usb(pre)
    assert m["sum_sq"] == 100000 * 2 ** 30 and m["clipped"] == 0
    assert m["sum_sq"] > 2 ** 32


@pytest.mark.parametrize("cstyle,scalecomp", [(0, 1), (1, 1), (1, 4)])
def test_int8_boundary(cstyle, scalecomp):
    d = VfoDesc(demod_usb=False, cstyle=cstyle, scalecomp=scalecomp)
    s = scalecomp / 128.0
    # pre of (127.99, -128.99): in range; 128 and -129: wrapped
    re = np.array([127.99, -128.99, 128.0, 1.0, 0.5], np.float64) * s
    im = np.array([1.0, 2.0, 3.0, -129.0, 0.25], np.float64) * s
    z = (re + 1j * im).astype(np.complex64)
    m = meter.meters_from_payload(d, None, z)
    assert m["n_values"] == 10
    assert m["clipped"] == 2
    pre_re, pre_im = meter.iq_prequant(d, z)
    v = np.concatenate([meter.wrap_int8(pre_re), meter.wrap_int8(pre_im)]).astype(np.int64)
    assert v[2] == -128 and v[5 + 3] == 127  # 128 -> -128, -129 -> 127
    assert m["sum_sq"] == int((v * v).sum())
    assert m["peak"] == np.float32(np.abs(np.concatenate([pre_re, pre_im])).max())
    if cstyle == 0:  # the payload holds v itself
        pay = np.stack([meter.wrap_int8(pre_re), meter.wrap_int8(pre_im)], 1).reshape(-1)
        assert meter.meters_from_payload(d, pay)["sum_sq"] == m["sum_sq"]


def test_cstyle1_needs_the_stream():
    with pytest.raises(ValueError):
        meter.meters_from_payload(VfoDesc(demod_usb=False, cstyle=1), np.zeros(4, np.int8))


def _meters(sum_sq, n, clipped, usb):
    recs = []
    for s, k, c in zip(sum_sq, n, clipped):
        r = type("R", (), {})()
        r.frame, r.sum_sq, r.n_values, r.clipped, r.peak = 0, s, k, c, 0.0
        recs.append(r)
    return meter.meters_dict(recs, usb)


def test_suggest_gains():
    n = 1000
    rms = np.array([3276.8, 3276.8 * 10 ** (-20 / 20), 0.5, 3276.8, 1000.0, 100.0])  # -20 dBFS, -40, silent, ..
    m = _meters([int(round(r * r * n)) for r in rms], [n] * 6, [0, 0, 0, 5, 0, 0], [1, 1, 1, 1, 0, 1])
    g = np.array([0.05, 0.05, 0.05, 0.05, 0.05, 0.02], np.float32)
    out = meter.suggest_gains(g, m, target_rms_dbfs=-18.0)
    assert out.dtype == np.float32
    assert np.isclose(out[0], g[0] * 10 ** (2 / 20), rtol=1e-5)  # +2 dB
    assert out[1] == np.float32(np.float64(g[1]) * 10 ** (6 / 20))  # +22 dB wanted, capped at +6
    assert out[2] == g[2]                                    # silent: kept
    assert out[3] == g[3]                                    # wrapped: never raised
    assert out[4] == g[4]                                    # compress() leaf: untouched
    assert out[5] > g[5]
    down = meter.suggest_gains(g, m, target_rms_dbfs=-40.0, max_step_db=3.0)
    assert down[0] == np.float32(np.float64(g[0]) * 10 ** (-3 / 20)) and down[3] < g[3]
    with pytest.raises(TypeError):
        meter.suggest_gains(g, m)  # no default target: nobody has measured JAERO's green light


def test_meters_dict_dbfs():
    m = _meters([32768 ** 2 * 10], [10], [0], [1])
    assert m["rms_dbfs"][0] == 0.0 and m["full_scale"][0] == 32768.0


def test_library_exports_meter_symbols():
    from sdrreceiver_amd import _lib
    L = _lib.lib()
    for name in ("sdrx_get_meters", "sdrx_group_get_meters"):
        assert hasattr(L, name), name
    assert C.sizeof(_lib.MeterC) == 32 and _lib.MeterC.peak.offset == 24
    assert L.sdrx_get_meters(None, None, 0, None) == _lib.SDRX_EINVAL


def test_c99_snippet_compiles(tmp_path):
    src = tmp_path / "m.c"
    src.write_text("""#include "sdrx.h"
#include <stddef.h>
_Static_assert(sizeof(sdrx_meter) == 32, "sdrx_meter layout");
_Static_assert(offsetof(sdrx_meter, peak) == 24, "sdrx_meter layout");
int use(sdrx_ctx *c, sdrx_group *g) {
    int ids[2] = {2, 3};
    sdrx_meter m[2];
    int rc = sdrx_get_meters(c, ids, 2, m);
    return rc ? rc : sdrx_group_get_meters(g, ids, 2, m) + (int)m[0].clipped + (int)m[1].n_values;
}
""")
    cc = next((c for c in ("cc", "gcc", "clang") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    if cc is None:
        pytest.fail("no C compiler")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(tmp_path / "m.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
