"""The integer sample formats (include/sdrx.h SDRX_FMT_*, sdrreceiver_amd/ingest.py) on the host: the table, the two
embeddings of dongle bytes that pin the signed formats to the real reference through the committed fixtures, and the
declarations.  No GPU needed."""
import os
import re

import numpy as np
import pytest

from helpers import DC_REFERENCE_REGIMES, dc_reference_bytes
from oracle import binding as ob
from sdrreceiver_amd import _lib, ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the regimes of tests/golden/dc_reference.npz that tests/test_gpu_ingest_formats.py feeds as int8 / int16
EMBEDDED_REGIMES = ("lcg", "capture480", "const0", "step")
NEW_SYMBOLS = ("sdrx_process_fmt", "sdrx_submit_fmt", "sdrx_process_device_fmt", "sdrx_submit_device_fmt", "sdrx_group_process_fmt",
               "sdrx_group_submit_fmt")


def embed_s8(b):
    """Bytes <= 254 as the int8 samples of the same value: v = b - 127."""
    assert int(np.max(b)) <= 254
    return (np.asarray(b).astype(np.int16) - 127).astype(np.int8)


def embed_s16(b):
    """Bytes <= 254 as the int16 samples of the same value: v = 256 (b - 127)."""
    assert int(np.max(b)) <= 254
    return ((np.asarray(b).astype(np.int32) - 127) * 256).astype(np.int16)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "sdrx.h")).read()
    for name, value in (("CU8", ingest.CU8), ("CS8", ingest.CS8), ("CS16", ingest.CS16)):
        assert re.search(rf"#define SDRX_FMT_{name} {value}\b", hdr), name
    assert (ingest.CU8, ingest.CS8, ingest.CS16) == (0, 1, 2)


def test_cu8_is_the_oracles_lut():
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(bits(ingest.to_float(b, ingest.CU8)), bits(ob.u8_to_float(b)))
    assert np.array_equal(bits(ingest.to_float(b)), bits(ob.u8_to_float(b)))  # (inferred from the dtype)


def test_the_two_embeddings_give_the_bytes_floats():
    b = np.arange(255, dtype=np.uint8)  # 0 .. 254: byte 255 (sample 128) has no image in either signed format
    want = bits(ob.u8_to_float(b))
    assert np.array_equal(bits(ingest.to_float(embed_s8(b), ingest.CS8)), want)
    assert np.array_equal(bits(ingest.to_float(embed_s16(b), ingest.CS16)), want)


def test_cs16_range_and_exact_scaling():
    v = np.array([-32768, 32767, 1, -1, 255, 256], np.int16)
    x = ingest.to_float(v)
    assert x.dtype == np.float32
    assert x[0] == np.float32(-128.0) and x[1] == np.float32(127.99609375)
    assert np.array_equal(x.astype(np.float64) * 256.0, v.astype(np.float64))  # exact: nothing was rounded
    full = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    assert np.array_equal(ingest.to_float(full).astype(np.float64) * 256.0, full.astype(np.float64))
    s8 = np.arange(-128, 128, dtype=np.int16).astype(np.int8)
    assert np.array_equal(ingest.to_float(s8).astype(np.int32), s8.astype(np.int32))


@pytest.mark.parametrize("rid", EMBEDDED_REGIMES)
def test_embedded_regimes_hold_no_byte_255(rid):
    """The condition the embeddings rest on, asserted for every regime the GPU file uses."""
    assert rid in DC_REFERENCE_REGIMES
    assert max(int(b.max()) for b in dc_reference_bytes(rid)) <= 254


def test_the_six_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sdrx.h")).read()
    declared = set(re.findall(r"\b(sdrx_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert _lib.SYMBOLS[name][1] == [_lib.C.c_void_p, _lib.C.c_void_p, _lib.C.c_int, _lib.C.c_int, _lib.C.c_int], name
        assert hasattr(_lib.lib(), name), name
    assert _lib.lib().sdrx_abi_version() == 5


class _FakeLib:
    """Records the one ABI call a wrapper method makes."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _wrapper(cls):
    w = cls.__new__(cls)
    w.L, w.h, w.published = _FakeLib(), None, []
    return w


@pytest.mark.parametrize("kind", ["Receiver", "Group"])
def test_process_fmt_infers_the_format_from_the_dtype(kind):
    from sdrreceiver_amd import receiver
    symbol = {"Receiver": "sdrx_{}_fmt", "Group": "sdrx_group_{}_fmt"}[kind]
    for dtype, fmt in ((np.uint8, ingest.CU8), (np.int8, ingest.CS8), (np.int16, ingest.CS16)):
        for verb in ("process", "submit"):
            w = _wrapper(getattr(receiver, kind))
            a = np.zeros(64, dtype)
            getattr(w, verb + "_fmt")(a, correct_dc=True)
            (name, args), = w.L.calls
            assert name == symbol.format(verb)
            assert args[1:] == (a.ctypes.data, 32, fmt, 1) or args[2:] == (32, fmt, 1), (name, args)
    w = _wrapper(getattr(receiver, kind))
    for bad in (np.zeros(64, np.float32), np.zeros(64, np.int32), np.zeros(64, np.uint16), [1, 2, 3, 4]):
        with pytest.raises(TypeError):
            w.process_fmt(bad)
    with pytest.raises(TypeError):
        w.process_fmt(np.zeros(64, np.int8), fmt=ingest.CS16)  # (the array is not what the format takes)
    with pytest.raises(ValueError):
        w.process_fmt(np.zeros(64, np.int8), fmt=3)
    assert w.L.calls == []
    w.process_fmt(np.zeros(64, np.int16), fmt=ingest.CS16)
    assert w.L.calls[0][1][3] == ingest.CS16
