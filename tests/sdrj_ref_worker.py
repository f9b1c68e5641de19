"""Worker of oracle/binding.py sdrj_run: ONE stream through the real sdrj (oracle/_ref/libsdrjref*.so) in a process of
its own.  sdrj::demodData keeps its DC estimate in a function-static variable (sdrj.cpp:280) that lives once per loaded
library and cannot be reset, so every stream that must start from the zero state needs a fresh process.

    python sdrj_ref_worker.py <library> <in.npz> <out.npz>

in.npz:  u8 (dongle bytes) or f32 (interleaved floats); frames (complex samples per demodData call); dc (0/1);
         topic (the string handed to fftVFOSlot after construction); topo (optional: a sdrreceiver_amd.topology function
         name whose tree is built on the same library's vfo and attached as sdrj's main VFOs).
out.npz: lut (the 256 floats of sdr::floats); samples (sdrj::samples of every call, concatenated, complex64);
         fft_calls, fft_len, fft_data (every fftData emission: its 1-based call index since fftVFOSlot, its length, its
         contents concatenated); with topo: v<i>_stream / v<i>_usb per call as f<k>_v<i>_stream / f<k>_v<i>_usb.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import binding as ob  # noqa: E402


def main(lib_path, in_path, out_path):
    a = np.load(in_path)
    kind = "sdrj_ofast" if os.path.basename(lib_path) == os.path.basename(ob.SDRJ_OFAST_SO) else "sdrj"
    L = ob.load(kind)
    assert os.path.samefile(L.lib._name, lib_path), (L.lib._name, lib_path)
    f = L.lib
    h = f.sdrjh_new()
    nodes = []
    if "topo" in a.files:
        from sdrreceiver_amd import topology as tp
        topo = getattr(tp, str(a["topo"]))()
        nodes, roots = ob.build_tree(kind, topo)
        for r in roots:
            r._owned = False  # ~sdrj deletes its main VFOs; the process ends without deleting sdrj
            f.sdrjh_add_root(h, r.h)
    f.sdrjh_set_dc_correction(h, int(a["dc"]))
    f.sdrjh_fft_vfo_slot(h, str(a["topic"]).encode())

    lut = np.zeros(256, np.float32)
    f.sdrjh_bytes_to_floats(h, np.arange(256, dtype=np.uint8).ctypes.data, 256, lut.ctypes.data)
    if "u8" in a.files:
        u8 = np.ascontiguousarray(a["u8"], np.uint8)
        data = np.zeros(u8.size, np.float32)
        f.sdrjh_bytes_to_floats(h, u8.ctypes.data, u8.size, data.ctypes.data)  # the real floats.at() for every byte
    else:
        data = np.ascontiguousarray(a["f32"], np.float32)
    frames = [int(n) for n in a["frames"]]
    assert 2 * sum(frames) == data.size, (sum(frames), data.size)

    out = {"lut": lut}
    samples = np.zeros(sum(frames), np.complex64)
    pos = 0
    for k, n in enumerate(frames):
        f.sdrjh_demod(h, data[2 * pos:].ctypes.data, 2 * n)
        got = f.sdrjh_get_samples(h, samples[pos:].ctypes.data, n)
        assert got == n, (got, n)
        pos += n
        for i, v in enumerate(nodes):
            out[f"f{k}_v{i}_stream"] = v.stream()
            if not v.children:
                out[f"f{k}_v{i}_usb"] = v.usb()
    out["samples"] = samples
    m = f.sdrjh_fft_count(h)
    out["fft_calls"] = np.array([f.sdrjh_fft_call(h, k) for k in range(m)], np.int64)
    lens = [f.sdrjh_fft_get(h, k, None, 0) for k in range(m)]
    fft = np.zeros(sum(lens), np.complex64)
    p = 0
    for k in range(m):
        f.sdrjh_fft_get(h, k, fft[p:].ctypes.data, lens[k])
        p += lens[k]
    out["fft_len"] = np.array(lens, np.int64)
    out["fft_data"] = fft
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(*sys.argv[1:4])
