"""How a demodulation block (demod_block, sdrreceiver_amd/csrc/demod.hip) brings its window of the leaf stream into LDS: in
16-byte sample pairs through a bounded load, without a test per sample.  Every case is the smallest tree that reaches the
staging code at one of its edges -- one main VFO (d = 1) and USB leaves of depth 4 to 8 below it, so a leaf frame can have any
length -- run for three consecutive frames from the zero state in both launch forms: sdrx_process (the kernel k_usb_demod)
and frames queued on the device and flushed with sdrx_fetch (the demodulation blocks inside k_levels_tail, the form bench.py
times).  The last quarter of every input frame is twelve times larger than the rest: a history prefix taken from the wrong
place shows.  The exact arithmetic is held to the oracle bit for bit, the tolerance and the robust arithmetic to the suite's
rule (pre-quantisation floats within 1e-5 of max|ref|, int16 within one LSB).

Leaf lengths: one below, at and one above a block's tile without the audio low-pass (1 024) and with the 47-tap one (976), and
a little above two tiles (2 054 and 1 957: a last block of 6 and 5 outputs).  The odd lengths put the frame's end in the middle of
a pair.
Low-pass lengths: firfilter's design only ever has an odd number of taps, so of 0, 29, 46, 47, 48 and 61 the even ones cannot be
reached: 45 and 49 stand in for 46 and 48.  E is then always N + 1 and the low-pass shift `soff` only ever 0 (no low-pass) or 3.
255 taps is the longest low-pass a block applies itself (kMaxFir = 256).
A plan whose stream is not 16-byte aligned or whose window starts on an odd sample cannot be made through the API (the history
and the tile are derived, the arena hands out 256-byte multiples), so the finalize-time check has no test of its own."""
import numpy as np
import pytest

from oracle import binding as ob
from sdrreceiver_amd import synth, topology as tp

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5  # north_star: "within 1e-5 relative float tolerance"
N_FRAMES = 3
ARITH = {"exact": 1, "tolerance": 0, "robust": 2}


def _bw_for(rate, taps):
    """an integer filter_bw for which firfilter::low_pass(2, rate, bw, bw / 4) has `taps` taps (firfilter.cpp:108-119)"""
    for bw in range(1, rate // 2 + 1):
        n = int(53.0 * rate / (22.0 * (bw / 4.0)))
        if (n | 1) == taps:
            return bw
    raise AssertionError(f"no filter_bw gives {taps} taps at {rate} S/s")


def _frame_ok(n):
    """what sdrx_finalize asks of a VFO's input frame: whole 16-sample runs, no last chunk shorter than 256 samples"""
    return n % 16 == 0 and (n % 1024 == 0 or n % 1024 >= 256)


def _tree(n_out, lpfs):
    """main VFO (d = 1, no demodulation) over one USB leaf of `n_out` samples a frame per entry of `lpfs` (taps, 0 = none); the
    leaves' depth is the smallest (4 .. 8) at which sdrx_finalize accepts both frames: the smallest frame for this length"""
    from sdrreceiver_amd.topology import Topology, VfoDesc, _g
    leaf_d = next(d for d in range(4, 9) if _frame_ok(n_out << d) and _frame_ok(2 * (n_out << d)))
    n_leaf_in = n_out << leaf_d
    frame, fs = 2 * n_leaf_in, 32 * n_leaf_in
    t = Topology(fs=fs, frame=frame, name=f"staging-{n_out}")
    t.vfos.append(VfoDesc(parent=-1, fs=fs, decimate_count=1, mixer_freq=float(fs // 11), demod_usb=False, cstyle=1, samples_per_buffer=frame))
    rate = (fs // 2) >> leaf_d
    for k, taps in enumerate(lpfs):
        t.vfos.append(VfoDesc(topic=f"S{k:02d}", parent=0, fs=fs // 2, decimate_count=leaf_d, mixer_freq=float((fs // 2) // (7 + 2 * k)),
                              demod_usb=True, filter_bw=_bw_for(rate, taps) if taps else 0, gain=_g(0.003), cstyle=1,
                              samples_per_buffer=n_leaf_in))
    return t


CASES = {f"n{n}": (n, (0, 47)) for n in (975, 976, 977, 1023, 1024, 1025, 1957, 2054)}
CASES["lpf-short"] = (1500, (29, 45, 49))
CASES["lpf-long"] = (1500, (61, 255))

_ref = {}


def _reference(case):
    """(topology, input frames, per frame and leaf: int16 payload and pre-quantisation doubles of the oracle), computed once"""
    if case not in _ref:
        n_out, lpfs = CASES[case]
        topo = _tree(n_out, lpfs)
        nodes, roots = ob.build_tree("port", topo)
        for i, taps in enumerate(lpfs):
            assert nodes[1 + i].taps("fir_usb").size == taps, (case, i)
        lcg = synth.Lcg(77)
        frames, want = [], []
        for f in range(N_FRAMES):
            iq = synth.lcg_frame(topo.frame, lcg)
            iq[2 * (topo.frame - topo.frame // 4):] *= 12.0
            frames.append(iq)
            ob.process_roots(roots, iq)
            want.append({i: (nodes[i].usb(), nodes[i].usb_prequant()) for i in range(1, len(topo.vfos))})
        for w in want:
            for a in w.values():
                a[0].setflags(write=False)
                a[1].setflags(write=False)
        _ref[case] = (topo, frames, want)
    return _ref[case]


def _check(rx, want, arith, ctx):
    for i, (pay, pre_ref) in want.items():
        got = rx.output(i)
        assert got.size == pay.size, (ctx, i)
        if arith == "exact":
            assert np.array_equal(got, pay), (ctx, i, "payload", np.flatnonzero(got != pay)[:8])
        else:
            pre = rx.prequant(i).astype(np.float64)
            s = float(np.abs(pre_ref).max())
            assert np.abs(pre - pre_ref).max() <= REL_TOL * s, (ctx, i, "prequant", np.abs(pre - pre_ref).max() / s)
            assert np.abs(got.astype(np.int32) - pay.astype(np.int32)).max() <= 1, (ctx, i, "payload")


def _demod_launches(rx):
    return rx.kernel_times().get("k_usb_demod", {"launches": 0})["launches"]


@pytest.mark.parametrize("arith", sorted(ARITH))
@pytest.mark.parametrize("case", sorted(CASES))
def test_blocks_of_k_usb_demod(case, arith):
    """sdrx_process: every frame runs through launches of its own, the demodulation in k_usb_demod"""
    from sdrreceiver_amd.receiver import Receiver
    topo, frames, want = _reference(case)
    rx = Receiver.from_topology(topo, exact=ARITH[arith], keep_prequant=arith != "exact")
    rx.enable_kernel_timing(True)
    for f, iq in enumerate(frames):
        rx.process(iq)
        _check(rx, want[f], arith, (case, arith, "frame", f))
    assert _demod_launches(rx) == N_FRAMES
    rx.close()


@pytest.mark.parametrize("arith", sorted(ARITH))
@pytest.mark.parametrize("case", sorted(CASES))
def test_blocks_inside_k_levels_tail(case, arith):
    """frames queued on the device: the demodulation blocks ride in the next step's launch, no k_usb_demod at all; a fetch
    after frame 0 (no history) and one after frame 2 (history across two frame boundaries)"""
    import torch
    from sdrreceiver_amd.receiver import Receiver
    topo, frames, want = _reference(case)
    dev = [torch.from_numpy(iq).cuda() for iq in frames]
    torch.cuda.synchronize()
    rx = Receiver.from_topology(topo, exact=ARITH[arith], keep_prequant=arith != "exact")
    rx.enable_kernel_timing(True)
    for f, d in enumerate(dev):
        rx.process_device(d.data_ptr(), topo.frame)
        if f in (0, N_FRAMES - 1):
            rx.fetch()
            _check(rx, want[f], arith, (case, arith, "queued frame", f))
    assert _demod_launches(rx) == 0
    rx.close()
