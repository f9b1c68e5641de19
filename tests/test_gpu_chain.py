"""The ingest chain as a whole on the device: format conversion, DC-bias removal, ADC meter, impulse blanker, half-band front
stages and rational resampler in one receiver, for eight frames, through every way a frame is handed over, every DC form and the
launch options, with live changes in between.  Per delivered frame the blanker's input, the resampler's input, the raw frame,
every field of the blanker's record and the ADC record are bit for bit tests/chain_ref.py's composed model; the tree behind is
bit for bit the oracle's (exact arithmetic) or a twin receiver's without the stages, each fed the model's raw frame.

The cases, their frames and the wrong launch paths they tell apart are tests/chain_ref.py's; tests/test_chain_model.py shows that
the comparisons here are not vacuous."""
import dataclasses
import functools

import numpy as np
import pytest

import adc_ref as ar
import chain_ref as cr
from helpers import bits
from oracle import binding as ob
from sdrreceiver_amd import blank as bl, ingest, iqbal as iq, notch as nt, shift as sh
from sdrreceiver_amd.receiver import Receiver
from test_gpu_ingest_formats import REL_TOL, _check_tolerance, _check_twin
from test_gpu_parity import _check_exact

pytestmark = pytest.mark.gpu

HANDED_OVER = ["A", "C", "D"]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.size == b.size and np.array_equal(bits(a), bits(b))


def _first_bad(got, want):
    bad = np.flatnonzero(got.view(np.uint64) != np.ascontiguousarray(want).view(np.uint64)) if got.size == want.size else np.zeros(1, int)
    return (got.size, want.size, int(bad.size), int(bad[0]) if bad.size else -1)


def _rx(case, **kw):
    return Receiver.from_topology(case.topo(), **case.receiver_kw(), **kw)


def _leaves(topo):
    return [i for i in range(len(topo.vfos)) if not topo.children(i)]


def _device(arrays):
    import torch
    out = [torch.from_numpy(np.array(v)).cuda() for v in arrays]  # (a copy: the shared frames are read-only)
    torch.cuda.synchronize()
    return out


def _check_records(rx, case, s, cfg, what, adc=True):
    """The records of the delivered frame: they may be read with frames in flight"""
    if case.guard is not None:
        got = rx.blanker
        assert {k: got[k] for k in bl.RECORD_FIELDS} == s.rec, (what, "blanker record", got, s.rec)
        assert got["cfg"] == bl.Cfg(float(np.float32(cfg.ratio)), float(np.float32(cfg.floor)), cfg.rank_q16, cfg.guard), (what, got["cfg"])
    if adc is True:
        got = rx.adc_meter()
        assert got == s.adc, (what, "adc", {k: (got[k], s.adc[k]) for k in s.adc if got[k] != s.adc[k]})
    elif adc is not None:
        assert rx.adc_meter() == adc, (what, "adc")


def _check_stages(rx, case, s, cfg, what, adc=True, blank_in=True):
    """Every stage of the last delivered frame against the model's Step `s` (nothing in flight)"""
    if case.guard is not None and blank_in:
        got = rx.blanker_input()
        assert _same(got, s.blank_in), (what, "blanker input", _first_bad(got, s.blank_in))
    if case.rs:
        got = rx.resampler_input()
        assert got.size == case.n0 and _same(got, s.front_out), (what, "resampler input", _first_bad(got, s.front_out))
    got = rx.raw()
    assert got.size == case.n and _same(got, s.raw), (what, "raw", _first_bad(got, s.raw))
    _check_records(rx, case, s, cfg, what, adc)


def _check_same_tree(rx, twin, topo, what):
    assert rx.published == twin.published and len(rx.published) > 0, (what, "published")
    _check_twin(rx, twin, topo, what)


# ---- 1. every case through process_fmt; case B in the three arithmetics --------------------------------------------------------------
@pytest.mark.parametrize("name,exact", [(k, 1) for k in cr.CASES] + [("B", 0), ("B", 2)])
def test_every_case(name, exact):
    case = cr.CASES[name]
    topo, run = case.topo(), cr.model_run(case)
    rx = _rx(case, exact=exact, keep_streams=True)
    if exact == 1:
        nodes, roots = ob.build_tree("port", topo)
    else:
        twin = Receiver.from_topology(topo, exact=exact, keep_streams=True)
    for f, ((v, fmt), s) in enumerate(zip(cr.frames(case), run)):
        if f and case.cfg(f) != case.cfg(f - 1):
            rx.set_blanker(case.cfg(f))
        rx.process_fmt(v, fmt=fmt, correct_dc=case.correct_dc)
        _check_stages(rx, case, s, case.cfg(f), (name, exact, f))
        assert len(rx.published) == len(_leaves(topo)), (name, f)
        if exact == 1:
            ob.process_roots(roots, np.ascontiguousarray(s.raw).view(np.float32))
            _check_exact(rx, nodes, topo, (name, f))
        else:
            twin.process(s.raw.view(np.float32))
            _check_same_tree(rx, twin, topo, (name, exact, f))
    rx.close()
    if exact != 1:
        twin.close()


# ---- 2. the DC forms in front of blanker, front stage and resampler --------------------------------------------------------------------
@pytest.mark.parametrize("form", [dict(dc_speculative=True), dict(dc_speculative=False), dict(dc_blocks_per_step=1), dict(dc_blocks_per_step=8)],
                         ids=["speculative", "plain", "per_step1", "per_step8"])
def test_the_exact_dc_forms(form):
    case = cr.CASES["B"]
    topo, run = case.topo(), cr.model_run(case)
    rx = _rx(case, keep_streams=True, **form)
    nodes, roots = ob.build_tree("port", topo)
    for f, ((v, fmt), s) in enumerate(zip(cr.frames(case), run)):
        rx.process_fmt(v, fmt=fmt, correct_dc=True)
        _check_stages(rx, case, s, case.cfg(f), (form, f))
        ob.process_roots(roots, np.ascontiguousarray(s.raw).view(np.float32))
        _check_exact(rx, nodes, topo, (form, f))
    rx.close()


def test_the_blocked_scan_in_front_of_the_stages():
    """Option dc_blocked_scan is a tolerance path: the frame it leaves is held to the float64 IIR response within
    test_gpu_ingest_formats.py's bound, and the tree to the oracle fed the model of that response within its _check_tolerance.
    Everything BEHIND the frame it left -- blanker, front stage, resampler, records -- is the model of that very frame, bit for
    bit, and the tree the oracle's."""
    import scipy.signal as sg
    case = cr.CASES["B"]
    topo = case.topo()
    rx = _rx(case, keep_streams=True, keep_prequant=True, dc_blocked_scan=True)
    of_device, of_response = cr.Chain(case), cr.Chain(case)
    nodes, roots = ob.build_tree("port", topo)
    tnodes, troots = ob.build_tree("port", topo)
    A, B = float(np.float32(1.0) - np.float32(0.000001)), float(np.float32(0.000001))
    z = [np.zeros(1), np.zeros(1)]
    for f, (v, fmt) in enumerate(cr.frames(case)):
        rx.process_fmt(v, fmt=fmt, correct_dc=True)
        x = ingest.to_float(v)
        iq = x.copy()
        for comp in (0, 1):
            a, z[comp] = sg.lfilter([B], [1.0, -A], x[comp::2].astype(np.float64), zi=z[comp])
            iq[comp::2] = x[comp::2] - a.astype(np.float32)
        got = rx.blanker_input()
        err = float(np.abs(got - iq.view(np.complex64)).max())
        print(f"frame {f}: max |blanker input - model| {err:.3g}, bound {REL_TOL * float(np.abs(x).max()):.3g}")
        assert got.size == case.in_frame and err <= REL_TOL * float(np.abs(x).max()), (f, err)
        s = of_device.step(v, fmt, converted=got)
        _check_stages(rx, case, s, case.cfg(f), ("blocked", f), blank_in=False)
        assert s.rec["hits"] == cr.model_run(case)[f].rec["hits"]
        ob.process_roots(roots, np.ascontiguousarray(s.raw).view(np.float32))
        _check_exact(rx, nodes, topo, ("blocked", f))
        t = of_response.step(v, fmt, converted=iq.view(np.complex64))
        ob.process_roots(troots, np.ascontiguousarray(t.raw).view(np.float32))
        _check_tolerance(rx, tnodes, topo, ("blocked, the response", f))
    rx.close()


# ---- 3. the ways a frame is handed over ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _published(name) -> tuple:
    """What process_fmt published for each of the case's frames: computed once"""
    case = cr.CASES[name]
    rx = _rx(case)
    out = []
    for v, fmt in cr.frames(case):
        rx.process_fmt(v, fmt=fmt, correct_dc=case.correct_dc)
        out.append(list(rx.published))
    rx.close()
    assert all(len(m) == len(_leaves(case.topo())) for m in out)
    return tuple(out)


@pytest.mark.parametrize("device", [False, True], ids=["submit_fmt", "submit_device_fmt"])
@pytest.mark.parametrize("name", HANDED_OVER)
def test_two_frames_in_flight_over_eight_frames(name, device):
    case = cr.CASES[name]
    run, want, frames = cr.model_run(case), _published(name), cr.frames(case)
    dev = _device([v for v, _ in frames]) if device else None
    rx = _rx(case)

    def submit(k):
        if device:
            rx.submit_device_fmt(dev[k].data_ptr(), case.in_frame, frames[k][1])
        else:
            rx.submit_fmt(frames[k][0], fmt=frames[k][1])

    submit(0)
    submit(1)
    for k in range(cr.N_FRAMES):
        rx.wait()
        assert rx.published == want[k], (name, k, "published")
        _check_records(rx, case, run[k], case.cfg(k), (name, k))
        if k + 2 < cr.N_FRAMES:
            submit(k + 2)
    assert rx.in_flight() == 0
    _check_stages(rx, case, run[-1], case.cfg(cr.N_FRAMES - 1), (name, "last"))
    rx.close()


@pytest.mark.parametrize("name", HANDED_OVER)
def test_six_device_frames_queued_then_two_more(name):
    case = cr.CASES[name]
    run, want, frames = cr.model_run(case), _published(name), cr.frames(case)
    dev = _device([v for v, _ in frames])
    rx = _rx(case)
    for k in range(6):
        rx.process_device_fmt(dev[k].data_ptr(), case.in_frame, frames[k][1])
    rx.fetch()
    assert rx.published == want[5], (name, "published", 5)
    _check_stages(rx, case, run[5], case.cfg(5), (name, 5))
    for k in (6, 7):
        rx.process_device_fmt(dev[k].data_ptr(), case.in_frame, frames[k][1])
    rx.fetch()
    assert rx.published == want[7], (name, "published", 7)
    _check_stages(rx, case, run[7], case.cfg(7), (name, 7))
    rx.close()


@pytest.mark.parametrize("name", HANDED_OVER)
def test_the_same_values_as_cf32(name):
    """Frames 0 .. 3 through process, 4 .. 7 through submit_device with two in flight, in ONE receiver: the states chain across
    the doors.  No frame arrives as integers: the ADC meter has nothing to measure."""
    case = cr.CASES[name]
    run, want, frames = cr.model_run(case), _published(name), cr.frames(case)
    floats = [ingest.to_float(v, fmt) for v, fmt in frames]
    dev = _device(floats)
    rx = _rx(case)
    for k in range(4):
        rx.process(floats[k])
        assert rx.published == want[k], (name, k, "published")
        _check_stages(rx, case, run[k], case.cfg(k), (name, k), adc=ar.unmeasured(k))
    rx.submit_device(dev[4].data_ptr(), case.in_frame)
    rx.submit_device(dev[5].data_ptr(), case.in_frame)
    for k in range(4, cr.N_FRAMES):
        rx.wait()
        assert rx.published == want[k], (name, k, "published")
        _check_records(rx, case, run[k], case.cfg(k), (name, k), adc=ar.unmeasured(k))
        if k + 2 < cr.N_FRAMES:
            rx.submit_device(dev[k + 2].data_ptr(), case.in_frame)
    _check_stages(rx, case, run[-1], case.cfg(cr.N_FRAMES - 1), (name, "last"), adc=ar.unmeasured(cr.N_FRAMES - 1))
    rx.close()


# ---- 4. live changes drain the pipeline and leave the stages' state alone ----------------------------------------------------------------
def test_live_changes_between_staged_frames():
    case = cr.CASES["C"]
    topo, frames = case.topo(), cr.frames(case)
    leaves = _leaves(topo)
    kw = dict(park=True, meter=True, keep_streams=True)
    rx, twin = _rx(case, **kw), Receiver.from_topology(topo, **kw)
    model = cr.Chain(case)
    changed = bl.Cfg(16.0, 0.0, case.cfg().rank_q16, 33)
    assert changed.guard != case.guard and changed.ratio != case.cfg().ratio
    # what is called on both receivers behind frame f
    live = {0: lambda r: r.set_mixer_freqs([1], [float(case.n // 9)]), 1: lambda r: r.set_gains([1], [0.03]), 2: lambda r: r.set_active([2], [0]),
            3: lambda r: r.set_active([2], [1]), 5: lambda r: r.set_active([3], [0]), 6: lambda r: r.set_active([3], [1])}
    hits = 0
    for f, (v, fmt) in enumerate(frames):
        s = model.step(v, fmt)
        if f in (4, 5):  # the frames around set_blanker are submitted and waited for
            rx.submit_fmt(v, fmt=fmt)
            rx.wait()
        else:
            rx.process_fmt(v, fmt=fmt)
        twin.process(s.raw.view(np.float32))
        _check_stages(rx, case, s, model.cfg, ("live", f))
        _check_same_tree(rx, twin, topo, ("live", f))
        a, b = rx.meters(leaves), twin.meters(leaves)
        for key in b:
            assert _same(np.atleast_1d(a[key]), np.atleast_1d(b[key])), (f, key)
        hits += s.rec["hits"]
        if f in live:
            live[f](rx), live[f](twin)
        if f == 4:
            rx.set_blanker(changed)
            model.set_blanker(changed)
    assert hits > 0 and model.st.frame == cr.N_FRAMES
    rx.close()
    twin.close()


# ---- 5. the launch options --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame_pipeline", [True, False])
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("name", ["W", "A"])
def test_launch_options(name, fuse, frame_pipeline):
    case = cr.CASES[name]
    topo, run = case.topo(), cr.model_run(case)
    kw = dict(fuse=fuse, frame_pipeline=frame_pipeline, segments=2, keep_streams=True)
    rx, twin = _rx(case, **kw), Receiver.from_topology(topo, **kw)
    nodes, roots = ob.build_tree("port", topo)
    for f, ((v, fmt), s) in enumerate(zip(cr.frames(case), run)):
        rx.process_fmt(v, fmt=fmt)
        twin.process(s.raw.view(np.float32))
        _check_stages(rx, case, s, case.cfg(f), (name, fuse, frame_pipeline, f))
        _check_same_tree(rx, twin, topo, (name, fuse, frame_pipeline, f))
        ob.process_roots(roots, np.ascontiguousarray(s.raw).view(np.float32))
        _check_exact(rx, nodes, topo, (name, fuse, frame_pipeline, f))
    rx.close()
    twin.close()


# ---- 6. every stage at once: the order of the chain and the route between its buffers ------------------------------------------------
# Case G is case D with every frame twice as long: the smallest geometry in which the canceller's frequency loop can move at all (it
# needs two FULL blocks of 4096 in the tree's frame; notch.step).  B's tree frame is shorter than a block and D's is exactly one, so
# their records are held to the model with `coherent` = `adapted` = 0 in every tone, and G is where a tone is followed.
SIX_G = cr.Case("G", (ingest.CS16,), 16448, 64, False, 1, 7, (256, 257, 8, 8224, 8192), 8224, 8192)
SIX_CASES = {"B": cr.CASES["B"], "D": cr.CASES["D"], "G": SIX_G, "E": cr.CASES["E"]}
SIX_FRAMES = 4
SIX_TONE = 171234567.25  # the steady tone at the tree's rate, in increment units (about 0.04 cycles a sample)
SIX_OFF = 55924          # ... and how far beside it the canceller is told to look: 0.33 rad a block, 20 Hz at 1.536 MS/s
SIX_NOISE, SIX_AMPL = 512, 5120  # CS16 codes: sigma of the noise per component, the tone's amplitude -- ten times the noise
SIX_ICFG = iq.Cfg(0.25, 0.0, 0.03, 1.1)
SIX_NCFG = nt.Cfg((int(SIX_TONE) - SIX_OFF, (-(1 << 30)) & nt.M32), 0.5, 1.0, 0.5, 4 * SIX_OFF)
SIX_PATHS = ["exact_dc", "blocked_dc", "no_dc", "cf32"]
# KIND_INGEST launches (event brackets) a frame, read from a run of this test on commit 75b0f6f ("Demodulation blocks: stage sample
# pairs with bounded loads, no branches"), the parent of the commit that gave the chain one launch function: one bracket encloses
# the format conversion (or the DC form's kernels) and all six stages, on every path and for real input too.
SIX_INGEST_LAUNCHES = {"exact_dc": 1, "blocked_dc": 1, "no_dc": 1, "cf32": 1, "real": 1}


def _six_shift(case):
    return sh.Cfg(sh.inc_of(4.0 * case.n, -123.4), 0xFEDCBA98)


@functools.lru_cache(maxsize=None)
def six_frames(name) -> tuple:
    """((samples, fmt), ...) of four frames, read-only.  B, D, G: CS16 noise around a DC offset, chain_ref's pulse plan (pulses of
    +-100 dongle LSB, which the blanker takes out) and one steady tone that lands on SIX_TONE at the tree's rate -- the front stage
    halves its frequency's denominator, the resampler multiplies it by M / L --, phase-continuous across the frames.  E: the
    case's own full-range real frames."""
    case = SIX_CASES[name]
    if case.real:
        return cr.frames(case)[:SIX_FRAMES]
    n, (L, M) = case.in_frame, case.rs[:2]
    rng = np.random.default_rng(6600 + n)
    turns = SIX_TONE / 4294967296.0 * L / M / 2 ** case.stages  # cycles per input sample
    out = []
    for f, starts in enumerate(cr.pulse_plan(n, case.guard)[:SIX_FRAMES]):
        j = np.arange(f * n, (f + 1) * n, dtype=np.float64)
        tone = SIX_AMPL * np.exp(2j * np.pi * ((turns * j) % 1.0))
        v = np.rint(rng.standard_normal(2 * n) * SIX_NOISE + np.tile([3.0, -2.0], n) * 256)
        v[0::2] += np.rint(tone.real)
        v[1::2] += np.rint(tone.imag)
        for s in starts:
            v[2 * s: 2 * (s + cr.PULSE_LEN)] = rng.choice([-100, 100], size=2 * cr.PULSE_LEN) * 256
        v = np.clip(v, -32768, 32767).astype(np.int16)
        v.setflags(write=False)
        out.append((v, ingest.CS16))
    return tuple(out)


SixStep = dataclasses.make_dataclass("SixStep", ["chain", "irec", "nrec", "srec", "raw"])


class AllSix:
    """chain_ref's composition with the IQ balance in front of it and the spur canceller and the shift behind: the state of one
    receiver across frames"""

    def __init__(self, case):
        self.case, self.chain = case, cr.Chain(case)
        self.dc = np.zeros(2, np.float32)
        self.ist, self.nst, self.sst = iq.State.initial(SIX_ICFG), nt.State.initial(SIX_NCFG), sh.State.initial(_six_shift(case))

    def balanced(self, v, fmt, correct_dc):
        """The frame behind the conversion, the exact DC-bias removal and the IQ balance: what the blanker reads"""
        iqf = ingest.to_float(v, fmt)
        if correct_dc:
            ob.dc_correct(iqf, self.dc)
        return iq.correct(iqf.view(np.complex64), self.ist.c, self.ist.d)

    def step(self, v, fmt, balanced=None) -> SixStep:
        """One frame.  `balanced`: the frame as it left the IQ balance (the statistics of the stage are of what it produced, so its
        record and its next pair follow from that frame alone); None: real input, which has no such stage"""
        irec = None
        if balanced is not None:
            st, n = self.ist, balanced.size
            sums = iq.sums(balanced)
            r = iq.step(sums, n, SIX_ICFG, st.c, st.d)
            irec = {"frame": st.frame, "n_complex": n, "measured": r["measured"], "adapted": r["adapted"], "rejected": r["rejected"],
                    "c_bits": iq.bits(st.c), "d_bits": iq.bits(st.d), "next_c_bits": iq.bits(r["c"]), "next_d_bits": iq.bits(r["d"]), **sums}
            self.ist = iq.State(r["c"], r["d"], st.frame + 1)
        s = self.chain.step(v, fmt, converted=balanced)
        y, nrec, self.nst = nt.apply(s.raw, SIX_NCFG, self.nst)
        w, srec, self.sst = sh.apply(y, self.sst)
        return SixStep(s, irec, nrec, srec, w)


@functools.lru_cache(maxsize=None)
def six_model(name, correct_dc=False) -> tuple:
    """The SixSteps of a case's frames under the exact DC-bias removal or none: computed once"""
    case, m = SIX_CASES[name], AllSix(SIX_CASES[name])
    return tuple(m.step(v, fmt, None if case.real else m.balanced(v, fmt, correct_dc)) for v, fmt in six_frames(name))


def _six_rx(case, **kw):
    args = dict(case.receiver_kw(), notch=SIX_NCFG, shift=_six_shift(case), keep_streams=True, **kw)
    if not case.real:
        args.update(iq_balance=SIX_ICFG)
    rx = Receiver.from_topology(case.topo(), **args)
    rx.enable_kernel_timing(True)
    return rx


def _check_six(rx, case, t, what):
    """Every stage of the last delivered frame against the SixStep `t`"""
    s = t.chain
    if case.guard is not None:
        got = rx.blanker_input()
        assert _same(got, s.blank_in), (what, "blanker input", _first_bad(got, s.blank_in))
        got = rx.blanker
        assert {k: got[k] for k in bl.RECORD_FIELDS} == s.rec, (what, "blanker record", got, s.rec)
        got = rx.iq_balance
        assert {k: got[k] for k in iq.RECORD_FIELDS} == t.irec, (what, "IQ record", got, t.irec)
    got = rx.resampler_input()
    assert got.size == case.n0 and _same(got, s.front_out), (what, "resampler input", _first_bad(got, s.front_out))
    got = rx.raw()
    assert got.size == case.n and _same(got, t.raw), (what, "raw", _first_bad(got, t.raw))
    assert nt.record_key(rx.notch) == nt.record_key(t.nrec), (what, "notch record", rx.notch, t.nrec)
    assert {k: rx.shift[k] for k in sh.RECORD_FIELDS} == t.srec, (what, "shift record", rx.shift, t.srec)


def _ingest_launches(rx):
    return rx.kernel_times().get("k_ingest", {"launches": 0})["launches"]


@pytest.mark.parametrize("path", SIX_PATHS)
@pytest.mark.parametrize("name", ["B", "D", "G"])
def test_all_six_stages(name, path):
    """IQ balance, blanker, front stage, resampler, spur canceller and shift in one receiver, four frames with a steady tone ten
    times the noise, through process_fmt with the exact DC-bias removal, with the blocked one, with none, and as cf32 frames of
    the same values: the blanker's and the resampler's input, the four records and the tree's raw frame are bit for bit the composed
    models', the tree the oracle's, and a frame is one KIND_INGEST bracket.

    The blocked DC form is a tolerance path (test_the_blocked_scan_in_front_of_the_stages): the frame the IQ balance left is held
    to the model of the float64 IIR response within REL_TOL of the largest sample times the largest gain the stage can have
    (|c| + |d| <= MAX_C + MAX_D: Q' = c I + d Q), and everything behind it is the model of that very frame, bit for bit.

    A tone can only be followed where the tree's frame has two full blocks: that is case G, where the canceller's record shows
    it coherent and adapted; in B (2048 samples) and D (4096) the model itself never sets either flag, and the device agrees."""
    import scipy.signal as sg
    case = SIX_CASES[name]
    topo, frames = case.topo(), six_frames(name)
    dc = path in ("exact_dc", "blocked_dc")
    rx = _six_rx(case, dc_blocked_scan=path == "blocked_dc")
    nodes, roots = ob.build_tree("port", topo)
    model = AllSix(case) if path == "blocked_dc" else None
    A, B = float(np.float32(1.0) - np.float32(0.000001)), float(np.float32(0.000001))
    z = [np.zeros(1), np.zeros(1)]
    hits = 0
    for f, (v, fmt) in enumerate(frames):
        if path == "cf32":
            rx.process(ingest.to_float(v, fmt))
        else:
            rx.process_fmt(v, fmt=fmt, correct_dc=dc)
        if model:
            x = ingest.to_float(v, fmt)
            resp = x.copy()
            for comp in (0, 1):
                a, z[comp] = sg.lfilter([B], [1.0, -A], x[comp::2].astype(np.float64), zi=z[comp])
                resp[comp::2] = x[comp::2] - a.astype(np.float32)
            want = iq.correct(resp.view(np.complex64), model.ist.c, model.ist.d)
            got = rx.blanker_input()
            err, bound = float(np.abs(got - want).max()), REL_TOL * float(np.abs(x).max()) * (iq.MAX_C + iq.MAX_D)
            print(f"frame {f}: max |blanker input - model| {err:.3g}, bound {bound:.3g}")
            assert got.size == case.in_frame and err <= bound, (f, err, bound)
            t = model.step(v, fmt, got)
        else:
            t = six_model(name, dc)[f]
        _check_six(rx, case, t, (name, path, f))
        assert t.srec["n_complex"] == t.nrec["n_complex"] == case.n != case.in_frame
        assert _ingest_launches(rx) == SIX_INGEST_LAUNCHES[path] * (f + 1), (name, path, f, rx.kernel_times())
        ob.process_roots(roots, np.ascontiguousarray(t.raw).view(np.float32))
        _check_exact(rx, nodes, topo, (name, path, f))
        hits += t.chain.rec["hits"]
    tones = t.nrec["tones"]
    assert hits and t.irec["adapted"] and tones[0]["a_re_bits"] | tones[0]["a_im_bits"]  # every stage did something
    if name == "G":
        assert tones[0]["coherent"] and tones[0]["adapted"] and tones[0]["inc_next"] != SIX_NCFG.inc0[0], tones[0]
    else:
        assert not any(k["coherent"] or k["adapted"] for k in tones)
    rx.close()


def test_all_six_stages_real_input():
    """Case E -- RS16 and RU12 frames into a real first front stage, two complex ones, the resampler 5/3 -- with the spur canceller and
    the shift behind it: the chain as real input runs it (no IQ balance and no blanker can sit in front of a real first stage)"""
    case = SIX_CASES["E"]
    topo = case.topo()
    rx = _six_rx(case)
    nodes, roots = ob.build_tree("port", topo)
    for f, ((v, fmt), t) in enumerate(zip(six_frames("E"), six_model("E"))):
        rx.process_fmt(v, fmt=fmt)
        _check_six(rx, case, t, ("E", f))
        assert _ingest_launches(rx) == SIX_INGEST_LAUNCHES["real"] * (f + 1), (f, rx.kernel_times())
        ob.process_roots(roots, np.ascontiguousarray(t.raw).view(np.float32))
        _check_exact(rx, nodes, topo, ("E", f))
    rx.close()


# ---- 7. the C++ host layer: sdrx_demo with all three stages in one run --------------------------------------------------------------------
def test_demo_with_front_stage_resampler_and_blanker(tmp_path):
    import os
    import subprocess
    from test_topology import INI_25E_LIKE
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    demo = os.path.join(root, "host", "sdrx_demo")
    subprocess.check_call(["make", "-C", os.path.join(root, "host")], stdout=subprocess.DEVNULL)
    profile = tmp_path / "profile.ini"
    profile.write_text(INI_25E_LIKE)
    staged = [demo, str(profile), "--frames", "3", "--format", "cs16", "--input-rate", "2400000", "--front-stages", "2", "--front-taps", "7"]
    plain = subprocess.check_output(staged, text=True).splitlines()
    assert plain[0].startswith("resampler ") and plain[1].startswith("front ") and len(plain) > 2
    # a floor nothing reaches: the same lines, and a record per frame whose references chain
    lines = subprocess.check_output(staged + ["--blanker", "1,64,3e38,1"], text=True).splitlines()
    recs = [ln.split() for ln in lines if ln.startswith("blanker ")]
    assert [ln for ln in lines if not ln.startswith("blanker ")] == plain and len(recs) == 3
    assert recs[0][1:4] == ["0", f"{bl.INF_BITS:08x}", "-1"] and all(r[5:] == ["0", "0", "0", "0"] for r in recs)
    for f in (1, 2):
        assert recs[f][1] == str(f) and recs[f][3] == recs[f - 1][4] and recs[f][2] == f"{bl.thr_bits(np.float32(3e38)):08x}"
