"""The expected spectrum display of every node of the lattice trees (tests/lattice.py) and of the seeded random trees
(tests/live_ref.py) under their schedules of live controls (test infrastructure; no GPU, no fixtures).

Nothing here comes from the device: a node's display is spectrum_ref.Display (pinned bit for bit to the real kiss_fft by
tests/test_spectrum_oracle.py) fed the MODEL stream of that node -- live_ref.ModelTree, pinned to the plain-C oracle by
tests/test_live_model.py and tests/test_lattice_model.py -- frame by frame, a frame without a stream (a parked leaf) skipped.

* :func:`displays` -- that, for any list of model frames; :func:`lattice_displays`, :func:`random_displays` the shared runs.
* :func:`raw_display` -- the raw frame at sdrj's every-4th-call cadence.
* :func:`tap_plan` -- the leaves that keep no stream under a set of options (include/sdrx.h: "fuse_late", "fuse_demod",
  "keep_streams"), split into those a test taps and the one it leaves alone.
* :func:`cells` -- what a tree's nodes cover as (layout, level, size class); tests/test_spectrum_trees_model.py asserts the
  union over the lattice and over the seeds, and that the reference alone can tell a wrong kernel from a right one."""
from __future__ import annotations

import functools

import numpy as np

import lattice as lt
import live_ref as lr
import spectrum_ref as sr

SEEDS = tuple(range(20))  # every residue of test_gpu_live_random._options' rotation (periods 2, 3, 4, 5 and 7 drift apart)
CHUNK = 1024
LATE_TAPS = {5: 49, 6: 73}    # vfo::init's design at every rate: 53 L (L - 1) / 22, made odd (LateGeom<L>::kTaps)
LATE_CHUNK = lt.LATE_CHUNK    # the shortest leaf frame the fused late decimation takes
DEMOD_MAX_LPF = 64            # "an audio low-pass of at most 64 taps"


class State:
    """One display state as tests/test_gpu_spectrum.py::check reads it."""

    __slots__ = ("updates", "bins", "pwr", "maxval", "aveval")

    def __init__(self, d: sr.Display | None = None):
        if d is None:
            d = sr.Display()
        self.updates, self.maxval, self.aveval = d.updates, d.maxval, d.aveval
        self.bins, self.pwr = d.bins.copy(), d.pwr.copy()
        self.bins.setflags(write=False)
        self.pwr.setflags(write=False)

    @property
    def smooth(self) -> np.ndarray:
        p, k = self.pwr, sr.N - 10
        return (p[4:k + 4] + p[3:k + 3] + p[2:k + 2] + p[1:k + 1] + p[:k]) / 5


ZERO = State()  # an enabled spectrum that never had a stream


def displays(want, n_nodes, fed=None) -> tuple:
    """states[f][i]: the display of node i after frame f of the model run `want` (the records of ModelTree.process).  A frame
    whose want[f]["streams"][i] is None -- the leaf is parked -- or for which fed(f, i) is false -- a leaf without a stream
    buffer that is not tapped -- is no update: the state is the one before, the same object."""
    disp = [sr.Display() for _ in range(n_nodes)]
    last = [ZERO] * n_nodes
    out = []
    for f, w in enumerate(want):
        for i in range(n_nodes):
            z = w["streams"][i]
            if z is None or (fed is not None and not fed(f, i)):
                continue
            disp[i].update(z)
            last[i] = State(disp[i])
        out.append(tuple(last))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def lattice_displays(name) -> tuple:
    """:func:`displays` of lattice tree `name` under lattice.schedule.  Computed once and shared: nobody writes into it."""
    want, _ = lt.model_frames(name)
    return displays(want, len(lt.trees()[name].vfos))


@functools.lru_cache(maxsize=None)
def random_displays(seed) -> tuple:
    """:func:`displays` of live_ref.reference(seed), for the seeds of :data:`SEEDS`."""
    topo, _, _, want, _, _ = lr.reference(seed)
    return displays(want, len(topo.vfos))


@functools.lru_cache(maxsize=None)
def lattice_plain_displays(name) -> tuple:
    """The states after the LAST frame without the schedule, on the plain-C oracle's streams (lattice.oracle_frames): what frames
    queued back to back, with no call between them to drain the software pipeline, must give."""
    return displays([dict(streams=[s.stream() for s in snaps]) for snaps in lt.oracle_frames(name)], len(lt.trees()[name].vfos))[-1]


@functools.lru_cache(maxsize=None)
def catchup_displays(key) -> tuple:
    """:func:`displays` of catchup_ref.reference_lattice(key) for a tree's name, of catchup_ref.reference_random(key) for a
    seed: a caught-up leaf's stream of frame K-1 is in no frame's record, so its display counts the frames from K on."""
    import catchup_ref as cr
    ref = cr.reference_lattice(key) if isinstance(key, str) else cr.reference_random(key)
    return displays(ref[3], len(ref[0].vfos))


def raw_display(frames) -> tuple:
    """states[f] of SDRX_SPECTRUM_RAW enabled before frame 0: the raw frame on the calls of spectrum_ref.raw_update_calls."""
    calls = sr.raw_update_calls(len(frames))
    d, last, out = sr.Display(), ZERO, []
    for f, iq in enumerate(frames):
        if f + 1 in calls:
            d.update(np.ascontiguousarray(iq, np.float32).reshape(-1).view(np.complex64))
            last = State(d)
        out.append(last)
    return tuple(out)


# ---- which leaves keep no stream ----------------------------------------------------------------------------------------------
def keeps_no_stream(topo, i, opts) -> bool:
    """include/sdrx.h, options "fuse_late" (default 1), "fuse_demod" (default 0) and "keep_streams" (default 0): a USB leaf
    below a parent with decimate_count 0 and late_decimate 5 | 6 writes only its decimated stream; with fuse_demod a USB leaf
    below a parent with decimate_count 2, no late decimation and an audio low-pass of at most 64 taps (none included) on a
    frame of at least one chunk writes only its payload.  keep_streams keeps decimate[d] of both."""
    d = topo.vfos[i]
    if opts.get("keep_streams", False) or topo.children(i) or not d.demod_usb or d.parent < 0:
        return False
    if d.late_decimate:
        return bool(opts.get("fuse_late", True)) and d.decimate_count == 0 and d.late_decimate in LATE_TAPS and \
            d.samples_per_buffer >= LATE_CHUNK[d.late_decimate]
    return bool(opts.get("fuse_demod", False)) and d.decimate_count == 2 and lt.lpf_taps(d) <= DEMOD_MAX_LPF and \
        d.samples_per_buffer >= CHUNK


def tap_plan(topo, opts) -> dict:
    """{"tapped": [...], "untapped": [...]} over the leaves of :func:`keeps_no_stream`, in id order (the first one tapped gets
    the arena's tap buffer, every further one a buffer of its own).  Of two or more the last stays untapped; a single one is
    tapped when its id is odd.  A tapped leaf has a stream in every frame in which it is active; the untapped one never has."""
    ids = [i for i in range(len(topo.vfos)) if keeps_no_stream(topo, i, opts)]
    if len(ids) >= 2:
        return dict(tapped=ids[:-1], untapped=ids[-1:])
    if len(ids) == 1 and ids[0] % 2 == 0:
        return dict(tapped=[], untapped=ids)
    return dict(tapped=ids, untapped=[])


# ---- what a tree covers -------------------------------------------------------------------------------------------------------
def stream_len(topo, i) -> int:
    d = topo.vfos[i]
    return d.samples_per_buffer >> d.decimate_count


def size_class(n) -> str:
    if n < 256:
        return "<256"
    if n < CHUNK:
        return "<1024"
    if n < sr.N:
        return "partial" if n % CHUNK else "full"
    return "=8192" if n == sr.N else ">8192"


def cell(topo, i) -> tuple:
    """(layout, level, size class) of node i: a node with children keeps its stream in tile layout, a leaf in natural order."""
    return ("tiled" if topo.children(i) else "natural", lt.level(topo, i), size_class(stream_len(topo, i)))


def cells(topo) -> set:
    return {cell(topo, i) for i in range(len(topo.vfos))}


def _cells(layout, level, *classes) -> set:
    return {(layout, level, c) for c in classes}


LATTICE_CELLS = (_cells("natural", 0, "<256", "<1024", "partial", ">8192") |
                 _cells("natural", 1, "<256", "<1024", "partial", "full", ">8192") |
                 _cells("natural", 2, "<256", "<1024", "full") |
                 _cells("tiled", 0, "partial", "full", "=8192", ">8192") |
                 _cells("tiled", 1, "full"))
RANDOM_ADDS = _cells("tiled", 1, "<1024", "partial", ">8192") | _cells("natural", 2, "partial", ">8192")


# ---- the tile layout, for the model test ---------------------------------------------------------------------------------------
def tiled(x) -> np.ndarray:
    """The buffer of an inner node's stream: whole 1024-sample tiles (the last one zero-filled), unit (chunk, i2, lane) =
    samples 16 lane + 2 i2, +1 (sdrx_get_stream's un-tiling, inverted)."""
    x = np.asarray(x, np.complex64).reshape(-1)
    g = np.arange(x.size)
    ch, r = g >> 10, g & 1023
    ln, i = r >> 4, r & 15
    buf = np.zeros((x.size + CHUNK - 1) // CHUNK * CHUNK, np.complex64)
    buf[ch * 1024 + (i >> 1) * 128 + ln * 2 + (i & 1)] = x
    return buf


def at_floor(bins) -> bool:
    """Every 100000 |bin| / 8192 <= 1: the update adds 0 dB to every pwr entry, and only the bins test anything."""
    re, im = bins.real.astype(np.float32), bins.imag.astype(np.float32)
    val = np.sqrt(im * im + re * re).astype(np.float64)
    return bool((100000.0 * np.abs((1.0 / sr.N) * val) <= 1).all())
