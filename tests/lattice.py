"""A deterministic lattice of small trees over the decimation depths and tree positions the random trees never draw
(test infrastructure; no GPU, no fixtures).

helpers.random_topology stops at d = 4 for leaves and d = 2 for inner nodes, divides by 1, 2 or 4 in compress() and mixes with
integers inside Nyquist.  :func:`trees` returns named topologies that hold, by construction, every cell of

* USB leaves at d = 0 .. 8 below a tiled parent, some with the audio low-pass (one of at most 64 taps at d = 2 for fuse_demod,
  one each at d = 5, 6 and 8), on leaf frames whose last 1024-chunk holds 256, 512, 768 and 1024 samples;
* d = 5 leaves -- the shaped body that pairs its chunks -- on parent streams of 3, 4, 5 and 8 full chunks, each with and
  without a partial last chunk (3 072, 3 840, 4 096, 4 352, 5 120, 5 376, 8 192, 8 704 samples);
* inner nodes at d = 4, 5, 6 at level 0 and at level 1, each with a USB child and an IQ child; level-2 leaves at d = 5 and 6;
* the /5 and /6 late decimation behind d = 1, 3, 5, 6, 7, 8, parent-less and below a parent, and at d = 0 below a parent on
  leaf frames of 2, 3 and 5 late-chunks (960 / 1 008 samples) and of 2 400 samples (2.5 / 2.38 chunks);
* IQ leaves at d = 5 .. 8 below a parent with cstyle 0 and 1 and scalecomp 1, 3, 5, 7, 10 and 100;
* mixer frequencies 0, +-(fs/2 - 1), a non-integer one (eighths) and one beyond Nyquist (fs/2 + 4 321: sdrx_check_vfo sets
  no bound on the mixer, and the oscillator table of fs entries simply aliases it).

:func:`cells` names what one tree covers as (position, depth, kind) triples, derived from the descriptors alone;
tests/test_lattice_model.py asserts that the union is the list above (:func:`required_cells`) plus the by-products that
:func:`incidental_cells` names, no more and no less.

Geometry: every root has fs = 4 x frame (the table wraps inside 5 frames), every fs and frame is a
multiple of 16, n_in % 2^d == 0, node fs >= 1024, last chunk >= 256 samples, child frame = parent frame >> d, and for a late
leaf (n_in >> d) % L == 0 == (fs >> d) % L.  Root frames stay <= 65 536 samples and trees <= 40 nodes.

Input (:func:`frames`): synth.lcg_frame noise plus one tone of 20 LSB inside the passband of every deep leaf (total decimation >= 8),
its raw frequency walked up the mixer chain.  USB gains are set so that no int16 wraps (asserted by the model tests): a
wrapped sample would turn the 1 LSB bar of the tolerance arithmetics into 65 535."""
from __future__ import annotations

import functools

import numpy as np

from sdrreceiver_amd import synth
from sdrreceiver_amd.topology import Topology, VfoDesc, _g

TONE_AMP = 20.0
N_FRAMES = 5
SCALECOMPS = (1, 3, 5, 7, 10, 100)
D5_FRAMES = {3072: 4, 3840: 4, 4096: 4, 4352: 2, 5120: 3, 5376: 3, 8192: 3, 8704: 2}  # leaf frame -> the main's depth
LATE_CHUNK = {5: 960, 6: 1008}  # the fused late decimation's walk (LateGeom)
LATE0_FRAMES = (1920, 2880, 4800, 2016, 3024, 5040, 2400)  # 2, 3, 5 chunks of 960; of 1008; 2.5 / 2.38 chunks


class _Build:
    def __init__(self, name, frame):
        self.t = Topology(fs=4 * frame, frame=frame, name=name)
        self.k = 0

    def _io(self, parent):
        if parent < 0:
            return self.t.fs, self.t.frame
        p = self.t.vfos[parent]
        return p.out_rate_stage, p.n_stage_out

    def _mixer(self, fs):
        """Inside +-0.3 fs (the parent's half-band passband), integers, golden-ratio spread so that no two siblings share one."""
        self.k += 1
        return float(int(((self.k * 0.6180339887) % 1.0 - 0.5) * 0.6 * fs) + 37)

    def _add(self, parent, d, mixer, **kw):
        fs, n = self._io(parent)
        assert n % (1 << d) == 0 and fs % 16 == 0 and n % 16 == 0 and fs >= 1024 and n <= fs, (self.t.name, parent, d, fs, n)
        assert n % 1024 == 0 or n % 1024 >= 256, (self.t.name, n)
        self.t.vfos.append(VfoDesc(parent=parent, fs=fs, decimate_count=d, mixer_freq=self._mixer(fs) if mixer is None else float(mixer),
                                   samples_per_buffer=n, **kw))
        return len(self.t.vfos) - 1

    def inner(self, parent, d, mixer=None):
        return self._add(parent, d, mixer, demod_usb=False, cstyle=1)

    def usb(self, parent, d, late=0, bw=0, mixer=None):
        fs, n = self._io(parent)
        if late:
            assert (n >> d) % late == 0 and (fs >> d) % late == 0, (self.t.name, parent, d, late)
        gain = 0.01  # (set by _finish once the tree's tones are known)
        return self._add(parent, d, mixer, topic=f"U{len(self.t.vfos):03d}", late_decimate=late, filter_bw=bw, gain=gain, cstyle=1)

    def iq(self, parent, d, cstyle, scalecomp=1, mixer=None):
        return self._add(parent, d, mixer, topic=f"Q{len(self.t.vfos):03d}", demod_usb=False, cstyle=cstyle, scalecomp=scalecomp)


def _sub_tree(n_leaf, dp, full):
    b = _Build(f"sub-{n_leaf}", n_leaf << dp)
    m = b.inner(-1, dp)
    rate = lambda d: (b.t.vfos[m].out_rate_stage >> d)  # noqa: E731
    b.usb(m, 5)
    b.usb(m, 5, bw=int(rate(5) / 4.8))
    if full:
        for d in (0, 1, 2, 3, 4, 6, 7, 8):
            b.usb(m, d)
        b.usb(m, 2, bw=int(rate(2) / 4.8))  # 47 taps: demodulates in the wave under fuse_demod
        b.usb(m, 6, bw=int(rate(6) / 4.8))
        b.usb(m, 8, bw=int(rate(8) / 4.8))
    else:
        b.usb(m, 6 + (n_leaf // 256) % 3)
    return b.t


def _iq_leaves(b, m):
    for d, cs, sc in ((5, 0, 1), (5, 1, 3), (6, 0, 1), (6, 1, 5), (7, 0, 1), (7, 1, 7), (8, 0, 1), (8, 1, 10), (5, 1, 100), (6, 1, 1)):
        b.iq(m, d, cs, sc)


def _freq_tree():
    """Below a d = 0 main (its stream is the whole band, so a tone next to Nyquist still reaches the leaf)."""
    b = _Build("freq", 8704)
    m = b.inner(-1, 0, mixer=0.0)
    fs = b.t.fs
    b.usb(m, 5, mixer=0.0)
    b.usb(m, 6, mixer=fs // 2 - 1)
    b.iq(m, 5, 1, 1, mixer=-(fs // 2 - 1))
    b.usb(m, 7, mixer=1234.625)
    b.usb(m, 2, mixer=-4001.375)
    b.usb(m, 8, mixer=fs // 2 + 4321)
    return b.t


def _inner_tree():
    b = _Build("inner", 65536)
    m0 = b.inner(-1, 0)
    a = b.inner(m0, 4)          # level 1, 4 096 samples at 16 384 S/s
    b.usb(a, 5)                 # level-2 leaves
    b.usb(a, 6)
    b.iq(a, 2, 1, 3)
    c = b.inner(m0, 5)
    b.usb(c, 1)
    b.iq(c, 3, 0)
    e = b.inner(m0, 6)          # 1 024 samples at 4 096 S/s
    b.usb(e, 2)
    b.iq(e, 0, 1, 7)
    for d in (4, 5, 6):         # level 0
        m = b.inner(-1, d)
        b.usb(m, 2)
        b.iq(m, 1, d % 2, 5)
    return b.t


def _late_deep_tree():
    b = _Build("late-deep", 61440)
    for d in (1, 3, 5, 6, 7, 8):
        for L in (5, 6):
            b.usb(-1, d, late=L, bw=(b.t.fs >> d) // L // 5 if d in (1, 6) else 0)
    m = b.inner(-1, 4)  # 3 840 samples at 15 360 S/s: 60, 30, 15 outputs at d = 6, 7, 8
    for d in (1, 3, 5, 6, 7, 8):
        for L in (5, 6):
            if (3840 >> d) % L == 0:
                b.usb(m, d, late=L, bw=(15360 >> d) // L // 5 if d == 3 else 0)
    m = b.inner(-1, 3)  # 7 680 samples: 30 outputs at d = 8, the /6 that 3 840 cannot carry
    b.usb(m, 8, late=6)
    b.usb(m, 8, late=5)
    return b.t


def _late0_tree(n_leaf):
    b = _Build(f"late0-{n_leaf}", 2 * n_leaf)
    m = b.inner(-1, 1)
    for L, chunk in LATE_CHUNK.items():
        if n_leaf % chunk == 0 or n_leaf == 2400:
            b.usb(m, 0, late=L)
            b.usb(m, 0, late=L, bw=(4 * n_leaf) // L // 5)
    b.usb(m, 5 if n_leaf % 32 == 0 else 4)
    return b.t


def _deep_long_tree():
    """32 chunks per leaf frame: room for several segments behind the 2 550-sample warm-up of a d = 8 leaf."""
    b = _Build("deep-long", 65536)
    m = b.inner(-1, 1)
    for d in (6, 7, 8):
        b.usb(m, d)
    b.usb(m, 7, bw=int((b.t.vfos[m].out_rate_stage >> 7) / 4.8))
    b.iq(m, 8, 1, 3)
    b.iq(m, 6, 0)
    return b.t


def _finish(t):
    """USB gains for an int16 peak of about 8 000 within N_FRAMES frames.  A tone of 20 LSB demodulates to 40; the late
    decimation's and the audio low-pass's designs have gain 2 each; a leaf that is not narrow hears its share of the tree's
    other tones; a leaf whose N_FRAMES frames end before the 62-sample delay line (plus half the audio low-pass) has filled shows only
    the leading edge of its 125-tap Hilbert transformer, about a fortieth of the tone."""
    n_tones = len(tones(t))
    for d in t.vfos:
        if d.demod_usb:
            late = d.late_decimate or 1
            est = 2.0 * TONE_AMP * (2 if d.late_decimate else 1) * (2 if d.filter_bw else 1) * max(1.0, n_tones / ((1 << d.decimate_count) * late))
            if d.n_out * N_FRAMES <= 62 + lpf_taps(d) // 2:
                est /= 40.0
            d.gain = _g(8000.0 / 32768.0 / est)


@functools.lru_cache(maxsize=None)
def _trees():
    out = {}
    for n_leaf, dp in D5_FRAMES.items():
        out[f"sub-{n_leaf}"] = _sub_tree(n_leaf, dp, full=n_leaf in (3840, 8704))
    t = out["sub-3840"]  # the widest tree: the IQ leaves live here too
    b = _Build(t.name, t.frame)
    b.t, b.k = t, len(t.vfos)
    _iq_leaves(b, 0)
    for t in (_freq_tree(), _inner_tree(), _late_deep_tree(), _deep_long_tree()):
        out[t.name] = t
    for n_leaf in LATE0_FRAMES:
        out[f"late0-{n_leaf}"] = _late0_tree(n_leaf)
    for t in out.values():
        _finish(t)
        assert len(t.vfos) <= 40 and t.frame <= 65536, t.name
    return out


def trees() -> dict:
    """name -> Topology.  The objects are shared: nobody writes into them."""
    return dict(_trees())


WIDEST = "sub-3840"
LATE_TREES = ("late-deep",) + tuple(f"late0-{n}" for n in LATE0_FRAMES)


# ---- what a tree covers -------------------------------------------------------------------------------------------------------
def level(topo, i) -> int:
    n = 0
    while topo.vfos[i].parent >= 0:
        i = topo.vfos[i].parent
        n += 1
    return n


def _ancestors(topo, i) -> list:
    out = []
    while topo.vfos[i].parent >= 0:
        i = topo.vfos[i].parent
        out.append(i)
    return out


def lpf_taps(d) -> int:
    """The audio low-pass's length: a Hamming design (53 dB) with a transition width of filter_bw / 4 at the output rate, made
    odd.  Plain arithmetic, so that this module needs no built library; tests/test_lattice_model.py holds it to the oracle's
    tap sets."""
    if not (d.demod_usb and d.filter_bw > 0):
        return 0
    return int(53.0 * d.output_rate / (22.0 * (d.filter_bw / 4))) | 1


def cells(topo) -> set:
    """(position, depth, kind) of everything in `topo`.  position: "root" (a parent-less leaf), "sub" (a leaf below a main),
    "level2", "inner0", "inner1", "any".  kind, for a leaf: usb, usb_lpf, usb_lpf<=64, late5, late6, iq0, iq1; for a leaf below
    a main also lastchunk:<n> (depth None), pair:<full chunks>+<partial> (d = 5 USB), late<L>:chunks=<n> (d = 0); for an inner
    node "usb+iq children"; and with position "any", depth None: scalecomp:<n> (cstyle 1) and freq:<class>."""
    out = set()
    for i, d in enumerate(topo.vfos):
        lv, ch = level(topo, i), topo.children(i)
        if ch:
            kinds = {("usb" if topo.vfos[c].demod_usb else "iq") for c in ch if not topo.children(c)}
            if kinds >= {"usb", "iq"} and lv < 2:
                out.add((f"inner{lv}", d.decimate_count, "usb+iq children"))
        else:
            pos = ("root", "sub", "level2")[lv]
            if not d.demod_usb:
                out.add((pos, d.decimate_count, f"iq{d.cstyle}"))
                if d.cstyle == 1:
                    out.add(("any", None, f"scalecomp:{d.scalecomp}"))
            elif d.late_decimate:
                out.add((pos, d.decimate_count, f"late{d.late_decimate}"))
                if d.decimate_count == 0 and lv == 1:
                    n = d.samples_per_buffer / LATE_CHUNK.get(d.late_decimate, 1)
                    out.add((pos, 0, f"late{d.late_decimate}:chunks={n:.3g}"))
            else:
                out.add((pos, d.decimate_count, "usb"))
                if d.filter_bw > 0:
                    out.add((pos, d.decimate_count, "usb_lpf"))
                    if lpf_taps(d) <= 64:
                        out.add((pos, d.decimate_count, "usb_lpf<=64"))
                if d.decimate_count == 5 and lv == 1:
                    out.add((pos, 5, f"pair:{d.samples_per_buffer // 1024}+{d.samples_per_buffer % 1024}"))
            if lv == 1:
                out.add((pos, None, f"lastchunk:{d.samples_per_buffer % 1024 or 1024}"))
        f, fs = d.mixer_freq, d.fs
        cls = "zero" if f == 0 else "+nyquist-1" if f == fs // 2 - 1 else "-nyquist+1" if f == -(fs // 2 - 1) else \
            "beyond nyquist" if abs(f) > fs / 2 else "eighths" if f != int(f) and f * 8 == int(f * 8) else None
        if cls and not ch:
            out.add(("any", None, "freq:" + cls))
    return out


def required_cells() -> set:
    """The lattice of the module docstring, spelled out."""
    r = set()
    r |= {("sub", d, "usb") for d in range(9)}
    r |= {("sub", 2, "usb_lpf<=64"), ("sub", 5, "usb_lpf"), ("sub", 6, "usb_lpf"), ("sub", 8, "usb_lpf")}
    r |= {("sub", None, f"lastchunk:{n}") for n in (256, 512, 768, 1024)}
    r |= {("sub", 5, f"pair:{n // 1024}+{n % 1024}") for n in D5_FRAMES}
    r |= {(f"inner{lv}", d, "usb+iq children") for lv in (0, 1) for d in (4, 5, 6)}
    r |= {(pos, d, f"late{L}") for pos in ("root", "sub") for d in (1, 3, 5, 6, 7, 8) for L in (5, 6)}
    r |= {("sub", 0, f"late5:chunks={c}") for c in ("2", "2.5", "3", "5")}
    r |= {("sub", 0, f"late6:chunks={c}") for c in ("2", "2.38", "3", "5")}
    r |= {("sub", d, f"iq{cs}") for d in (5, 6, 7, 8) for cs in (0, 1)}
    r |= {("any", None, f"scalecomp:{s}") for s in SCALECOMPS}
    r |= {("level2", 5, "usb"), ("level2", 6, "usb")}
    r |= {("any", None, "freq:" + c) for c in ("zero", "+nyquist-1", "-nyquist+1", "eighths", "beyond nyquist")}
    return r


def incidental_cells() -> set:
    """What the trees carry beyond that list, spelled out as well, so that the test can ask for equality: the shallow children
    that make an inner node a parent, the d = 5 (or d = 4) leaf every late0 tree keeps next to its late leaves (frames of 1 920 to
    5 040 samples: pairs and last chunks of their own), the d = 0 late leaves' plain cells, and the short filters of the deep leaves."""
    r = {("inner0", 0, "usb+iq children"), ("inner0", 1, "usb+iq children")}
    r |= {("level2", 0, "iq1"), ("level2", 1, "usb"), ("level2", 2, "iq1"), ("level2", 2, "usb"), ("level2", 3, "iq0")}
    r |= {("sub", 0, "late5"), ("sub", 0, "late6"), ("sub", 1, "iq0"), ("sub", 1, "iq1")}
    r |= {("sub", 2, "usb_lpf"), ("sub", 7, "usb_lpf")} | {("sub", d, "usb_lpf<=64") for d in (5, 6, 7, 8)}
    r |= {("sub", 5, f"pair:{p}") for p in ("1+896", "1+992", "2+352", "2+832", "4+704")}
    r |= {("sub", None, f"lastchunk:{n}") for n in (352, 704, 832, 896, 944, 976, 992)}
    return r


# ---- the input ----------------------------------------------------------------------------------------------------------------
def total_decimation(topo, i) -> int:
    """Raw samples per output sample of node i: the product of 2^d (and L) down its chain."""
    n = 1
    while i >= 0:
        d = topo.vfos[i]
        n *= (1 << d.decimate_count) * (d.late_decimate if d.demod_usb and d.late_decimate else 1)
        i = d.parent
    return n


def is_deep(topo, i) -> bool:
    """A leaf that gets a tone of its own: narrower than an eighth of the raw band."""
    return not topo.children(i) and total_decimation(topo, i) >= 8


def tones(topo) -> list:
    """One (raw frequency, amplitude) per deep leaf: an eighth of its output rate above its centre, walked up the chain
    (every mixer shifts by +mixer_freq; a frequency is taken modulo the node's input rate)."""
    out = []
    for i, d in enumerate(topo.vfos):
        if not is_deep(topo, i):
            continue
        f = d.output_rate / 8.0
        j = i
        while j >= 0:
            n = topo.vfos[j]
            f = (f - n.mixer_freq + n.fs / 2.0) % n.fs - n.fs / 2.0
            j = n.parent
        out.append((f, TONE_AMP))
    return out


@functools.lru_cache(maxsize=None)
def frames(name, n=N_FRAMES) -> tuple:
    """The raw frames of tree `name` (shared; read-only)."""
    topo = _trees()[name]
    lcg = synth.Lcg(4000 + sorted(_trees()).index(name))
    tn = tones(topo)
    out = []
    for f in range(n):
        iq = synth.lcg_frame(topo.frame, lcg) + synth.tone_frame(topo.frame, topo.fs, tn, f * topo.frame)
        iq.setflags(write=False)
        out.append(iq)
    return tuple(out)


# ---- one fixed schedule of live controls per tree -----------------------------------------------------------------------------
def schedule(topo, n=N_FRAMES) -> list:
    """sched[f] = the calls before frame f (the op tuples of live_ref.ModelTree.apply).  Before frame 1: park the first
    d >= 6 leaf, the first late leaf and the first IQ leaf.  Before frame 2: retune the deepest sub leaf and the deepest inner
    node (a non-integer and an integer frequency) and change the gain of the first USB leaf that is not parked.  Before frame
    3: unpark.  A tree without one of these kinds goes without that call."""
    leaves = topo.leaves_in_publish_order()
    v = topo.vfos

    def first(pred):
        return next((i for i in leaves if pred(v[i])), None)

    park = []
    for i in (first(lambda d: d.decimate_count >= 6), first(lambda d: d.demod_usb and d.late_decimate > 0), first(lambda d: not d.demod_usb)):
        if i is not None and i not in park:
            park.append(i)
    sched = [[] for _ in range(n)]
    if park:
        sched[1].append(("park", park))
        sched[3].append(("unpark", park))
    subs = [i for i in leaves if v[i].parent >= 0 and i not in park]
    inner = [i for i in range(len(v)) if topo.children(i)]

    def step(i):
        """A sixteenth of the slowest output rate below node i, in eighths of a Hz: every tone stays inside its passband."""
        below = [k for k in leaves if k == i or i in _ancestors(topo, k)]
        return max(1, round(min(v[k].output_rate for k in below) / 16.0 * 8)) / 8.0

    if subs:
        i = max(subs, key=lambda k: (v[k].decimate_count, -k))
        sched[2].append(("freq", i, v[i].mixer_freq + step(i) + 0.375))
    if inner:
        i = max(inner, key=lambda k: (v[k].decimate_count, -k))
        sched[2].append(("freq", i, v[i].mixer_freq - step(i)))
    usb = [i for i in leaves if v[i].demod_usb and i not in park]
    if usb:
        sched[2].append(("gain", usb[0], _g(v[usb[0]].gain * 0.5)))
    return sched


# ---- references, computed once per tree and shared ----------------------------------------------------------------------------
class Snapshot:
    """One oracle node after one frame, with the read-out methods tests/test_gpu_parity.py's checkers call."""

    def __init__(self, node, desc, leaf):
        self._stream = node.stream()
        self._usb = node.usb() if leaf and desc.demod_usb else None
        self._pre = node.usb_prequant() if leaf and desc.demod_usb else None
        self._iq = node.iq() if leaf and not desc.demod_usb else None

    def stream(self):
        return self._stream

    def usb(self):
        return self._usb

    def usb_prequant(self):
        return self._pre

    def iq(self):
        return self._iq


@functools.lru_cache(maxsize=None)
def oracle_frames(name, n=N_FRAMES) -> tuple:
    """Per frame the list of Snapshots of the plain-C oracle (no controls) on frames(name)."""
    from oracle import binding as ob
    topo = _trees()[name]
    nodes, roots = ob.build_tree("port", topo)
    out = []
    for iq in frames(name, n):
        ob.process_roots(roots, iq)
        out.append([Snapshot(nodes[i], d, not topo.children(i)) for i, d in enumerate(topo.vfos)])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def model_frames(name, n=N_FRAMES) -> tuple:
    """(want, descs): live_ref.ModelTree.process of every frame under schedule(tree), and the descriptors afterwards."""
    import live_ref as lr
    topo = _trees()[name]
    sched = schedule(topo, n)
    model = lr.ModelTree(topo)
    want = []
    for f, iq in enumerate(frames(name, n)):
        model.apply(sched[f])
        want.append(model.process(iq))
    return tuple(want), tuple(model.descs)
