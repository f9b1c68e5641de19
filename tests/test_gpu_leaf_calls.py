"""The calling rules of the per-leaf control calls, one table for the context's calls and the group's.

Every batched setter and getter (squelch, auto-squelch, parking, catch-up, watch, meters, retune, gain), the single-id
getters (output, pre-roll, watch PSD) and the single-leaf calls of the analyses on a watched source (drift estimate, band scan)
are called with each kind of wrong input, alone and two at a time, and the code that comes back is compared with the order
DESIGN.md states: handle, finalized, option, list shape, ids (range, leaf, once), values, frames in flight or delivered.  Then
one frame runs and every pair is read back: what was set is what is got.

The tree is helpers.tree_1536(): mains 0 and 1, leaves 2 3 (under 0) and 4 5 6 (under 1).  As a group on [0, 0] member 0
holds {0, 1, 2, 4} and member 1 {0, 1, 3, 5, 6}.  The ABI has no getter for a gain: a leaf's gain is read off its payload
(gain 0: a silent payload), a replicated main's retune off every replica's oscillator table (as test_gpu_retune does)."""
import ctypes as C

import numpy as np
import pytest

import retune_ref as rr
from helpers import tree_1536
from sdrreceiver_amd import _lib, synth

pytestmark = pytest.mark.gpu

OK, EINVAL, ESTATE = 0, _lib.SDRX_EINVAL, _lib.SDRX_ESTATE
NAN = float("nan")
LEAVES, PARENT = [2, 3, 4, 5, 6], 0
OPTIONS = ("meter", "squelch", "squelch_auto", "preroll", "park", "catchup", "watch")

# name: (option that must be on, value dtypes, a good entry, a bad entry)
SETTERS = {
    "set_squelch": ("squelch", (np.uint64, np.uint32), (1000, 2), None),
    "set_squelch_auto": ("squelch_auto", (np.uint32, np.uint32), (512, 3), (512, 0)),  # window_frames 0 with a ratio
    "set_active": ("park", (np.int32,), (1,), (2,)),
    "set_watch": ("watch", (np.int32,), (0,), (2,)),
    "set_mixer_freqs": (None, (np.float64,), (1000.0,), (NAN,)),
    "set_gains": (None, (np.float32,), (0.5,), (NAN,)),
}
ANY_VFO = ("set_mixer_freqs", "set_gains")  # accept an id with children
# name: (option that must be on, the record, needs a delivered frame)
GETTERS = {
    "get_meters": ("meter", _lib.MeterC, True),
    "get_squelch": ("squelch", _lib.SquelchStateC, True),
    "get_squelch_auto": ("squelch_auto", _lib.SquelchAutoStateC, True),
    "get_active": (None, _lib.ActiveStateC, False),
    "get_catchup": ("catchup", _lib.MeterC, False),
    "get_watch": ("watch", _lib.WatchLevelC, True),
}
# The single-leaf calls about the source of a watched leaf (besides get_watch_psd): True = needs no frame in flight -- there the
# group looks at ITS frames in flight before the member looks at anything, so a group with a frame in flight answers ESTATE
# where a context answers EINVAL; False = reads the delivered frame's record, and is the member's from the id's range on.
SINGLE = {"set_drift": True, "get_drift": False, "get_drift_profile": True, "set_scan": True, "get_scan": False,
          "get_scan_hits": True, "get_scan_cells": True}
GOOD_SCAN = dict(cell_bins=4, frames=1, floor_permille=500, ratio_q8=512, min_cells=1)
# what each setter refuses for its values: (call, arguments, what is wrong)
BAD_VALUES = [("set_drift", dict(max_shift=-1), "max_shift -1"), ("set_drift", dict(max_shift=_lib.DRIFT_MAX_SHIFT + 1), "max_shift past the limit"),
              ("set_drift", dict(templ=-1.0), "a negative template entry"), ("set_drift", dict(templ=NAN), "a template entry that is no number")]
BAD_VALUES += [("set_scan", dict(cfg=dict(GOOD_SCAN, **{key: v})), f"{key} {v}") for key, v in
               (("cell_bins", 3), ("cell_bins", -4), ("cell_bins", 512), ("frames", 0), ("frames", 65537), ("floor_permille", -1),
                ("floor_permille", 1001), ("ratio_q8", 0), ("min_cells", 0), ("min_cells", _lib.SPECTRUM_BINS // 4 + 1))]
BAD_VALUES += [("set_scan", dict(cfg=dict(GOOD_SCAN, reserved=(0, 0, 1))), "a reserved field"),
               ("set_scan", dict(cfg=dict(GOOD_SCAN, cell_bins=0, reserved=(1, 0, 0))), "a reserved field of a switch-off")]


class Api:
    """The context's calls or the group's, by prefix, on one handle; every call returns its code."""

    def __init__(self, kind, finalize=True, **options):
        from sdrreceiver_amd.receiver import Group, Receiver
        self.kind, self.topo = kind, tree_1536()
        self.prefix = "sdrx_" if kind == "ctx" else "sdrx_group_"
        if kind == "ctx":
            self.obj = Receiver(**{k: True for k in options})
        else:
            self.obj = Group([0, 0], **{k: 1 for k in options})
        self.L, self.h = self.obj.L, self.obj.h
        for d in self.topo.vfos:
            c, out = _lib.desc_to_c(d), C.c_int(-1)
            assert self.call("add_vfo", C.byref(c), C.byref(out)) == OK
            self.obj.descs.append(d)
        if finalize:
            assert self.call("finalize") == OK, self.error()

    def call(self, name, *args, handle=True):
        return getattr(self.L, self.prefix + name)(self.h if handle else None, *args)

    def error(self):
        return self.call("last_error").decode()

    def setter(self, name, ids, *vals, n=None, handle=True):
        """`ids` and each of `vals`: a list, or None for a null pointer."""
        arrs = [None if ids is None else np.asarray(ids, np.int32)]
        arrs += [None if v is None else np.asarray(v, dt) for v, dt in zip(vals, SETTERS[name][1])]
        ptrs = [None if a is None else a.ctypes.data for a in arrs]
        return self.call(name, *ptrs, len(ids) if n is None else n, handle=handle)

    def good(self, name, ids):
        return [[v] * len(ids) for v in SETTERS[name][2]]

    def getter(self, name, ids, n=None, out=True, handle=True):
        """(code, records)"""
        a = None if ids is None else np.asarray(ids, np.int32)
        count = (0 if ids is None else len(ids)) if n is None else n
        rec = (GETTERS[name][1] * max(1, count, 0 if ids is None else len(ids)))()
        rc = self.call(name, None if a is None else a.ctypes.data, count, rec if out else None, handle=handle)
        return rc, rec

    def output(self, vid, buf=True, handle=True):
        b, ln, rate = C.c_void_p(), C.c_uint32(), C.c_uint32()
        rc = self.call("get_output", vid, C.byref(b) if buf else None, C.byref(ln), C.byref(rate), handle=handle)
        return rc, (C.string_at(b.value, ln.value) if rc == OK and buf and ln.value else b"")

    def preroll(self, vid, handle=True):
        b, ln, f = C.c_void_p(), C.c_uint32(), C.c_int64(-7)
        return self.call("get_preroll", vid, C.byref(b), C.byref(ln), C.byref(f), handle=handle), ln.value, f.value

    def watch_psd(self, vid, handle=True):
        psd, f = np.zeros(_lib.SPECTRUM_BINS, np.float64), C.c_int64(-7)
        return self.call("get_watch_psd", vid, psd.ctypes.data, C.byref(f), handle=handle), psd, f.value

    def single(self, name, vid, handle=True, out=True, **kw):
        """(code, what it wrote) of the SINGLE call `name` about leaf `vid`, with good arguments but for `kw`: `templ` (a value
        for template entry 5; default: capture), `max_shift`, `cfg` (a dict of sdrx_scan_cfg's fields or None), `max_hits`;
        out = False: a null pointer for the result."""
        f = C.c_int64(-7)
        if name == "set_drift":
            t = None
            if "templ" in kw:
                t = np.ones(_lib.SPECTRUM_BINS, np.float64)
                t[5] = kw["templ"]
            return self.call(name, vid, None if t is None else t.ctypes.data, kw.get("max_shift", 2), handle=handle), None
        if name == "set_scan":
            cfg = dict(kw.get("cfg", GOOD_SCAN) or {})
            reserved = (C.c_int32 * 3)(*cfg.pop("reserved", (0, 0, 0)))
            c = _lib.ScanCfgC(reserved=reserved, **cfg)
            return self.call(name, vid, None if kw.get("cfg", GOOD_SCAN) is None else C.byref(c), handle=handle), None
        if name in ("get_drift", "get_scan"):
            rec = (_lib.DriftLevelC if name == "get_drift" else _lib.ScanLevelC)()
            return self.call(name, vid, C.byref(rec) if out else None, handle=handle), rec
        if name == "get_scan_hits":
            hits, n = (_lib.ScanHitC * 4)(), C.c_int(-7)
            rc = self.call(name, vid, C.cast(hits, C.c_void_p) if out else None, kw.get("max_hits", 4), C.byref(n), C.byref(f), handle=handle)
            return rc, (n.value, f.value)
        buf = np.zeros(max(_lib.SPECTRUM_BINS, 2 * _lib.DRIFT_MAX_SHIFT + 1), np.float64)  # get_drift_profile, get_scan_cells
        return self.call(name, vid, buf.ctypes.data, C.byref(f), handle=handle), (buf, f.value)

    def contexts_of(self, vid):
        """(context, local id) of every holder of VFO `vid`"""
        if self.kind == "ctx":
            return [(self.h, vid)]
        out = []
        for k in range(2):
            ctx, _ = self.obj.member_context(k)
            local = [i for i in ({0, 1, 2, 4}, {0, 1, 3, 5, 6})[k]]
            if vid in local:
                out.append((ctx, sorted(local).index(vid)))
        return out

    def nco(self, vid, count=64):
        tabs = []
        for ctx, lid in self.contexts_of(vid):
            out = np.zeros(2 * count, np.float32)
            assert self.L.sdrx_get_nco(ctx, lid, 0, count, out.ctypes.data) == OK
            tabs.append(out.view(np.complex64))
        return tabs

    def settings(self):
        """What the getters that answer at any time after a delivery say is set (the selection of the watch: through the PSD call,
        EINVAL for a leaf that is not watched)."""
        sq, au, ac = self.getter("get_squelch", LEAVES)[1], self.getter("get_squelch_auto", LEAVES)[1], self.getter("get_active", LEAVES)[1]
        # (a drift setting that took effect makes the profile ESTATE until the next frame, a scan setting the hits and the cells)
        reads = [(rc, out[0].tobytes()) for n in ("get_drift_profile", "get_scan_cells") for i in LEAVES for rc, out in [self.single(n, i)]]
        return ([(s.thr_sum_sq, s.hang_frames) for s in sq[:5]], [(s.ratio_q8, s.window_frames) for s in au[:5]],
                [(s.active, s.since_frame) for s in ac[:5]], [self.watch_psd(i)[0] == EINVAL for i in LEAVES],
                [t.tobytes() for i in range(7) for t in self.nco(i)], reads, [self.single("get_scan_hits", i) for i in LEAVES])

    def close(self):
        self.obj.close()


class Report:
    """Collects every line that differs, so that one run shows them all."""

    def __init__(self):
        self.lines = []

    def code(self, got, want, *what):
        if got != want:
            self.lines.append(f"{' '.join(str(w) for w in what)}: code {got}, expected {want}")

    def true(self, cond, *what):
        if not cond:
            self.lines.append(" ".join(str(w) for w in what))


def _unfinalized_and_null(api, r):
    """Before finalize everything is ESTATE whatever else is wrong with the call -- but for three single-id getters, which look
    at the id's range first; a null handle is EINVAL."""
    k = api.kind
    for name in SETTERS:
        r.code(api.setter(name, [2], *api.good(name, [2])), ESTATE, k, name, "before finalize")
        r.code(api.setter(name, [2], *api.good(name, [2]), n=-1), ESTATE, k, name, "before finalize, n = -1")
        r.code(api.setter(name, [2], *api.good(name, [2]), handle=False), EINVAL, k, name, "null handle")
    for name in GETTERS:
        r.code(api.getter(name, [2])[0], ESTATE, k, name, "before finalize")
        r.code(api.getter(name, None, n=-1)[0], ESTATE, k, name, "before finalize, n = -1")
        r.code(api.getter(name, [2], handle=False)[0], EINVAL, k, name, "null handle")
    r.code(api.output(2)[0], ESTATE, k, "get_output before finalize")
    r.code(api.preroll(2)[0], ESTATE, k, "get_preroll before finalize")
    r.code(api.watch_psd(2)[0], ESTATE, k, "get_watch_psd before finalize")
    r.code(api.output(99)[0], EINVAL, k, "get_output before finalize, id 99")
    r.code(api.preroll(99)[0], EINVAL if k == "ctx" else ESTATE, k, "get_preroll before finalize, id 99")
    r.code(api.watch_psd(99)[0], ESTATE, k, "get_watch_psd before finalize, id 99")
    r.code(api.output(2, handle=False)[0], EINVAL, k, "get_output, null handle")
    r.code(api.preroll(2, handle=False)[0], EINVAL, k, "get_preroll, null handle")
    r.code(api.watch_psd(2, handle=False)[0], EINVAL, k, "get_watch_psd, null handle")
    for name in SINGLE:  # finalized before the id, the shape and the values, on a context and on a group
        r.code(api.single(name, 2)[0], ESTATE, k, name, "before finalize")
        r.code(api.single(name, 99)[0], ESTATE, k, name, "before finalize, id 99")
        r.code(api.single(name, 2, out=False, max_hits=-1, max_shift=-1, cfg=dict(GOOD_SCAN, frames=0))[0], ESTATE, k, name, "before finalize, bad arguments")
        r.code(api.single(name, 2, handle=False)[0], EINVAL, k, name, "null handle")


def _options_off(api, r):
    """The option comes before the list.  The group's getters have no option check of their own -- the member that answers has
    it -- so there a malformed list is seen first, and an empty one asks no member."""
    k, grp = api.kind, api.kind == "group"
    for name, (opt, _, _, bad) in SETTERS.items():
        if opt is None:
            r.code(api.setter(name, [2], *api.good(name, [2])), OK, k, name, "needs no option")
            continue
        r.code(api.setter(name, [2], *api.good(name, [2])), ESTATE, k, name, "option off")
        r.code(api.setter(name, None, *[None] * len(api.good(name, [])), n=0), ESTATE, k, name, "option off, n = 0")
        # THE NAMED CASE: sdrx_group_set_squelch and sdrx_group_set_squelch_auto with the option off and a malformed list gave
        # SDRX_EINVAL before the calls were folded onto one path; SDRX_ESTATE like every other setter since.
        r.code(api.setter(name, [2], *api.good(name, [2]), n=-1), ESTATE, k, name, "option off, n = -1")  # named case (group squelch setters)
        r.code(api.setter(name, [99], *api.good(name, [99])), ESTATE, k, name, "option off, id 99")  # named case (group squelch setters)
        r.code(api.setter(name, [2, 2], *api.good(name, [2, 2])), ESTATE, k, name, "option off, id twice")  # named case (group squelch setters)
        if bad:
            r.code(api.setter(name, [2], *[[v] for v in bad]), ESTATE, k, name, "option off, bad value")  # named case (group squelch_auto setter)
    for name, (opt, _, _) in GETTERS.items():
        if opt is None:
            r.code(api.getter(name, [2])[0], OK, k, name, "needs no option")
            continue
        r.code(api.getter(name, [2])[0], ESTATE, k, name, "option off")
        r.code(api.getter(name, None, n=0, out=False)[0], OK if grp else ESTATE, k, name, "option off, n = 0")
        r.code(api.getter(name, [2], n=-1)[0], EINVAL if grp else ESTATE, k, name, "option off, n = -1")
        r.code(api.getter(name, [99])[0], EINVAL if grp else ESTATE, k, name, "option off, id 99")
    r.code(api.preroll(2)[0], ESTATE, k, "get_preroll, option off")
    r.code(api.preroll(99)[0], EINVAL, k, "get_preroll, option off, id 99")  # (the id's range comes first in this call)
    r.code(api.watch_psd(2)[0], ESTATE, k, "get_watch_psd, option off")
    r.code(api.watch_psd(99)[0], EINVAL if grp else ESTATE, k, "get_watch_psd, option off, id 99")
    for name in SINGLE:  # as get_watch_psd: the group has looked at the id's range when the member finds the option off
        r.code(api.single(name, 2)[0], ESTATE, k, name, "option off")
        r.code(api.single(name, 99)[0], EINVAL if grp else ESTATE, k, name, "option off, id 99")
        r.code(api.single(name, PARENT)[0], ESTATE, k, name, "option off, a VFO with children")
        r.code(api.single(name, 2, out=False, max_hits=-1, max_shift=-1, cfg=dict(GOOD_SCAN, frames=0))[0], ESTATE, k, name, "option off, bad arguments")


def _wrong_lists(api, r, when, in_flight, delivered):
    """Shape, ids and values of every call: SDRX_EINVAL whether or not a frame is in flight or delivered (the list comes first).
    Two things the group leaves to the member that answers, and so sees later than a context does: that an id of a getter
    names a leaf (a listed leaf in front of it is asked first, and may have no delivered frame to answer from), and that the
    id of the PSD call does (the group's frames in flight come first)."""
    k, grp = api.kind, api.kind == "group"
    for name, (_, dts, _, bad) in SETTERS.items():
        two = api.good(name, [2, 3])
        r.code(api.setter(name, [2, 3], *two, n=-1), EINVAL, k, name, when, "n = -1")
        r.code(api.setter(name, None, *two, n=2), EINVAL, k, name, when, "null ids")
        for q in range(len(dts)):
            r.code(api.setter(name, [2, 3], *[None if j == q else v for j, v in enumerate(two)]), EINVAL, k, name, when, "null values", q)
        r.code(api.setter(name, None, *[None] * len(dts), n=0), ESTATE if in_flight else OK, k, name, when, "n = 0, null arrays")
        for ids in ([-1], [99], [3, 99], [3, 3]) + (() if name in ANY_VFO else ([PARENT], [3, PARENT])):
            r.code(api.setter(name, list(ids), *api.good(name, ids)), EINVAL, k, name, when, "ids", ids)
        if bad:
            r.code(api.setter(name, [2], *[[v] for v in bad]), EINVAL, k, name, when, "bad value")
            r.code(api.setter(name, [3, 2], *[[g, v] for g, v in zip(SETTERS[name][2], bad)]), EINVAL, k, name, when, "a good entry beside a bad one")
    for name in GETTERS:
        r.code(api.getter(name, [2, 3], n=-1)[0], EINVAL, k, name, when, "n = -1")
        r.code(api.getter(name, None, n=2)[0], EINVAL, k, name, when, "null ids")
        r.code(api.getter(name, [2, 3], out=False)[0], EINVAL, k, name, when, "null out")
        r.code(api.getter(name, None, n=0, out=False)[0], OK, k, name, when, "n = 0, null arrays")
        for ids in ([-1], [99], [3, 99], [PARENT]):
            r.code(api.getter(name, ids)[0], EINVAL, k, name, when, "ids", ids)
        unanswered = grp and GETTERS[name][2] and not delivered
        r.code(api.getter(name, [3, PARENT])[0], ESTATE if unanswered else EINVAL, k, name, when, "ids", [3, PARENT])
    for vid in (-1, 99, PARENT):
        r.code(api.output(vid)[0], EINVAL, k, "get_output", when, "id", vid)
        r.code(api.preroll(vid)[0], EINVAL, k, "get_preroll", when, "id", vid)
        r.code(api.watch_psd(vid)[0], ESTATE if grp and in_flight and vid == PARENT else EINVAL, k, "get_watch_psd", when, "id", vid)
    # The single-leaf calls of the drift and the scan.  Leaf 3 is never watched, leaf 5's source never has a drift or a scan; leaf 2
    # is watched, and its source has both, from _round_trip on (before that, that it is not watched is what is wrong with it).
    # On a group every call that needs no frame in flight is ESTATE while there is one, whatever else is wrong past the id's range.
    early = ESTATE if grp and in_flight else EINVAL
    for name, between in SINGLE.items():
        for vid in (-1, 99):
            r.code(api.single(name, vid)[0], EINVAL, k, name, when, "id", vid)
        r.code(api.single(name, PARENT)[0], early if between else EINVAL, k, name, when, "id", PARENT)
        if between:
            r.code(api.single(name, 3)[0], early, k, name, when, "a leaf that is not watched")
    for name in ("get_drift_profile", "get_scan_hits", "get_scan_cells"):
        r.code(api.single(name, 5)[0], early, k, name, when, "a source without the analysis")
    for name, kw, what in BAD_VALUES:
        r.code(api.single(name, 2, **kw)[0], early, k, name, when, what)
    r.code(api.single("get_drift", 2, out=False)[0], EINVAL, k, "get_drift", when, "null out")
    r.code(api.single("get_scan", 2, out=False)[0], EINVAL, k, "get_scan", when, "null out")
    r.code(api.single("get_scan_hits", 2, max_hits=-1)[0], early, k, "get_scan_hits", when, "max_hits -1")
    r.code(api.single("get_scan_hits", 2, out=False)[0], early, k, "get_scan_hits", when, "null hits with room for 4")
    r.code(api.single("get_scan_hits", 99, max_hits=-1)[0], EINVAL, k, "get_scan_hits", when, "max_hits -1, id 99")


def _nothing_delivered(api, r, when, in_flight):
    """The getters of a frame's results before any frame has been delivered; the two that answer at any time."""
    k = api.kind
    for name, (_, _, needs_frame) in GETTERS.items():
        r.code(api.getter(name, [2, 3])[0], ESTATE if needs_frame else OK, k, name, when)
    r.code(api.output(2)[0], ESTATE, k, "get_output", when)
    r.code(api.output(2, buf=False)[0], ESTATE if in_flight else OK, k, "get_output as a length query", when)
    r.code(api.preroll(2)[0], ESTATE, k, "get_preroll", when)
    r.code(api.single("get_drift", 2)[0], ESTATE, k, "get_drift", when)
    r.code(api.single("get_scan", 2)[0], ESTATE, k, "get_scan", when)


def _round_trip(api, r, iq):
    """Sets every pair, runs ONE frame (submitted, so that the calls meet a frame in flight) and reads every pair back."""
    k, topo = api.kind, api.topo
    f0, f6 = 480000.0, -60000.0  # main 0 (a replica on every member) and leaf 6
    steps = [("set_squelch", [2, 5], [1, 7], [2, 3]), ("set_squelch_auto", [2, 3], [128, 300], [2, 4]), ("set_active", [3, 2], [0, 1]),
             ("set_watch", [2, 5], [1, 1]), ("set_gains", [4, PARENT], [0.0, 0.25]), ("set_mixer_freqs", [PARENT, 6], [f0, f6])]
    for name, ids, *vals in steps:
        r.code(api.setter(name, ids, *vals), OK, k, name, "valid", api.error())
    r.code(api.watch_psd(3)[0], EINVAL, k, "get_watch_psd of a leaf that is not watched")
    r.code(api.watch_psd(2)[0], ESTATE, k, "get_watch_psd before the first measured frame")
    for name in ("get_drift_profile", "get_scan_hits", "get_scan_cells"):
        r.code(api.single(name, 2)[0], EINVAL, k, name, "of a watched leaf whose source has no such analysis")
    r.code(api.single("set_drift", 2, max_shift=0)[0], OK, k, "set_drift: off where it is off", api.error())
    r.code(api.single("set_scan", 2, cfg=None)[0], OK, k, "set_scan: off where it is off", api.error())
    r.code(api.single("set_drift", 2)[0], OK, k, "set_drift", "valid", api.error())  # captures frame 0 as the template
    r.code(api.single("set_scan", 2)[0], OK, k, "set_scan", "valid", api.error())  # one frame per evaluation
    r.code(api.single("get_drift_profile", 2)[0], ESTATE, k, "get_drift_profile before the first measured frame")
    r.code(api.single("get_scan_hits", 2)[0], ESTATE, k, "get_scan_hits before the first evaluation")
    r.code(api.single("get_scan_cells", 2)[0], ESTATE, k, "get_scan_cells before the first evaluation")
    api.obj.submit(iq)
    for name in SETTERS:  # a frame submitted and not waited for
        r.code(api.setter(name, [2], *api.good(name, [2])), ESTATE, k, name, "a frame in flight")
    r.code(api.watch_psd(2)[0], ESTATE, k, "get_watch_psd, a frame in flight")
    for name, between in SINGLE.items():
        if between:
            r.code(api.single(name, 2)[0], ESTATE, k, name, "a frame in flight")
    _wrong_lists(api, r, "in flight", True, False)  # the list before the frames in flight
    _nothing_delivered(api, r, "in flight, nothing delivered", True)
    api.obj.wait()
    for name in GETTERS:  # a getter takes an id twice
        rc, rec = api.getter(name, [5, 2, 5])
        r.code(rc, OK, k, name, "an id twice")
        r.true(bytes(rec[0]) == bytes(rec[2]), k, name, "an id twice: two different answers")
    sq, au = api.getter("get_squelch", [2, 5, 3])[1], api.getter("get_squelch_auto", [2, 3, 5])[1]
    r.true([(s.frame, s.thr_sum_sq, s.hang_frames) for s in sq[:3]] == [(0, 1, 2), (0, 7, 3), (0, 0, 0)], k, "squelch read back")
    r.true([(s.frame, s.ratio_q8, s.window_frames) for s in au[:3]] == [(0, 128, 2), (0, 300, 4), (0, 0, 0)], k, "squelch_auto read back")
    ac = api.getter("get_active", LEAVES)[1]
    r.true([(s.active, s.since_frame) for s in ac[:5]] == [(1, 0), (0, 0), (1, 0), (1, 0), (1, 0)], k, "active read back")
    r.true(api.output(3) == (OK, b""), k, "a parked leaf has a payload")
    wa = api.getter("get_watch", [2, 5, 4])[1]
    r.true([(w.frame, w.watched) for w in wa[:3]] == [(0, 1), (0, 1), (0, 0)] and wa[0].band_pwr > 0 and wa[1].total_pwr > 0, k, "watch read back")
    rc, psd, frame = api.watch_psd(2)
    r.true(rc == OK and frame == 0 and float(psd.sum()) > 0, k, "get_watch_psd of a watched leaf", rc, frame)
    rc, dl = api.single("get_drift", 2)
    r.true(rc == OK and (dl.frame, dl.measured, dl.captured, dl.max_shift, dl.shift) == (0, 1, 1, 2, 0), k, "drift read back", rc, dl.frame, dl.measured, dl.captured)
    rc, sl = api.single("get_scan", 2)
    r.true(rc == OK and (sl.frame, sl.measured, sl.complete, sl.cell_bins, sl.frames, sl.integrated) == (0, 1, 1, 4, 1, 1), k, "scan read back", rc, sl.frame, sl.complete)
    for name in ("get_drift", "get_scan"):  # a leaf whose source has no analysis: an empty record of the delivered frame
        rc, rec = api.single(name, 5)
        r.true(rc == OK and (rec.frame, rec.measured) == (0, 0), k, name, "of a source without the analysis", rc, rec.frame, rec.measured)
    rc, (prof, frame) = api.single("get_drift_profile", 2)
    r.true(rc == OK and frame == 0 and prof[2] > 0 and not prof[5:].any(), k, "get_drift_profile of a measured source", rc, frame)
    rc, (n, frame) = api.single("get_scan_hits", 2)
    r.true(rc == OK and frame == 0 and 0 <= n <= min(4, sl.n_stored), k, "get_scan_hits of a completed evaluation", rc, n, frame)
    r.code(api.single("get_scan_hits", 2, out=False, max_hits=0)[0], OK, k, "get_scan_hits as a question without room")
    rc, (cells, frame) = api.single("get_scan_cells", 2)
    r.true(rc == OK and frame == 0 and float(cells[:2048].sum()) > 0 and not cells[2048:].any(), k, "get_scan_cells of a completed evaluation", rc, frame)
    me = api.getter("get_meters", LEAVES)[1]
    for j, i in enumerate(LEAVES):
        rc, pay = api.output(i)
        v = np.frombuffer(pay, np.int16).astype(np.int64)
        r.true(rc == OK and me[j].frame == 0 and me[j].sum_sq == int((v ** 2).sum()) and me[j].n_values == v.size, k, "meter of leaf", i)
        r.true(v.size == (0 if i == 3 else topo.vfos[i].samples_per_buffer >> topo.vfos[i].decimate_count), k, "payload length of leaf", i)
        r.true(i != 4 or not v.any(), k, "gain 0 on leaf 4: its payload is not silent")
        r.true(i in (3, 4) or v.any(), k, "leaf", i, "is silent")
    for vid, f in ((PARENT, f0), (6, f6)):  # every holder of the VFO has the new oscillator
        tabs, want = api.nco(vid), rr.table(topo.vfos[vid].fs, f)[:64]
        r.true(len(tabs) == (2 if k == "group" and vid == PARENT else 1), k, "holders of vfo", vid)
        for t in tabs:
            r.true(np.array_equal(t.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), k, "oscillator table of vfo", vid)
    rc, ln, frame = api.preroll(2)
    r.true((rc, ln, frame) == (OK, 0, -1), k, "get_preroll of a leaf that did not just open", rc, ln, frame)
    # refused calls change nothing: a good entry beside a bad one included
    before = api.settings()
    _wrong_lists(api, r, "delivered", False, True)
    r.true(api.settings() == before, k, "a refused call changed a setting")
    # unparked with a catch-up: leaf 3 runs frame 0 before the call returns, and its meter of that frame is there at once
    r.code(api.setter("set_active", [3], [1]), OK, k, "unpark", api.error())
    cu = api.getter("get_catchup", [3, 2])[1]
    r.true(cu[0].frame == 0 and cu[0].n_values == 96000 >> 5 and cu[0].sum_sq > 0 and cu[1].frame == -1, k, "catch-up read back", cu[0].frame, cu[1].frame)
    ac = api.getter("get_active", [3])[1]
    r.true((ac[0].active, ac[0].since_frame) == (1, 1), k, "active after the unpark")
    # a new setting: the profile and the evaluation are no longer this setting's; switched off: the source has no analysis
    r.code(api.single("set_drift", 2, templ=1.0, max_shift=3)[0], OK, k, "set_drift with a template", api.error())
    r.code(api.single("get_drift_profile", 2)[0], ESTATE, k, "get_drift_profile after a new setting")
    r.code(api.single("set_scan", 2)[0], OK, k, "set_scan again", api.error())
    r.code(api.single("get_scan_cells", 2)[0], ESTATE, k, "get_scan_cells after a new setting")
    r.code(api.single("set_drift", 2, max_shift=0)[0], OK, k, "set_drift: off", api.error())
    r.code(api.single("set_scan", 2, cfg=None)[0], OK, k, "set_scan: off", api.error())
    for name in ("get_drift_profile", "get_scan_hits", "get_scan_cells"):
        r.code(api.single(name, 2)[0], EINVAL, k, name, "after the switch-off")
    rc, dl = api.single("get_drift", 2)  # the delivered frame ran with the analyses on
    r.true(rc == OK and (dl.frame, dl.measured) == (0, 1), k, "get_drift of frame 0 after the switch-off", rc, dl.frame, dl.measured)
    rc, sl = api.single("get_scan", 2)
    r.true(rc == OK and (sl.frame, sl.measured) == (0, 1), k, "get_scan of frame 0 after the switch-off", rc, sl.frame, sl.measured)


@pytest.mark.parametrize("kind", ["ctx", "group"])
def test_leaf_call_rules(kind):
    r = Report()
    raw = Api(kind, finalize=False, **{o: 1 for o in OPTIONS})
    _unfinalized_and_null(raw, r)
    raw.close()
    off = Api(kind)
    _options_off(off, r)
    off.close()
    on = Api(kind, **{o: 1 for o in OPTIONS})
    _wrong_lists(on, r, "no frame yet", False, False)
    _nothing_delivered(on, r, "no frame yet", False)
    _round_trip(on, r, synth.lcg_frame(on.topo.frame, synth.Lcg(23)))
    on.close()
    assert not r.lines, "\n" + "\n".join(r.lines)
