"""Host-side mirror of the reference interface for the VFO chain, over the C ABI.

Two layers:

* :class:`Receiver` -- thin object wrapper around ``sdrx_*`` (one context = one VFO tree).
* :class:`vfo` and :class:`sdrj` -- the reference's own class and method names (vfo.h:16-49,
  sdrj.h:29-48) so that host code and parity tests read like reference-side code:
  ``v = vfo(); v.setFs(...); v.setMixerFreq(...); v.init(n, True); main.setVFOs([...]);
  radio = sdrj(); radio.setVFOs([main]); radio.demodData(data, len)``.

Everything here is plumbing; the arithmetic runs in the HIP kernels of libsdrx.so.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib, agc as _agc, blank as _blank, postdet, iqbal as _iqbal, drift as _drift, front as _front, ingest, meter, notch as _notch, resample as _resample, scan as _scan, shift as _shift, squelch as _squelch, wake as _wake, watch as _watch
from .topology import Topology, VfoDesc


class SdrxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"sdrx error {code}: {msg}")
        self.code = code


def arithmetic(exact) -> int:
    """Option "exact" of include/sdrx.h: True / 1 / "exact" -> 1 (bit-identical to the -O2 reference), False / 0 / "tolerance" -> 0
    (NCO as rotations of its exact checkpoints, FMA mixer and filters), 2 / "robust" -> 2 (exact NCO, FMA mixer and filters)."""
    if isinstance(exact, str):
        return {"exact": 1, "tolerance": 0, "fast": 0, "robust": 2}[exact]
    return 2 if (exact is not True and exact == 2) else int(bool(exact))


SPECTRUM_RAW = _lib.SPECTRUM_RAW  # the raw frame's spectrum (sdrj's own fftData, every 4th frame)


def _value_list(vids, values, dtype) -> tuple[np.ndarray, np.ndarray]:
    ids = np.ascontiguousarray(np.atleast_1d(np.asarray(vids)), dtype=np.int32).reshape(-1)
    vals = np.ascontiguousarray(np.atleast_1d(np.asarray(values, dtype=dtype)), dtype=dtype).reshape(-1)
    if ids.size != vals.size:
        raise ValueError(f"{ids.size} ids but {vals.size} values")
    return ids, vals


class _LeafCalls:
    """The per-leaf calls a :class:`Receiver` and a :class:`Group` share: ``sdrx_<name>`` on a context, ``sdrx_group_<name>`` --
    with ids of the whole tree, answered by the member that holds the VFO, the counts summed over the members -- on a group."""

    _prefix = "sdrx_"

    def _call(self, name, *args) -> None:
        self._chk(getattr(self.L, self._prefix + name)(self.h, *args))

    def _get_list(self, symbol, vids, StructC):
        """``(ids, records)`` of the batched getter `symbol` for the leaves `vids`."""
        ids = np.ascontiguousarray(vids, dtype=np.int32).reshape(-1)
        out = (StructC * max(1, ids.size))()
        self._call(symbol, ids.ctypes.data, ids.size, out)
        return ids, out[:ids.size]

    def _set_list(self, symbol, vids, *columns) -> tuple[np.ndarray, np.ndarray]:
        """The batched setter `symbol` with one ``(values, dtype)`` column per array of the call; ``(ids, last column)``."""
        cols = [_value_list(vids, values, dtype) for values, dtype in columns]
        ids = cols[0][0]
        self._call(symbol, ids.ctypes.data, *[v.ctypes.data for _, v in cols], ids.size)
        return ids, cols[-1][1]

    def _payload(self, vid, buf, length) -> np.ndarray:
        raw = C.string_at(buf.value, length.value) if length.value else b""
        return np.frombuffer(raw, dtype=np.int16 if self._int16(vid) else np.int8).copy()

    def _int16(self, vid) -> bool:
        """int16 payload values: a USB leaf or a detector leaf; int8 otherwise (compress())"""
        return bool(self.descs[vid].demod_usb or self.descs[vid].detector)

    def output(self, vid: int) -> np.ndarray:
        """Leaf `vid`'s payload of the last delivered frame (int16 audio -- USB or a detector's -- or int8 I/Q)."""
        buf, ln, rate = C.c_void_p(), C.c_uint32(), C.c_uint32()
        self._call("get_output", vid, C.byref(buf), C.byref(ln), C.byref(rate))
        return self._payload(vid, buf, ln)

    def meters(self, vids) -> dict:
        """Output meters of the leaves `vids` for the last delivered frame (option ``meter``): arrays in the order of
        `vids` -- see :func:`sdrreceiver_amd.meter.meters_dict`."""
        ids, out = self._get_list("get_meters", vids, _lib.MeterC)
        return meter.meters_dict(out, [self._int16(i) for i in ids.tolist()])

    # -- squelch-gated egress (option ``squelch``; sdrreceiver_amd.squelch has the definition) ---------------------
    def set_squelch(self, vids, thr_sum_sq, hang_frames) -> None:
        """Leaf vids[k] opens when its meter ``sum_sq`` reaches thr_sum_sq[k] and stays open hang_frames[k] frames
        after it last did; from the next frame on.  Resets the named leaves' ``hang_left``."""
        self._set_list("set_squelch", vids, (thr_sum_sq, np.uint64), (hang_frames, np.uint32))

    def squelch(self, vids) -> dict:
        """Squelch state of the leaves `vids` after the last delivered frame: ``frame``, ``thr_sum_sq``,
        ``hang_frames``, ``hang_left``, ``open`` as arrays in the order of `vids`."""
        return _squelch.squelch_dict(self._get_list("get_squelch", vids, _lib.SquelchStateC)[1])

    def egress(self) -> dict:
        """What the last delivered frame's payload copy moved: ``frame``, ``n_open``, ``n_leaves``,
        ``payload_bytes_copied``."""
        f, o, n, b = C.c_int64(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._call("get_egress", C.byref(f), C.byref(o), C.byref(n), C.byref(b))
        return {"frame": f.value, "n_open": o.value, "n_leaves": n.value, "payload_bytes_copied": b.value}

    def preroll(self, vid: int) -> np.ndarray:
        """Option ``preroll``: leaf `vid`'s payload of the frame before the delivered one, if the leaf has just opened (what
        the callback saw first); an empty array of the leaf's dtype otherwise."""
        buf, ln, f = C.c_void_p(), C.c_uint32(), C.c_int64()
        self._call("get_preroll", vid, C.byref(buf), C.byref(ln), C.byref(f))
        return self._payload(vid, buf, ln)

    def preroll_count(self) -> dict:
        """Pre-rolled leaves of the last delivered frame and the bytes that added to its copy: ``n_preroll``,
        ``preroll_bytes``."""
        n, b = C.c_uint32(), C.c_uint64()
        self._call("get_preroll_count", C.byref(n), C.byref(b))
        return {"n_preroll": n.value, "preroll_bytes": b.value}

    # -- auto-squelch (option ``squelch_auto``): the threshold as a ratio over the leaf's tracked noise floor -----------
    def set_squelch_auto(self, vids, ratio_q8, window_frames) -> None:
        """Leaf vids[k]'s threshold becomes ``max(thr, floor * ratio_q8[k] / 256)``, the floor being the minimum ``sum_sq``
        of the last ``window_frames[k]`` .. ``2 * window_frames[k] - 1`` frames (:func:`sdrreceiver_amd.squelch.decide_auto`);
        ``ratio_q8`` 0 switches it off for the leaf.  Restarts the named leaves' floor."""
        self._set_list("set_squelch_auto", vids, (ratio_q8, np.uint32), (window_frames, np.uint32))

    def squelch_auto(self, vids) -> dict:
        """What decided the last delivered frame for the leaves `vids`: ``frame``, ``floor_sum_sq``, ``thr_eff_sum_sq``,
        ``ratio_q8``, ``window_frames``, ``floor_valid`` as arrays in the order of `vids`."""
        return _squelch.squelch_auto_dict(self._get_list("get_squelch_auto", vids, _lib.SquelchAutoStateC)[1])

    # -- device-side AGC (option ``agc``; sdrreceiver_amd.agc has the rule): the gain follows the meter between frames --------
    def set_agc(self, vids, lo_ms, hi_ms, silent_ms, hold_frames, up, down, gain_min, gain_max) -> None:
        """AGC settings of the USB leaves `vids` from the next frame on (``sdrx_agc_cfg``; every argument a scalar or one value
        per leaf): the window ``lo_ms`` .. ``hi_ms`` on the payload's mean square in LSB^2 (``hi_ms`` 0: off for the leaf),
        ``silent_ms`` below which a frame is no observation, ``hold_frames`` cold frames to sit out before a raise, the step
        factors and the limits.  Restarts the named leaves' ``quiet_run``."""
        ids = np.ascontiguousarray(np.atleast_1d(np.asarray(vids)), dtype=np.int32).reshape(-1)
        cols = [np.broadcast_to(np.asarray(v, dt), ids.shape) for v, dt in
                ((lo_ms, np.uint32), (hi_ms, np.uint32), (silent_ms, np.uint32), (hold_frames, np.uint32),
                 (up, np.float32), (down, np.float32), (gain_min, np.float32), (gain_max, np.float32))]
        cfgs = (_lib.AgcCfgC * max(1, ids.size))()
        for k in range(ids.size):
            cfgs[k] = _lib.AgcCfgC(int(cols[0][k]), int(cols[1][k]), int(cols[2][k]), int(cols[3][k]),
                                   float(cols[4][k]), float(cols[5][k]), float(cols[6][k]), float(cols[7][k]))
        self._call("set_agc", ids.ctypes.data, cfgs, ids.size)

    def agc(self, vids) -> dict:
        """What the gain step did behind the last delivered frame for the leaves `vids`: ``frame``, ``gain_used`` (the gain
        that frame was computed with), ``gain_next``, ``action`` (-1 / 0 / +1), ``quiet_run`` and the settings as set, as
        arrays in the order of `vids`.  This is how a host reads a gain the device steps."""
        return _agc.agc_dict(self._get_list("get_agc", vids, _lib.AgcStateC)[1])

    # -- parking (option ``park``): leaves switched off and on between frames --------------------------------------------
    def set_active(self, vids, active) -> None:
        """Park (``active[k]`` 0) or unpark (1) the leaves `vids` before the next frame.  A parked leaf costs no arithmetic and
        is delivered like a closed one; an unparked leaf starts as a new VFO does (fresh oscillator, zero filter state)."""
        self._set_list("set_active", vids, (active, np.int32))

    def active(self, vids) -> dict:
        """``active`` and ``since_frame`` (the first frame in the present state; a group counts its own frames) of the leaves
        `vids`, as arrays."""
        _, out = self._get_list("get_active", vids, _lib.ActiveStateC)
        return {"active": np.array([o.active for o in out], dtype=np.int32),
                "since_frame": np.array([o.since_frame for o in out], dtype=np.int64)}

    def catchup(self, vids) -> dict:
        """Option ``catchup``: the meter of the frame each of the leaves `vids` was caught up in -- the frame before the one
        :meth:`set_active` unparked it for, run on the parent's stream the device still held -- as :meth:`meters` gives it;
        ``frame`` is -1 (and the figures 0) for a leaf whose present active state did not begin with a catch-up.  Good as
        soon as :meth:`set_active` has returned."""
        ids, out = self._get_list("get_catchup", vids, _lib.MeterC)
        return meter.meters_dict(out, [self._int16(i) for i in ids.tolist()])

    # -- channel watch (option ``watch``; sdrreceiver_amd.watch): band power of a leaf from its source's spectrum -------------
    def set_watch(self, vids, on) -> None:
        """Watch (``on[k]`` 1) or stop watching (0) the leaves `vids` from the next frame on, whether they are active or
        parked."""
        self._set_list("set_watch", vids, (on, np.int32))

    def watch(self, vids) -> dict:
        """Watch figures of the leaves `vids` for the last delivered frame: ``frame``, ``band_pwr``, ``total_pwr``,
        ``first_bin``, ``n_bins``, ``segments``, ``watched`` as arrays in the order of `vids`."""
        return _watch.watch_dict(self._get_list("get_watch", vids, _lib.WatchLevelC)[1])

    def watch_psd(self, vid: int) -> tuple[np.ndarray, int]:
        """``(PSD, frame)``: the power spectrum (8192 float64, kiss_fft's natural order) of the source of watched leaf `vid`
        after the last frame."""
        psd = np.zeros(_lib.SPECTRUM_BINS, np.float64)
        f = C.c_int64()
        self._call("get_watch_psd", int(vid), psd.ctypes.data, C.byref(f))
        return psd, f.value

    # -- device-side wake (option ``wake``; sdrreceiver_amd.wake has the rule): the watch parks and unparks leaves in the frame ----
    def set_wake(self, vids, min_band_pwr, contrast_q8=0, hold_frames=0, on=1) -> None:
        """Wake settings of the watched leaves `vids` from the next frame on (``sdrx_wake_cfg``; every argument a scalar or one
        value per leaf): a leaf is hot when its ``band_pwr`` reaches ``min_band_pwr`` and -- ``contrast_q8`` > 0 -- its contrast
        reaches ``contrast_q8 / 256``; it runs in hot frames and ``hold_frames`` frames after the last one, and is parked in
        the others, decided on the device for the very frame that was measured.  ``on`` 0 releases the leaf in the state its
        last frame ran in.  Restarts the named leaves' ``hold_left``."""
        ids = np.ascontiguousarray(np.atleast_1d(np.asarray(vids)), dtype=np.int32).reshape(-1)
        cols = [np.broadcast_to(np.asarray(v, dt), ids.shape) for v, dt in
                ((min_band_pwr, np.float64), (contrast_q8, np.uint32), (hold_frames, np.uint32), (on, np.uint32))]
        cfgs = (_lib.WakeCfgC * max(1, ids.size))()
        for k in range(ids.size):
            cfgs[k] = _lib.WakeCfgC(float(cols[0][k]), int(cols[1][k]), int(cols[2][k]), int(cols[3][k]))
        self._call("set_wake", ids.ctypes.data, cfgs, ids.size)

    def wake(self, vids) -> dict:
        """What the wake step decided for the leaves `vids` in the last delivered frame: ``frame``, ``since_frame``, ``active``,
        ``hot``, ``hold_left``, ``controlled`` as arrays in the order of `vids` (``controlled`` 0: the leaf was not under the
        device's control in that frame; ``active`` and ``since_frame`` are then the host's bookkeeping)."""
        return _wake.wake_dict(self._get_list("get_wake", vids, _lib.WakeStateC)[1])

    # -- ADC meter (option ``adc_meter``; sdrreceiver_amd.ingest has the derived figures): the integer samples as they arrived ---
    def adc_meter(self) -> dict:
        """The ADC record of the last delivered frame (:func:`sdrreceiver_amd.ingest.adc_dict`): exact integer statistics of the
        frame's integer samples before conversion and DC removal; ``measured`` 0 (and ``fmt`` -1) for a frame that did not
        arrive as integer samples.  On a group: the first member's record (every member's is the same).
        :func:`sdrreceiver_amd.ingest.adc_levels` turns it into levels, headroom and IQ balance."""
        out = _lib.AdcMeterC()
        self._call("get_adc_meter", C.byref(out))
        return ingest.adc_dict(out)

    # -- drift estimate (part of option ``watch``; sdrreceiver_amd.drift): the source's spectrum registered against a template --
    def set_drift(self, vid: int, template=None, max_shift: int = 0) -> None:
        """The drift estimate of the source of watched leaf `vid` from the next frame on, over the shifts ``-max_shift ..
        max_shift`` bins (0: off).  `template`: 8192 float64, each finite and >= 0; None: capture -- the source's spectrum of
        the next measured frame becomes the template, on the device."""
        t = None if template is None else np.ascontiguousarray(template, dtype=np.float64).reshape(-1)
        if t is not None and t.size != _lib.SPECTRUM_BINS:
            raise ValueError(f"a template has {_lib.SPECTRUM_BINS} entries, not {t.size}")
        self._call("set_drift", int(vid), None if t is None else t.ctypes.data, int(max_shift))

    def drift(self, vid: int) -> dict:
        """The drift record of the source of leaf `vid` for the last delivered frame (:func:`sdrreceiver_amd.drift.drift_dict`;
        :func:`sdrreceiver_amd.drift.estimate_hz` turns it into Hz)."""
        out = _lib.DriftLevelC()
        self._call("get_drift", int(vid), C.byref(out))
        return _drift.drift_dict(out)

    def drift_profile(self, vid: int) -> tuple[np.ndarray, int]:
        """``(profile, frame)``: the correlation at the shifts ``-K .. K`` (2K + 1 float64) of the source of watched leaf `vid`
        after the last frame."""
        prof = np.zeros(2 * _lib.DRIFT_MAX_SHIFT + 1, np.float64)
        f = C.c_int64()
        self._call("get_drift_profile", int(vid), prof.ctypes.data, C.byref(f))
        return prof[:2 * self.drift(vid)["max_shift"] + 1].copy(), f.value

    # -- band scan (part of option ``watch``; sdrreceiver_amd.scan): the carriers in the source's integrated spectrum -------------
    def set_scan(self, vid: int, cell_bins: int = 0, frames: int = 1, floor_permille: int = 0, ratio_q8: int = 0,
                 min_cells: int = 1) -> None:
        """The band scan of the source of watched leaf `vid` from the next frame on: cells of `cell_bins` bins (a power of two 1 ..
        256; 0: off), `frames` frames integrated per evaluation, the floor at rank ``floor_permille (C - 1) / 1000`` of the
        cells, hot above ``ratio_q8 / 256`` times the floor, runs of at least `min_cells` cells reported.  Every call that
        switches it on restarts the integration."""
        if int(cell_bins) == 0:
            self._call("set_scan", int(vid), None)
            return
        if not 0 <= int(ratio_q8) < 1 << 32:
            raise ValueError(f"ratio_q8 {ratio_q8} is no uint32")
        cfg = _lib.ScanCfgC(int(cell_bins), int(frames), int(floor_permille), int(ratio_q8), int(min_cells))
        self._call("set_scan", int(vid), C.byref(cfg))
        self._scan_w[self.descs[int(vid)].parent] = int(cell_bins)

    def scan(self, vid: int) -> dict:
        """The scan record of the source of leaf `vid` for the last delivered frame (:func:`sdrreceiver_amd.scan.scan_dict`)."""
        out = _lib.ScanLevelC()
        self._call("get_scan", int(vid), C.byref(out))
        return _scan.scan_dict(out)

    def scan_hits(self, vid: int, max_hits: int = _lib.SCAN_MAX_HITS) -> tuple[list, int]:
        """``(hits, frame)``: the stored hits (dicts, :func:`sdrreceiver_amd.scan.hit_dict`) of the last completed evaluation of
        the source of watched leaf `vid`, at most `max_hits`, and the frame it completed on."""
        buf = (_lib.ScanHitC * max(int(max_hits), 1))()
        n, f = C.c_int(), C.c_int64()
        self._call("get_scan_hits", int(vid), C.cast(buf, C.c_void_p), int(max_hits), C.byref(n), C.byref(f))
        return [_scan.hit_dict(buf[k]) for k in range(n.value)], f.value

    def scan_cells(self, vid: int) -> tuple[np.ndarray, int]:
        """``(cells, frame)``: the C = 8192 / cell_bins cell powers (float64, display order) of that evaluation."""
        cells = np.zeros(_lib.SPECTRUM_BINS, np.float64)
        f = C.c_int64()
        self._call("get_scan_cells", int(vid), cells.ctypes.data, C.byref(f))
        return cells[:_lib.SPECTRUM_BINS // self._scan_cell_bins(int(vid))].copy(), f.value

    def _scan_cell_bins(self, vid: int) -> int:
        # the width this wrapper last set for the leaf's source (the C call returns C doubles and leaves C to its caller)
        return self._scan_w.get(self.descs[vid].parent, 1)

    # -- retuning between frames (on a group: on every member that holds the VFO) -------------------------------------------
    def set_mixer_freqs(self, vids, freqs) -> None:
        """VFO vids[k] mixes with a fresh oscillator at freqs[k] Hz from the next frame on; every filter state is kept."""
        ids, vals = self._set_list("set_mixer_freqs", vids, (freqs, np.float64))
        for i, f in zip(ids.tolist(), vals.tolist()):
            self.descs[i] = dataclasses.replace(self.descs[i], mixer_freq=f)

    def set_gains(self, vids, gains) -> None:
        """vfo::setGain of VFO vids[k] between two frames: from the next frame on."""
        ids, vals = self._set_list("set_gains", vids, (gains, np.float32))
        for i, g in zip(ids.tolist(), vals.tolist()):
            self.descs[i] = dataclasses.replace(self.descs[i], gain=g)


class Receiver(_LeafCalls):
    """One libsdrx context: a VFO tree on one GPU."""

    def __init__(self, device: int = 0, exact: bool = True, keep_prequant: bool = False, segments: int = 0,
                 dc_blocked_scan: bool = False, pipeline: bool = False, fuse: bool = True, frame_pipeline: bool = True,
                 fuse_late: bool = True, keep_streams: bool = False, dc_speculative: bool = True,
                 dc_blocks_per_step: int | None = None, fuse_demod: bool = False,
                 tail_in_levels: bool = True, meter: bool = False, squelch: bool = False, preroll: bool = False,
                 squelch_auto: bool = False, park: bool = False, watch: bool = False, catchup: bool = False,
                 agc: bool = False, wake: bool = False, adc_meter: bool = False, input_rate: int | None = None,
                 resample_taps=32, resample_atten_db: float = 80.0, front_stages: int = 0, front_real: bool = False,
                 front_taps=15, front_atten_db: float = 80.0, blanker=None, iq_balance=None, shift=None, notch=None):
        # notch: the spur canceller in front of the shift (sdrreceiver_amd.notch) -- a notch.Cfg (increments and max_pull in inc
        # units), or a dict of set_notch's keywords (hz=[...], max_pull_hz=..: converted at finalize); None: off.
        self._notch = notch
        # shift: the frequency shift at the end of the ingest chain (sdrreceiver_amd.shift) -- a number is Hz at the tree's rate
        # (mix_offset's Hz; converted at finalize), a shift.Cfg or an (inc[, phase0]) tuple the 32-bit words themselves; None: off.
        self._shift = None if shift is None else _shift.Cfg(*shift) if isinstance(shift, (tuple, list)) else shift
        # iq_balance: the IQ balance correction's settings (sdrreceiver_amd.iqbal.Cfg, or a (mu, min_power[, c0, d0]) tuple) -- the
        # stage cancels a direct-conversion front end's image in the frame behind the format conversion and the DC removal, in
        # front of the blanker; None: off.
        self._iq_balance = None if iq_balance is None else _iqbal.Cfg(*iq_balance) if isinstance(iq_balance, (tuple, list)) else iq_balance
        # blanker: the impulse blanker's settings (sdrreceiver_amd.blank.Cfg, or a (ratio, floor, rank_q16, guard) tuple) -- the
        # stage zeroes pulses in the frame behind the format conversion and in front of everything else; None: off.
        self._blanker = None if blanker is None else _blank.Cfg(*blanker) if isinstance(blanker, (tuple, list)) else blanker
        # front_stages: 1 .. 3 half-band decimations by 2 in front of the resampler (or of level 0) -- frames then have
        # front["in_frame"] samples (sdrreceiver_amd.front).  front_real: the first stage reads REAL samples (process_fmt with
        # fmt=ingest.RS16 or ingest.RU12).  front_taps: K of the built-in design (N = 4 K + 3 taps) with front_atten_db, or the
        # caller's own prototype.  With both, input_rate stays the rate at the resampler's input: behind the front stage.
        self._front_stages, self._front_real = int(front_stages), bool(front_real)
        self._front_taps, self._front_atten = front_taps, float(front_atten_db)
        # input_rate: the front end's sample rate where it is not the parent-less VFOs' fs -- frames then have
        # resampler["in_frame"] samples and a rational resampler on the device makes the tree's frame (sdrreceiver_amd.resample).
        # resample_taps: the taps per phase of the built-in design with resample_atten_db, or the caller's own L * T prototype.
        self._input_rate, self._resample_taps, self._resample_atten = input_rate, resample_taps, float(resample_atten_db)
        self._passband_hz = 0.0
        self.L = _lib.lib()
        h = C.c_void_p()
        rc = self.L.sdrx_create(C.byref(h), int(device))
        if rc != 0:
            raise SdrxError(rc, self.L.sdrx_last_error(None).decode())
        self.h = h
        self.descs: list[VfoDesc] = []
        self._scan_w: dict[int, int] = {}  # source -> the cell width last set through this object (scan_cells trims to it)
        self.published: list[tuple[bytes, int, bytes]] = []
        self._cb = _lib.PUBLISH_FN(self._on_publish)
        self._chk(self.L.sdrx_set_publish_callback(self.h, self._cb, None))
        self._chk(self.L.sdrx_set_option(self.h, b"exact", arithmetic(exact)))
        self._chk(self.L.sdrx_set_option(self.h, b"keep_prequant", int(bool(keep_prequant))))
        self._chk(self.L.sdrx_set_option(self.h, b"segments", int(segments)))
        self._chk(self.L.sdrx_set_option(self.h, b"dc_blocked_scan", int(bool(dc_blocked_scan))))
        self._chk(self.L.sdrx_set_option(self.h, b"pipeline", int(bool(pipeline))))
        self._chk(self.L.sdrx_set_option(self.h, b"fuse", int(bool(fuse))))
        self._chk(self.L.sdrx_set_option(self.h, b"frame_pipeline", int(bool(frame_pipeline))))
        self._chk(self.L.sdrx_set_option(self.h, b"fuse_late", int(bool(fuse_late))))
        self._chk(self.L.sdrx_set_option(self.h, b"keep_streams", int(bool(keep_streams))))
        self._chk(self.L.sdrx_set_option(self.h, b"fuse_demod", int(bool(fuse_demod))))
        self._chk(self.L.sdrx_set_option(self.h, b"tail_in_levels", int(bool(tail_in_levels))))
        self._chk(self.L.sdrx_set_option(self.h, b"meter", int(bool(meter))))
        if squelch:  # (off is the library's default: a library without the option is never asked)
            self._chk(self.L.sdrx_set_option(self.h, b"squelch", 1))
        if preroll:
            self._chk(self.L.sdrx_set_option(self.h, b"preroll", 1))
        if squelch_auto:
            self._chk(self.L.sdrx_set_option(self.h, b"squelch_auto", 1))
        if park:
            self._chk(self.L.sdrx_set_option(self.h, b"park", 1))
        if watch:
            self._chk(self.L.sdrx_set_option(self.h, b"watch", 1))
        if catchup:
            self._chk(self.L.sdrx_set_option(self.h, b"catchup", 1))
        if agc:
            self._chk(self.L.sdrx_set_option(self.h, b"agc", 1))
        if wake:
            self._chk(self.L.sdrx_set_option(self.h, b"wake", 1))
        if adc_meter:
            self._chk(self.L.sdrx_set_option(self.h, b"adc_meter", 1))
        self._chk(self.L.sdrx_set_option(self.h, b"dc_speculative", int(bool(dc_speculative))))
        if dc_blocks_per_step is not None:
            self._chk(self.L.sdrx_set_option(self.h, b"dc_blocks_per_step", int(dc_blocks_per_step)))
        self.finalized = False

    # -- plumbing -----------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            raise SdrxError(rc, self.L.sdrx_last_error(self.h).decode())

    def _on_publish(self, user, topic, rate, buf, length):
        self.published.append((C.string_at(topic, 5), int(rate), C.string_at(buf, length)))

    def set_publish(self, enabled: bool) -> None:
        """Install / remove the per-leaf publish callback (a ctypes callback costs microseconds per
        leaf: a C or C++ host pays nanoseconds)."""
        self._chk(self.L.sdrx_set_publish_callback(self.h, self._cb if enabled else _lib.PUBLISH_FN(0), None))

    def close(self):
        if getattr(self, "h", None):
            self.L.sdrx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration --------------------------------------------------------------
    def add_vfo(self, d: VfoDesc) -> int:
        c = _lib.desc_to_c(d)
        out = C.c_int(-1)
        self._chk(self.L.sdrx_add_vfo(self.h, C.byref(c), C.byref(out)))
        self.descs.append(d)
        if d.detector:
            self.set_detector(out.value, d.detector)
        if len(d.post_taps):
            self.set_postfilter(out.value, d.post_taps, d.post_decim)
        return out.value

    def set_detector(self, vid: int, kind: int) -> None:
        """Before finalize: leaf `vid` (``demod_usb`` False) leaves as an AM envelope (1) or an FM discriminator (2) in int16
        instead of compress()'s bytes (sdrreceiver_amd.detect); 0 takes the detector away."""
        cfg = _lib.DetectCfgC(kind=int(kind))
        self._chk(self.L.sdrx_set_detector(self.h, int(vid), C.byref(cfg)))
        if 0 <= vid < len(self.descs):
            self.descs[vid] = dataclasses.replace(self.descs[vid], detector=int(kind))

    def detector(self, vid: int) -> int:
        """The detector kind of VFO `vid` (0 none, 1 AM, 2 FM)."""
        cfg = _lib.DetectCfgC()
        self._chk(self.L.sdrx_get_detector(self.h, int(vid), C.byref(cfg)))
        return int(cfg.kind)

    def set_postfilter(self, vid: int, taps, decim: int = 1) -> None:
        """Before finalize: detector leaf `vid` leaves through a FIR of `taps` (float32, 1 .. 256) over the detector's floats,
        decimated by `decim` (1 .. 16): n / decim int16 per frame (sdrreceiver_amd.postdet).  No taps (None or empty) take the
        filter away."""
        h = np.ascontiguousarray(() if taps is None else taps, dtype=np.float32).reshape(-1)
        cfg = _lib.PostfilterCfgC(decim=int(decim) if h.size else 0, ntaps=int(h.size))
        self._chk(self.L.sdrx_set_postfilter(self.h, int(vid), C.byref(cfg), h.ctypes.data if h.size else None))
        if 0 <= vid < len(self.descs):
            self.descs[vid] = dataclasses.replace(self.descs[vid], post_taps=tuple(h.tolist()), post_decim=int(decim) if h.size else 1)

    def postfilter(self, vid: int) -> dict:
        """The post-detection filter of VFO `vid`: :func:`sdrreceiver_amd.postdet.info_dict` plus ``taps`` (float32).  SdrxError
        (SDRX_ESTATE) for a node without one."""
        info = _lib.PostfilterInfoC()
        h = np.zeros(postdet.MAX_TAPS, np.float32)
        self._chk(self.L.sdrx_get_postfilter(self.h, int(vid), C.byref(info), h.ctypes.data, h.size))
        out = postdet.info_dict(info)
        out["taps"] = h[:info.ntaps].copy()
        return out

    def finalize(self):
        if self._input_rate:
            self._set_resampler()
        if self._front_stages:
            self._set_front()
        if self._blanker is not None:
            self.set_blanker(self._blanker)
        if self._iq_balance is not None:
            self.set_iq_balance(self._iq_balance)
        if self._shift is not None:
            if isinstance(self._shift, _shift.Cfg):
                self.set_shift(inc=self._shift.inc, phase=self._shift.phase0)
            else:
                self.set_shift(hz=float(self._shift))
        if self._notch is not None:
            if isinstance(self._notch, _notch.Cfg):
                self._set_notch_cfg(self._notch)
            else:
                self.set_notch(**self._notch)
        self._chk(self.L.sdrx_finalize(self.h))
        self.finalized = True

    def _set_resampler(self) -> None:
        fs_in, fs_out = int(self._input_rate), next(d.fs for d in self.descs if d.parent < 0)
        if np.ndim(self._resample_taps) == 0:  # taps per phase: the library's own design
            T = int(self._resample_taps)
            info = _lib.ResamplerInfoC()
            taps = np.zeros(max(1, _resample.MAX_TAPS), np.float32)
            rc = self.L.sdrx_resampler_design(fs_in, fs_out, T, self._resample_atten, taps.ctypes.data, taps.size, C.byref(info))
            if rc != 0:
                raise SdrxError(rc, self.L.sdrx_last_error(None).decode())
            self._passband_hz = info.passband_hz
        else:
            taps = np.ascontiguousarray(self._resample_taps, dtype=np.float32).reshape(-1)
            L, _ = _resample.ratio(fs_in, fs_out)
            if taps.size % L:
                raise ValueError(f"resample_taps holds {taps.size} floats, no multiple of L = {L}")
            T = taps.size // L
        self._chk(self.L.sdrx_set_resampler(self.h, fs_in, taps.ctypes.data, T))

    def _set_front(self) -> None:
        if np.ndim(self._front_taps) == 0:  # K: the library's own design
            self._chk(self.L.sdrx_set_front(self.h, int(self._front_real), self._front_stages, None, int(self._front_taps), self._front_atten))
        else:
            taps = np.ascontiguousarray(self._front_taps, dtype=np.float32).reshape(-1)
            self._chk(self.L.sdrx_set_front(self.h, int(self._front_real), self._front_stages, taps.ctypes.data, _front.k_of(taps), 0.0))

    @property
    def front(self) -> dict | None:
        """The front stage's ``sdrx_front_info`` as a dict (``tw`` and ``alias_free`` of the built-in design; 0 for the caller's
        own taps) with ``taps``, the prototype as the library holds it; None without ``front_stages``."""
        if not self._front_stages:
            return None
        info = _lib.FrontInfoC()
        taps = np.zeros(_front.MAX_N, np.float32)
        self._chk(self.L.sdrx_get_front(self.h, C.byref(info), taps.ctypes.data, taps.size))
        d = _front.info_dict(info)
        d["taps"] = taps[: d["N"]].copy()
        return d

    def set_blanker(self, cfg) -> None:
        """The impulse blanker's settings (``sdrx_set_blanker``): before :meth:`finalize` this switches the stage on (None: off
        again); afterwards it changes ratio, floor, rank_q16 and guard between two frames."""
        if cfg is None:
            self._chk(self.L.sdrx_set_blanker(self.h, None))
            self._blanker = None
            return
        cfg = _blank.Cfg(*cfg) if isinstance(cfg, (tuple, list)) else cfg
        c = _lib.BlankerCfgC(float(cfg.ratio), float(cfg.floor), int(cfg.rank_q16), int(cfg.guard))
        self._chk(self.L.sdrx_set_blanker(self.h, C.byref(c)))
        self._blanker = cfg

    @property
    def blanker(self) -> dict | None:
        """The blanker's record of the last delivered frame (``sdrx_blanker_record`` as a dict: ``thr_bits``, ``ref_bin``,
        ``next_ref_bin``, ``hits``, ``blanked``, ``runs``, ``carry_in``) with ``cfg``, the settings that frame ran with; None
        without ``blanker``."""
        if self._blanker is None:
            return None
        cfg, rec = _lib.BlankerCfgC(), _lib.BlankerRecordC()
        self._chk(self.L.sdrx_get_blanker(self.h, C.byref(cfg), C.byref(rec)))
        d = _blank.record_dict(rec)
        d["cfg"] = _blank.cfg_of(cfg)
        return d

    def set_iq_balance(self, cfg) -> None:
        """The IQ balance correction's settings (``sdrx_set_iq_balance``): before :meth:`finalize` this switches the stage on
        (None: off again) and sets the pair it starts from; afterwards it changes mu and min_power between two frames, and with
        ``iqbal.IQ_LOAD`` in ``flags`` loads ``c0``, ``d0`` as the pair of the next frame."""
        if cfg is None:
            self._chk(self.L.sdrx_set_iq_balance(self.h, None))
            self._iq_balance = None
            return
        cfg = _iqbal.Cfg(*cfg) if isinstance(cfg, (tuple, list)) else cfg
        c = _lib.IqCfgC(float(cfg.mu), float(cfg.min_power), float(cfg.c0), float(cfg.d0), int(cfg.flags))
        self._chk(self.L.sdrx_set_iq_balance(self.h, C.byref(c)))
        self._iq_balance = cfg

    @property
    def iq_balance(self) -> dict | None:
        """The IQ balance correction's record of the last delivered frame (``sdrx_iq_record`` as a dict: ``measured``,
        ``adapted``, ``rejected``, the pair used and the next one as fp32 bits, the five sums) with ``cfg``, the settings that frame
        ran with; None without ``iq_balance``.  ``iqbal.levels`` turns it into the residual imbalance."""
        if self._iq_balance is None:
            return None
        cfg, rec = _lib.IqCfgC(), _lib.IqRecordC()
        self._chk(self.L.sdrx_get_iq_balance(self.h, C.byref(cfg), C.byref(rec)))
        d = _iqbal.record_dict(rec)
        d["cfg"] = _iqbal.cfg_of(cfg)
        return d

    @property
    def tree_rate(self) -> float:
        """The parent-less VFOs' sample rate: the rate the frequency shift runs at"""
        return float(next(d.fs for d in self.descs if d.parent < 0))

    def set_shift(self, hz: float | None = None, inc: int | None = None, phase: int | None = None, off: bool = False) -> None:
        """The frequency shift's settings (``sdrx_set_shift``): ``hz`` at the tree's rate (``shift.inc_of``) or ``inc``, the
        32-bit increment itself.  Before :meth:`finalize` this switches the stage on (``off=True``: off again) and ``phase`` is
        the phase it starts from (default 0); afterwards it changes the increment between two frames -- the phase carries on --
        and a ``phase`` that is not None is loaded as the phase of the next frame (``SDRX_SHIFT_LOAD_PHASE``)."""
        if off:
            self._chk(self.L.sdrx_set_shift(self.h, None))
            self._shift = None
            return
        if (hz is None) == (inc is None):
            raise ValueError("set_shift takes hz or inc")
        word = _shift.inc_of(self.tree_rate, hz) if inc is None else int(inc) & _shift.M32
        flags = _shift.LOAD_PHASE if phase is not None and self.finalized else 0
        c = _lib.ShiftCfgC(word, int(phase or 0) & _shift.M32, flags)
        self._chk(self.L.sdrx_set_shift(self.h, C.byref(c)))
        self._shift = _shift.Cfg(word, int(phase or 0) & _shift.M32, flags)

    @property
    def shift(self) -> dict | None:
        """The frequency shift's record of the last delivered frame (``sdrx_shift_record`` as a dict: the phase and increment the
        frame used, and what it left behind) with ``cfg``, the settings that frame ran with, and ``hz``, its increment in Hz at
        the tree's rate; None without ``shift``."""
        if self._shift is None:
            return None
        cfg, rec = _lib.ShiftCfgC(), _lib.ShiftRecordC()
        self._chk(self.L.sdrx_get_shift(self.h, C.byref(cfg), C.byref(rec)))
        d = _shift.record_dict(rec)
        d["cfg"] = _shift.cfg_of(cfg)
        d["hz"] = _shift.hz_of(self.tree_rate, d["inc"])
        return d

    def _set_notch_cfg(self, cfg) -> None:
        c = _lib.NotchCfgC(n_tones=cfg.n_tones, flags=int(cfg.flags), max_pull=int(cfg.max_pull), mu=float(cfg.mu), afc_gain=float(cfg.afc_gain),
                           min_coherence=float(cfg.min_coherence))
        for k, v in enumerate(cfg.inc0):
            c.inc0[k] = int(v)
        self._chk(self.L.sdrx_set_notch(self.h, C.byref(c)))
        self._notch = cfg if cfg.n_tones or self.finalized else None

    def set_notch(self, hz=None, inc=None, mu: float | None = None, afc_gain: float | None = None, min_coherence: float | None = None,
                  max_pull_hz: float | None = None, max_pull: int | None = None, load: bool = False, off: bool = False) -> None:
        """The spur canceller's settings (``sdrx_set_notch``): the tones as ``hz`` at the tree's rate (``shift.inc_of``) or as
        ``inc``, the 32-bit increments themselves; the loop gain ``mu``, the frequency loop's ``afc_gain`` (0 holds the
        frequencies) and its gate ``min_coherence``; how far a tone may move from where it was given, ``max_pull_hz`` (or
        ``max_pull`` in increment units).  No defaults: the first call names them all; a later call keeps what it does not name.
        Before :meth:`finalize` this switches the stage on (``off=True``: off again); afterwards it changes the settings between
        two frames -- a tone whose increment is unchanged keeps its state, a new or moved one starts afresh, ``load=True``
        restarts all."""
        if off:
            self._chk(self.L.sdrx_set_notch(self.h, None))
            self._notch = None
            return
        old = self._notch if isinstance(self._notch, _notch.Cfg) else None
        if hz is not None and inc is not None:
            raise ValueError("set_notch takes hz or inc")
        if len(hz if hz is not None else inc if inc is not None else ()) > _notch.MAX:
            raise ValueError("set_notch: at most 8 tones")
        words = tuple(_shift.inc_of(self.tree_rate, v) for v in hz) if hz is not None else tuple(int(v) & _shift.M32 for v in inc) if inc is not None else \
            old.inc0 if old else None
        if max_pull_hz is not None:
            if not 0 <= float(max_pull_hz) <= self.tree_rate / 2:
                raise ValueError("set_notch: max_pull_hz lies in 0 .. half the tree's rate")
            max_pull = _shift.inc_of(self.tree_rate, float(max_pull_hz))
        vals = [words, mu, afc_gain, min_coherence, max_pull]
        if old:
            vals = [v if v is not None else o for v, o in zip(vals, (old.inc0, old.mu, old.afc_gain, old.min_coherence, old.max_pull))]
        if any(v is None for v in vals):
            raise ValueError("set_notch: the first call names the tones, mu, afc_gain, min_coherence and max_pull_hz (no defaults)")
        self._set_notch_cfg(_notch.Cfg(vals[0], float(vals[1]), float(vals[2]), float(vals[3]), int(vals[4]), _notch.LOAD if load else 0))

    @property
    def notch(self) -> dict | None:
        """The spur canceller's record of the last delivered frame (``sdrx_notch_record`` as a dict, ``tones`` a list of eight) with
        ``cfg``, the settings as last written, and ``levels`` (``notch.levels``: per tone the tracked Hz, the amplitude, the
        coherence, the depth figure and the lock flags); None without ``notch``."""
        if self._notch is None:
            return None
        cfg, rec = _lib.NotchCfgC(), _lib.NotchRecordC()
        self._chk(self.L.sdrx_get_notch(self.h, C.byref(cfg), C.byref(rec)))
        d = _notch.record_dict(rec)
        d["cfg"] = _notch.cfg_of(cfg)
        d["levels"] = _notch.levels(d, self.tree_rate)
        return d

    def blanker_input(self) -> np.ndarray:
        """The last frame as it reached the blanker: after the format conversion and the DC-bias removal, natural order."""
        n = self.front["in_frame"] if self._front_stages else self.resampler["in_frame"] if self._input_rate else \
            next(d.samples_per_buffer for d in self.descs if d.parent < 0)
        out = np.zeros(2 * max(n, 1), np.float32)
        self._chk(self.L.sdrx_get_blanker_input(self.h, out.ctypes.data, n))
        return out[: 2 * n].view(np.complex64).copy()

    @property
    def resampler(self) -> dict | None:
        """The resampler's ``sdrx_resampler_info`` as a dict (``passband_hz`` of the built-in design; 0 for the caller's own
        taps) with ``taps``, the prototype as the library holds it; None without ``input_rate``."""
        if not self._input_rate:
            return None
        info = _lib.ResamplerInfoC()
        taps = np.zeros(_resample.MAX_TAPS, np.float32)
        self._chk(self.L.sdrx_get_resampler(self.h, C.byref(info), taps.ctypes.data, taps.size))
        d = _resample.info_dict(info)
        d["passband_hz"] = self._passband_hz
        d["taps"] = taps[: d["L"] * d["taps_per_phase"]].copy()
        return d

    def resampler_input(self) -> np.ndarray:
        """The last frame at the input rate as the resampler read it: after the format conversion and the DC-bias removal."""
        n = self.resampler["in_frame"]
        out = np.zeros(2 * max(n, 1), np.float32)
        self._chk(self.L.sdrx_get_resampler_input(self.h, out.ctypes.data, n))
        return out[: 2 * n].view(np.complex64).copy()

    @classmethod
    def from_topology(cls, topo: Topology, **kw) -> "Receiver":
        r = cls(**kw)
        for d in topo.vfos:
            r.add_vfo(d)
        r.finalize()
        return r

    # -- per frame ----------------------------------------------------------------------
    def process(self, iq) -> None:
        """One frame of interleaved float32 I/Q on the host (sdrj::demodData's argument)."""
        iq = np.ascontiguousarray(iq, dtype=np.float32).reshape(-1)
        self.published.clear()
        self._chk(self.L.sdrx_process(self.h, iq.ctypes.data, iq.size // 2))

    def process_u8(self, iq_bytes, correct_dc: bool = False) -> None:
        """One frame of raw dongle bytes (I,Q unsigned, offset 127), LUT + optional DC-bias IIR on the
        device (sdrj::readyRead + demodData, sdrj.cpp:149-165,271-286)."""
        b = np.ascontiguousarray(iq_bytes, dtype=np.uint8).reshape(-1)
        self.published.clear()
        self._chk(self.L.sdrx_process_u8(self.h, b.ctypes.data, b.size // 2, int(bool(correct_dc))))

    def process_fmt(self, iq, correct_dc: bool = False, fmt=None) -> None:
        """One frame of integer samples on the host in one of the formats of :mod:`sdrreceiver_amd.ingest` (dongle bytes,
        int8, int16; `fmt` None: the one the array's dtype stands for): conversion + optional DC-bias IIR on the device."""
        a, fmt = ingest.as_samples(iq, fmt)
        self.published.clear()
        self._chk(self.L.sdrx_process_fmt(self.h, a.ctypes.data, a.size if ingest.is_real(fmt) else a.size // 2, fmt, int(bool(correct_dc))))

    def process_device(self, dev_ptr: int, n_complex: int) -> None:
        self.published.clear()  # the payloads of this frame arrive with the next (explicit or implicit) fetch
        self._chk(self.L.sdrx_process_device(self.h, C.c_void_p(dev_ptr), int(n_complex)))

    def process_device_fmt(self, dev_ptr: int, n_complex: int, fmt: int, correct_dc: bool = False) -> None:
        """One frame of integer samples of format `fmt` already in this context's device memory (16-byte aligned), queued
        like :meth:`process_device`."""
        self.published.clear()
        self._chk(self.L.sdrx_process_device_fmt(self.h, C.c_void_p(dev_ptr), int(n_complex), int(fmt), int(bool(correct_dc))))

    def fetch(self) -> None:
        self.published.clear()
        self._chk(self.L.sdrx_fetch(self.h))

    # -- pipelined interface: submit returns at once, wait delivers the oldest undelivered frame ------
    def submit(self, iq) -> None:
        iq = np.ascontiguousarray(iq, dtype=np.float32).reshape(-1)
        self._chk(self.L.sdrx_submit(self.h, iq.ctypes.data, iq.size // 2))

    def submit_u8(self, iq_bytes, correct_dc: bool = False) -> None:
        b = np.ascontiguousarray(iq_bytes, dtype=np.uint8).reshape(-1)
        self._chk(self.L.sdrx_submit_u8(self.h, b.ctypes.data, b.size // 2, int(bool(correct_dc))))

    def submit_device(self, dev_ptr: int, n_complex: int) -> None:
        """One frame of cf32 already in this context's device memory, pipelined like :meth:`submit`.  The frame must be
        complete in the order of the context's stream (:meth:`set_stream`; by default: complete already) and stay untouched
        until :meth:`wait` has delivered it."""
        self._chk(self.L.sdrx_submit_device(self.h, C.c_void_p(dev_ptr), int(n_complex)))

    def submit_fmt(self, iq, correct_dc: bool = False, fmt=None) -> None:
        """:meth:`process_fmt`'s frame, pipelined like :meth:`submit_u8`."""
        a, fmt = ingest.as_samples(iq, fmt)
        self._chk(self.L.sdrx_submit_fmt(self.h, a.ctypes.data, a.size if ingest.is_real(fmt) else a.size // 2, fmt, int(bool(correct_dc))))

    def submit_device_fmt(self, dev_ptr: int, n_complex: int, fmt: int, correct_dc: bool = False) -> None:
        """:meth:`process_device_fmt`'s frame, pipelined like :meth:`submit_device`."""
        self._chk(self.L.sdrx_submit_device_fmt(self.h, C.c_void_p(dev_ptr), int(n_complex), int(fmt), int(bool(correct_dc))))

    def process_shared(self, src: "Receiver") -> None:
        """The frame `src` staged last (same device), once more through THIS tree, without a second upload."""
        self.published.clear()
        self._chk(self.L.sdrx_process_shared(self.h, src.h))

    def submit_shared(self, src: "Receiver") -> None:
        self._chk(self.L.sdrx_submit_shared(self.h, src.h))

    def process_if_same(self, src: "Receiver", iq) -> bool:
        """Like process_shared, but only if `iq` IS the frame `src` staged last (the library compares it byte for byte with
        src's pinned staging copy).  False -- and nothing processed -- when it is not."""
        iq = np.ascontiguousarray(iq, dtype=np.float32).reshape(-1)
        self.published.clear()
        rc = self.L.sdrx_process_if_same(self.h, src.h, iq.ctypes.data, iq.size // 2)
        if rc == _lib.SDRX_DIFFERENT:
            return False
        self._chk(rc)
        return True

    def submit_if_same(self, src: "Receiver", iq) -> bool:
        iq = np.ascontiguousarray(iq, dtype=np.float32).reshape(-1)
        rc = self.L.sdrx_submit_if_same(self.h, src.h, iq.ctypes.data, iq.size // 2)
        if rc == _lib.SDRX_DIFFERENT:
            return False
        self._chk(rc)
        return True

    def wait(self) -> None:
        """Blocks until the oldest undelivered frame's payloads are on the host; `published` then
        holds that frame's messages and output() serves it."""
        self.published.clear()
        self._chk(self.L.sdrx_wait(self.h))

    def in_flight(self) -> int:
        return int(self.L.sdrx_in_flight(self.h))

    def sync(self) -> None:
        self._chk(self.L.sdrx_sync(self.h))

    def set_stream(self, hip_stream: int | None) -> None:
        self._chk(self.L.sdrx_set_stream(self.h, C.c_void_p(hip_stream or 0)))

    # -- results ------------------------------------------------------------------------
    def output_rate(self, vid: int) -> int:
        rate = C.c_uint32()
        self._chk(self.L.sdrx_get_output(self.h, vid, None, None, C.byref(rate)))
        return rate.value

    def stream(self, vid: int, missing_ok: bool = False):
        """decimate[decimateCount] of VFO `vid` after the last frame.  A leaf whose late decimation or whose demodulation runs
        inside the mix wave keeps it only while it is the tap (:meth:`set_tap`) or with ``keep_streams``: SdrxError otherwise,
        or None with `missing_ok`."""
        n = C.c_int()
        rc = self.L.sdrx_get_stream(self.h, vid, None, 0, C.byref(n))
        if rc == _lib.SDRX_ENOSTREAM and missing_ok:
            return None
        self._chk(rc)
        out = np.zeros(2 * max(n.value, 1), np.float32)
        self._chk(self.L.sdrx_get_stream(self.h, vid, out.ctypes.data, n.value, C.byref(n)))
        return out[: 2 * n.value].view(np.complex64).copy()

    def set_tap(self, vid: int) -> None:
        """fftVFOSlot: from the next frame on :meth:`stream` serves VFO `vid` whatever its kind; REPLACES the selection
        (-1: nothing selected)."""
        self._chk(self.L.sdrx_set_tap(self.h, int(vid)))

    def add_tap(self, vid: int) -> None:
        """One more tapped VFO (fftVFOSlot sets emitFFT on every VFO whose topic matches, vfo.cpp:492-509)."""
        self._chk(self.L.sdrx_add_tap(self.h, int(vid)))

    def set_taps(self, vids) -> None:
        """The selection becomes exactly `vids`."""
        self.set_tap(-1)
        for v in vids:
            self.add_tap(v)

    def raw(self) -> np.ndarray:
        """The raw frame as the main VFOs consumed it (after the byte LUT / DC-bias removal)."""
        out = np.zeros(2 * self.root_frame(), np.float32)
        n = C.c_int()
        self._chk(self.L.sdrx_get_raw(self.h, out.ctypes.data, out.size // 2, C.byref(n)))
        return out[: 2 * n.value].view(np.complex64).copy()

    def root_frame(self) -> int:
        return max(d.samples_per_buffer for d in self.descs if d.parent < 0)

    def prequant(self, vid: int) -> np.ndarray:
        n = C.c_int()
        self._chk(self.L.sdrx_get_prequant(self.h, vid, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.float32)
        self._chk(self.L.sdrx_get_prequant(self.h, vid, out.ctypes.data, n.value, C.byref(n)))
        return out[: n.value].copy()

    def taps(self, vid: int, which: str) -> np.ndarray:
        w = {"fir_usb": 0, "fir_dec": 1, "hilbert": 2}[which]
        n = C.c_int()
        self._chk(self.L.sdrx_get_taps(self.h, vid, w, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.float32)
        self._chk(self.L.sdrx_get_taps(self.h, vid, w, out.ctypes.data, n.value, C.byref(n)))
        return out[: n.value].copy()

    def nco(self, vid: int, first: int, count: int) -> np.ndarray:
        out = np.zeros(2 * max(count, 1), np.float32)
        self._chk(self.L.sdrx_get_nco(self.h, vid, first, count, out.ctypes.data))
        return out[: 2 * count].view(np.complex64).copy()

    # -- spectrum display (MainWindow::fftHandlerSlot on the device) ---------------------------------------------
    def set_spectrum(self, vid: int, on: bool = True) -> None:
        """Enable (and zero: the GUI's combo-box reset) or release the spectrum of VFO `vid`, or of the raw frame with
        ``SPECTRUM_RAW``."""
        self._chk(self.L.sdrx_set_spectrum(self.h, int(vid), int(bool(on))))

    def spectrum(self, vid: int) -> dict:
        """The display state after the last frame: ``pwr`` (8192 float64), ``smooth`` (8182), ``bins`` (the last update's
        FFT output, complex64, natural order), ``maxval``, ``aveval``, ``updates``, ``n_in``."""
        info = _lib.SpectrumInfoC()
        pwr = np.zeros(_lib.SPECTRUM_BINS, np.float64)
        smooth = np.zeros(_lib.SPECTRUM_BINS - 10, np.float64)
        bins = np.zeros(2 * _lib.SPECTRUM_BINS, np.float32)
        self._chk(self.L.sdrx_get_spectrum(self.h, int(vid), C.byref(info), pwr.ctypes.data, smooth.ctypes.data,
                                           bins.ctypes.data))
        return {"pwr": pwr, "smooth": smooth, "bins": bins.view(np.complex64), "maxval": info.maxval,
                "aveval": info.aveval, "updates": info.updates, "n_in": info.n_in}

    def spectrum_levels(self, vids) -> dict:
        """maxval / aveval / updates of many spectra in one small copy: arrays in the order of `vids`."""
        ids = np.ascontiguousarray(vids, dtype=np.int32).reshape(-1)
        mx, av = np.zeros(ids.size, np.float64), np.zeros(ids.size, np.float64)
        up = np.zeros(ids.size, np.int64)
        self._chk(self.L.sdrx_get_spectrum_levels(self.h, ids.ctypes.data, ids.size, mx.ctypes.data, av.ctypes.data,
                                                  up.ctypes.data))
        return {"maxval": mx, "aveval": av, "updates": up}

    # -- measurement -----------------------------------------------------------------------
    def stats(self) -> dict:
        s = _lib.StatsC()
        self._chk(self.L.sdrx_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def enable_kernel_timing(self, on: bool) -> None:
        self._chk(self.L.sdrx_enable_kernel_timing(self.h, int(on)))

    def kernel_times(self) -> dict:
        ms = (C.c_double * _lib.NKERNELS)()
        n = (C.c_int64 * _lib.NKERNELS)()
        b = (C.c_int64 * _lib.NKERNELS)()
        self._chk(self.L.sdrx_get_kernel_times(self.h, ms, n, b))
        return {self.L.sdrx_kernel_name(k).decode(): {"ms": ms[k], "launches": n[k], "alg_bytes": b[k]}
                for k in range(_lib.NKERNELS) if n[k]}


class Group(_LeafCalls):
    """One VFO tree on several GPUs from this one process (``sdrx_group_*``): one context per entry of
    `devices` (a device may be named twice: two shards on one GPU), sub VFOs block-partitioned per
    main VFO, the raw frame fanned out from the first device by peer-to-peer copies.  Ids are those of
    the whole tree; `published` holds the last delivered frame's messages in the reference's order."""

    _prefix = "sdrx_group_"

    def __init__(self, devices, exact: bool = True, **options):
        # (`options`: the library's option names as keywords -- meter=1, squelch=1, preroll=1, squelch_auto=1, ...)
        self.L = _lib.lib()
        h = C.c_void_p()
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        rc = self.L.sdrx_group_create(C.byref(h), arr, len(devices))
        if rc != 0:
            raise SdrxError(rc, self.L.sdrx_group_last_error(None).decode())
        self.h = h
        self.devices = list(devices)
        self.descs: list[VfoDesc] = []
        self._scan_w: dict[int, int] = {}  # source -> the cell width last set through this object (scan_cells trims to it)
        self.published: list[tuple[bytes, int, bytes]] = []
        self._cb = _lib.PUBLISH_FN(lambda user, topic, rate, buf, length: self.published.append(
            (C.string_at(topic, 5), int(rate), C.string_at(buf, length))))
        self._chk(self.L.sdrx_group_set_publish_callback(self.h, self._cb, None))
        self._chk(self.L.sdrx_group_set_option(self.h, b"exact", arithmetic(exact)))
        for k, v in options.items():
            self._chk(self.L.sdrx_group_set_option(self.h, k.encode(), int(v)))

    def _chk(self, rc):
        if rc != 0:
            raise SdrxError(rc, self.L.sdrx_group_last_error(self.h).decode())

    @classmethod
    def from_topology(cls, topo: Topology, devices, **kw) -> "Group":
        g = cls(devices, **kw)
        for d in topo.vfos:
            if d.detector or len(d.post_taps):
                raise ValueError("groups do not offer detector leaves (include/sdrx.h \"Detector leaves\")")
            c = _lib.desc_to_c(d)
            out = C.c_int(-1)
            g._chk(g.L.sdrx_group_add_vfo(g.h, C.byref(c), C.byref(out)))
            g.descs.append(d)
        g._chk(g.L.sdrx_group_finalize(g.h))
        return g

    def process(self, iq) -> None:
        iq = np.ascontiguousarray(iq, dtype=np.float32).reshape(-1)
        self.published.clear()
        self._chk(self.L.sdrx_group_process(self.h, iq.ctypes.data, iq.size // 2))

    def submit(self, iq) -> None:
        iq = np.ascontiguousarray(iq, dtype=np.float32).reshape(-1)
        self._chk(self.L.sdrx_group_submit(self.h, iq.ctypes.data, iq.size // 2))

    def submit_u8(self, iq_bytes, correct_dc: bool = False) -> None:
        b = np.ascontiguousarray(iq_bytes, dtype=np.uint8).reshape(-1)
        self._chk(self.L.sdrx_group_submit_u8(self.h, b.ctypes.data, b.size // 2, int(bool(correct_dc))))

    def process_u8(self, iq_bytes, correct_dc: bool = False) -> None:
        b = np.ascontiguousarray(iq_bytes, dtype=np.uint8).reshape(-1)
        self.published.clear()
        self._chk(self.L.sdrx_group_process_u8(self.h, b.ctypes.data, b.size // 2, int(bool(correct_dc))))

    def submit_fmt(self, iq, correct_dc: bool = False, fmt=None) -> None:
        """Integer samples of any format of :mod:`sdrreceiver_amd.ingest`: the integers are fanned out, every member converts."""
        a, fmt = ingest.as_samples(iq, fmt)
        self._chk(self.L.sdrx_group_submit_fmt(self.h, a.ctypes.data, a.size // 2, fmt, int(bool(correct_dc))))

    def process_fmt(self, iq, correct_dc: bool = False, fmt=None) -> None:
        a, fmt = ingest.as_samples(iq, fmt)
        self.published.clear()
        self._chk(self.L.sdrx_group_process_fmt(self.h, a.ctypes.data, a.size // 2, fmt, int(bool(correct_dc))))

    def peer_access(self) -> bool:
        """True: every member reaches the first device's frame directly (same device or xGMI peer access)."""
        return bool(self.L.sdrx_group_peer_access(self.h))

    def member_context(self, k: int):
        ctx, dev = C.c_void_p(), C.c_int()
        self._chk(self.L.sdrx_group_member(self.h, k, C.byref(ctx), C.byref(dev)))
        return ctx, dev.value

    def stream(self, vid: int, missing_ok: bool = False):
        """decimate[decimateCount] of VFO `vid` (an id of the whole tree) from the member that holds it."""
        m, lid = self.locate(vid)
        ctx, _ = self.member_context(m)
        n = C.c_int()
        rc = self.L.sdrx_get_stream(ctx, lid, None, 0, C.byref(n))
        if rc == _lib.SDRX_ENOSTREAM and missing_ok:
            return None
        if rc != 0:
            raise SdrxError(rc, self.L.sdrx_last_error(ctx).decode())
        out = np.zeros(2 * max(n.value, 1), np.float32)
        rc = self.L.sdrx_get_stream(ctx, lid, out.ctypes.data, n.value, C.byref(n))
        if rc != 0:
            raise SdrxError(rc, self.L.sdrx_last_error(ctx).decode())
        return out[: 2 * n.value].view(np.complex64).copy()

    def submit_device(self, dev_ptr: int, n_complex: int, producer_stream: int | None = None) -> None:
        """One frame of cf32 already on the first device, pipelined like :meth:`submit`.  The frame must be complete in the
        order of `producer_stream` (a hipStream_t of that device, e.g. ``torch.cuda.Stream().cuda_stream``; None: complete
        already) and stay untouched until :meth:`wait` has delivered it."""
        self._chk(self.L.sdrx_group_submit_device(self.h, C.c_void_p(dev_ptr), int(n_complex), C.c_void_p(producer_stream or 0)))

    def process_device(self, dev_ptr: int, n_complex: int, producer_stream: int | None = None) -> None:
        self._chk(self.L.sdrx_group_process_device(self.h, C.c_void_p(dev_ptr), int(n_complex), C.c_void_p(producer_stream or 0)))

    def wait(self) -> None:
        self.published.clear()
        self._chk(self.L.sdrx_group_wait(self.h))

    def sync(self) -> None:
        self._chk(self.L.sdrx_group_sync(self.h))

    def in_flight(self) -> int:
        return int(self.L.sdrx_group_in_flight(self.h))

    def locate(self, vid: int) -> tuple[int, int]:
        m, l = C.c_int(), C.c_int()
        self._chk(self.L.sdrx_group_locate(self.h, vid, C.byref(m), C.byref(l)))
        return m.value, l.value

    def member_stats(self) -> list[dict | None]:
        out = []
        for k in range(len(self.devices)):
            ctx, dev = C.c_void_p(), C.c_int()
            self._chk(self.L.sdrx_group_member(self.h, k, C.byref(ctx), C.byref(dev)))
            if not ctx.value:
                out.append(None)
                continue
            s = _lib.StatsC()
            self.L.sdrx_get_stats(ctx, C.byref(s))
            out.append({k2: getattr(s, k2) for k2, _ in s._fields_})
        return out

    def close(self):
        if getattr(self, "h", None):
            self.L.sdrx_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# =============================================================================================
# The reference's own names
# =============================================================================================
class vfo:  # noqa: N801  (the reference's class name, vfo.h:11)
    """Mirror of ``class vfo`` (vfo.h:11-116): same setters, ``init`` and ``setVFOs``.  Nodes
    only collect parameters; the tree is instantiated on the GPU by the :class:`sdrj` that
    owns the main VFOs, at its first ``demodData`` (or an explicit ``start``)."""

    def __init__(self):
        self.desc = VfoDesc(gain=float(np.float32(0.01)), demod_usb=True, scalecomp=1)  # vfo.cpp:6-31
        self.children: list[vfo] = []
        self._radio: "sdrj | None" = None
        self._id = -1
        self._init = False
        self.emitFFT = False
        self.fftData = None  # callable(np.ndarray complex64): the Qt signal of vfo.h:46

    def setFs(self, samplerate): self.desc.fs = int(samplerate)
    def setDecimationCount(self, count): self.desc.decimate_count = int(count)
    def setMixerFreq(self, freq): self.desc.mixer_freq = float(freq)
    def getMixerFreq(self): return self.desc.mixer_freq
    def getOutRate(self): return self.desc.out_rate_stage
    def setFilterBandwidth(self, bw): self.desc.filter_bw = int(bw)
    def setGain(self, g): self.desc.gain = float(np.float32(g))
    def setDemodUSB(self, usb): self.desc.demod_usb = bool(usb)
    def getDemodUSB(self): return self.desc.demod_usb
    def setDetector(self, kind): self.desc.detector = int(kind)  # (no counterpart in vfo.h: sdrx_set_detector, 0 none / 1 AM / 2 FM)

    def setPostFilter(self, taps, decim=1):  # (no counterpart in vfo.h: sdrx_set_postfilter on a detector leaf)
        self.desc.post_taps = tuple(np.asarray(() if taps is None else taps, np.float32).reshape(-1).tolist())
        self.desc.post_decim = int(decim) if self.desc.post_taps else 1
    def setCompressonStyle(self, st): self.desc.cstyle = int(st)  # sic
    def setScaleComp(self, scale): self.desc.scalecomp = int(scale)
    def setZmqTopic(self, topic): self.desc.topic = str(topic)
    def setZmqAddress(self, address): self.zmqAddress = str(address)  # socket stays host-side

    def init(self, samplesPerBuffer, bind=True, lateDecimate=0):
        self.desc.samples_per_buffer = int(samplesPerBuffer)
        self.desc.late_decimate = int(lateDecimate)
        self._init = True

    def setVFOs(self, pVFOs):
        self.children = list(pVFOs)

    def fftVFOSlot(self, topic):
        """vfo.cpp:492-509: this VFO's decimate[decimateCount] goes to ``fftData`` after every
        frame while the selected topic is its own."""
        self.emitFFT = str(topic) == self.desc.topic
        if self._radio is not None and self._radio.rx is not None:
            self._radio._sync_taps()  # (a deselected fused leaf stops writing its decimate[0]; several VFOs may share a topic)

    # observation, available once the owning sdrj has started
    def _r(self) -> Receiver:
        if self._radio is None or self._radio.rx is None:
            raise RuntimeError("vfo is not attached to a started sdrj")
        return self._radio.rx

    @property
    def transmit_usb(self): return self._r().output(self._id)
    @property
    def transmit_iq(self): return self._r().output(self._id)
    @property
    def decimate_final(self): return self._r().stream(self._id)
    @property
    def outputRate(self): return self._r().output_rate(self._id)


class sdrj:  # noqa: N801  (the reference's class name, sdrj.h)
    """Mirror of the hot-path part of ``class sdrj``: ``setVFOs`` (sdrj.h) and
    ``demodData(const float*, int)`` (sdrj.cpp:266-305).  ``setDCCorrection`` keeps the DC-bias
    IIR on the host side for float input, exactly where the reference has it."""

    def __init__(self, device: int = 0, exact: bool = True, keep_prequant: bool = False):
        self.mains: list[vfo] = []
        self.rx: Receiver | None = None
        self.correctDC = False
        self._avept = np.zeros(2, np.float32)
        self._kw = dict(device=device, exact=exact, keep_prequant=keep_prequant)
        self.emitFFT = False
        self.count = 0
        self.fftData = None  # callable(np.ndarray complex64): the Qt signal of sdrj.h:40

    def setVFOs(self, vfos): self.mains = list(vfos)
    def setDCCorrection(self, dc): self.correctDC = bool(dc)

    def fftVFOSlot(self, topic):
        """sdrj.cpp:84-101: the raw spectrum is selected by the topic "Main"; any selection
        restarts the every-4th-call counter."""
        self.emitFFT = str(topic) == "Main"
        self.count = 0

    def _all_vfos(self):
        stack = list(self.mains)
        while stack:
            v = stack.pop(0)
            yield v
            stack[0:0] = v.children

    def _sync_taps(self):
        """The library's selection = the VFOs with emitFFT (every VFO whose topic equals the selected string, vfo.cpp:492-509)."""
        self.rx.set_taps([v._id for v in self._all_vfos() if v.emitFFT])

    def _after_frame(self):
        # vfo::process ends with `if (emitFFT) emit fftData(decimate[decimateCount])` (vfo.cpp:290-293),
        # demodData with the every-4th-call raw tap (sdrj.cpp:296-303)
        for v in self._all_vfos():
            if v.emitFFT and v.fftData is not None:
                v.fftData(self.rx.stream(v._id))
        if self.count == 4 and self.emitFFT:
            if self.fftData is not None:
                self.fftData(self.rx.raw())
            self.count = 0
        self.count += 1

    def start(self):
        self.rx = Receiver(**self._kw)

        def add(node: vfo, parent: int):
            if not node._init:
                raise RuntimeError("vfo::init was not called")
            node.desc.parent = parent
            node._id = self.rx.add_vfo(node.desc)
            node._radio = self
            for ch in node.children:
                add(ch, node._id)

        # ids must be assigned parents-first; children of main i come before main i+1's, which
        # is also the reference's publish order (sdrj.cpp:288-294, vfo.cpp:257-263)
        for m in self.mains:
            add(m, -1)
        self.rx.finalize()
        self._sync_taps()  # a selection made before the tree existed (fftVFOSlot, vfo.cpp:492-509)

    def demodData(self, data, length=None):
        if self.rx is None:
            self.start()
        data = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
        if length is not None:
            data = data[: int(length)]
        if self.correctDC:
            data = data.copy()
            _dc_correct(data, self._avept)
        self.rx.process(data)
        self._after_frame()

    def demodBytes(self, data):
        """The rtl_tcp byte stream (sdrj.cpp:155-160 feeds it through the LUT into demodData):
        LUT and DC-bias removal run on the device.  An int8 or int16 array is a wideband front end's samples instead
        (:mod:`sdrreceiver_amd.ingest`); anything else is taken as bytes, as before."""
        if self.rx is None:
            self.start()
        if isinstance(data, np.ndarray) and data.dtype in (np.int8, np.int16):
            self.rx.process_fmt(data, correct_dc=self.correctDC)
        else:
            self.rx.process_u8(np.ascontiguousarray(data, dtype=np.uint8).reshape(-1), correct_dc=self.correctDC)
        self._after_frame()

    @property
    def published(self):
        return self.rx.published if self.rx else []


def _dc_correct(iq: np.ndarray, state: np.ndarray) -> None:
    """sdrj.cpp:277-283 on the host: avept = avept*(1-1e-6) + 1e-6*curr; curr -= avept, in fp32.
    A first-order recursion; evaluated blockwise in closed form is not bit-exact, so this is the
    plain sequential loop the reference runs (the device-side version lives in the library)."""
    keep = np.float32(1.0) - np.float32(0.000001)
    k = np.float32(0.000001)
    ar, ai = np.float32(state[0]), np.float32(state[1])
    re, im = iq[0::2], iq[1::2]
    for i in range(re.size):
        ar = np.float32(np.float32(ar * keep) + np.float32(k * re[i]))
        ai = np.float32(np.float32(ai * keep) + np.float32(k * im[i]))
        re[i] -= ar
        im[i] -= ai
    state[0], state[1] = ar, ai
