"""Per-leaf output meters (option ``meter``): the reference definition, and a gain suggestion built on it.

The library computes the meters on the device where the payload is produced (``sdrx_get_meters``,
:meth:`Receiver.meters`).  :func:`meters_from_payload` restates the same definition in numpy from a leaf's payload
and its pre-quantisation values; the tests hold the device to it exactly.

* USB leaf (int16 audio): ``pre = usb' * gain * 32768.0`` (vfo.cpp:328,364), ``v`` = the int16 on the wire.  The
  conversion truncates and WRAPS, so a sample is counted in ``clipped`` when ``!(pre > -32769.0 and pre < 32768.0)``
  (NaN included): exactly where the emitted short differs from ``trunc(pre)``.
* compress() leaf (int8 IQ, vfo.cpp:389-424): per component ``pre = re * 128`` (cstyle 0) or
  ``(re / scalecomp) * 128`` (cstyle 1), ``v`` = its int8 value before cstyle 1's nibble masking; ``n_values = 2 n``;
  a sample is clipped when either component has ``!(pre > -129 and pre < 128)``.

``sum_sq`` = sum of ``v * v`` (exact), ``peak`` = max ``|pre|`` as float32 (NaN if any ``pre`` was NaN).
"""
from __future__ import annotations

import numpy as np

FULL_SCALE_INT16 = 32768.0
FULL_SCALE_INT8 = 128.0


def wrap_int16(pre) -> np.ndarray:
    """The library's float -> short conversion of ``pre`` (the reference's x86-64 ``short = double``): truncation to
    int32 (INT32_MIN outside int32 or for NaN), low 16 bits kept."""
    p = np.asarray(pre, np.float64)
    ok = (p >= -2147483648.0) & (p < 2147483648.0)
    t = np.where(ok, np.trunc(np.where(ok, p, 0.0)), -2147483648.0).astype(np.int64)
    return (t & 0xFFFF).astype(np.uint16).view(np.int16)


def wrap_int8(pre) -> np.ndarray:
    """``to_schar`` of compress(): the same truncation to int32, low 8 bits kept."""
    p = np.asarray(pre, np.float32).astype(np.float64)
    ok = (p >= -2147483648.0) & (p < 2147483648.0)
    t = np.where(ok, np.trunc(np.where(ok, p, 0.0)), -2147483648.0).astype(np.int64)
    return (t & 0xFF).astype(np.uint8).view(np.int8)


def _peak(pre: np.ndarray) -> np.float32:
    a = np.abs(np.asarray(pre, np.float32).reshape(-1))
    if a.size == 0:
        return np.float32(0.0)
    if np.isnan(a).any():
        return np.float32(np.nan)
    return np.float32(a.max())


def _sum_sq(v: np.ndarray) -> int:
    v = np.asarray(v, np.int64).reshape(-1)
    return int(np.sum(v * v, dtype=np.uint64))


def iq_prequant(desc, stream) -> tuple[np.ndarray, np.ndarray]:
    """compress(): the float32 ``pre`` of both components of a leaf's stream (decimate[d], complex64), as k_compress
    computes them."""
    z = np.asarray(stream, np.complex64).reshape(-1)
    re, im = z.real.astype(np.float32), z.imag.astype(np.float32)
    if int(desc.cstyle) == 1:
        sc = np.float32(desc.scalecomp)
        return (re / sc) * np.float32(128.0), (im / sc) * np.float32(128.0)
    return re * np.float32(128.0), im * np.float32(128.0)


def meters_from_payload(desc, payload, prequant=None) -> dict:
    """The meter of one leaf for one frame.

    USB leaf: `payload` is the int16 output, `prequant` the float32 ``pre`` values (``Receiver(keep_prequant=True)``,
    :meth:`Receiver.prequant`).  compress() leaf: `prequant` is the leaf's complex stream (:meth:`Receiver.stream`),
    from which ``pre`` and ``v`` follow (cstyle 1's payload holds only the high nibbles); `payload` is then unused,
    except that without `prequant` a cstyle 0 payload still gives ``sum_sq``.  Without `prequant`, ``clipped`` and
    ``peak`` are None.  Returns ``n_values``, ``sum_sq``, ``clipped``, ``peak``."""
    if desc.demod_usb:
        v = np.asarray(payload, np.int16).reshape(-1)
        out = {"n_values": int(v.size), "sum_sq": _sum_sq(v), "clipped": None, "peak": None}
        if prequant is not None:
            pre = np.asarray(prequant, np.float32).reshape(-1)
            if pre.size != v.size:
                raise ValueError(f"{pre.size} prequant values for {v.size} payload values")
            with np.errstate(invalid="ignore"):
                out["clipped"] = int(np.count_nonzero(~((pre > -32769.0) & (pre < 32768.0))))
            out["peak"] = _peak(pre)
        return out
    if prequant is None:
        if int(desc.cstyle) == 1:
            raise ValueError("a cstyle 1 payload holds only the high nibbles: pass the leaf's stream as prequant")
        v = np.asarray(payload, np.int8).reshape(-1)
        return {"n_values": int(v.size), "sum_sq": _sum_sq(v), "clipped": None, "peak": None}
    pre_re, pre_im = iq_prequant(desc, prequant)
    v = np.concatenate([wrap_int8(pre_re), wrap_int8(pre_im)])
    with np.errstate(invalid="ignore"):
        ok = (pre_re > -129.0) & (pre_re < 128.0) & (pre_im > -129.0) & (pre_im < 128.0)
    return {"n_values": int(v.size), "sum_sq": _sum_sq(v), "clipped": int(np.count_nonzero(~ok)),
            "peak": _peak(np.concatenate([pre_re, pre_im]))}


def meters_dict(records, is_usb) -> dict:
    """``sdrx_meter`` records (in the order asked for) as arrays, with ``full_scale`` (32768 for int16, 128 for int8)
    and the derived ``rms_dbfs = 20 log10(sqrt(sum_sq / n_values) / full_scale)`` and ``peak_dbfs``."""
    n = len(records)
    d = {
        "frame": np.array([r.frame for r in records], np.int64).reshape(n),
        "n_values": np.array([r.n_values for r in records], np.int64).reshape(n),
        "sum_sq": np.array([r.sum_sq for r in records], np.uint64).reshape(n),
        "clipped": np.array([r.clipped for r in records], np.int64).reshape(n),
        "peak": np.array([r.peak for r in records], np.float32).reshape(n),
        "full_scale": np.where(np.asarray(is_usb, bool).reshape(n), FULL_SCALE_INT16, FULL_SCALE_INT8),
    }
    with np.errstate(divide="ignore", invalid="ignore"):
        rms = np.sqrt(d["sum_sq"].astype(np.float64) / np.maximum(d["n_values"], 1))
        d["rms_dbfs"] = 20.0 * np.log10(rms / d["full_scale"])
        d["peak_dbfs"] = 20.0 * np.log10(d["peak"].astype(np.float64) / d["full_scale"])
    return d


def suggest_gains(gains, meters: dict, target_rms_dbfs: float, max_step_db: float = 6.0,
                  min_rms_lsb: float = 1.0) -> np.ndarray:
    """float32 gains that move each USB leaf's RMS to `target_rms_dbfs`, for ``set_gains`` at the next frame.

    `gains[k]` is the current gain of the leaf `meters` reports at index k (a dict of :meth:`Receiver.meters`).  The
    output scales linearly with the gain, so the step is ``target - rms_dbfs``, capped at +-`max_step_db`.  A leaf
    whose payload wrapped (``clipped > 0``) is never raised: its RMS is that of the wrapped values.  Silent leaves
    (RMS below `min_rms_lsb` LSB) and compress() leaves (the gain does not act on them) keep their gain.

    There is deliberately no default target: what level JAERO's "green volume light" corresponds to has not been
    measured -- choose it for your setup."""
    g = np.asarray(gains, np.float32).reshape(-1).copy()
    full = np.asarray(meters["full_scale"], np.float64)
    if g.size != full.size:
        raise ValueError(f"{g.size} gains for {full.size} meters")
    n = np.maximum(np.asarray(meters["n_values"], np.float64), 1.0)
    rms = np.sqrt(np.asarray(meters["sum_sq"], np.float64) / n)
    usb = full == FULL_SCALE_INT16
    live = usb & (rms >= float(min_rms_lsb))
    with np.errstate(divide="ignore"):
        step = float(target_rms_dbfs) - 20.0 * np.log10(np.where(live, rms, 1.0) / full)
    step = np.clip(step, -float(max_step_db), float(max_step_db))
    step = np.where(np.asarray(meters["clipped"]) > 0, np.minimum(step, 0.0), step)
    scaled = (g.astype(np.float64) * 10.0 ** (step / 20.0)).astype(np.float32)
    return np.where(live, scaled, g).astype(np.float32)
