"""ctypes binding of libsdrx.so (include/sdrx.h).  There is no fallback: if the HIP library is
missing or cannot be loaded this module raises, and without a GPU ``sdrx_create`` fails."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDRX_LIB") or os.path.join(_HERE, "libsdrx.so")  # SDRX_LIB: A/B builds of the SAME HIP library
CSRC = os.path.join(_HERE, "csrc")

NKERNELS = 8
SDRX_EINVAL, SDRX_ESTATE, SDRX_EFILTER, SDRX_EHIP, SDRX_EUNSUPPORTED, SDRX_ENOMEM, SDRX_ENOSTREAM = -1, -2, -3, -4, -5, -6, -7  # include/sdrx.h
SDRX_DIFFERENT = 1  # sdrx_*_if_same: the frame is not the one the source context staged
SPECTRUM_BINS, SPECTRUM_RAW = 8192, -2  # SDRX_SPECTRUM_BINS, SDRX_SPECTRUM_RAW
DRIFT_MAX_SHIFT = 1024  # SDRX_DRIFT_MAX_SHIFT
SCAN_MAX_HITS = 512  # SDRX_SCAN_MAX_HITS


class VfoDescC(C.Structure):
    """struct sdrx_vfo_desc"""
    _fields_ = [
        ("fs", C.c_int32), ("decimate_count", C.c_int32), ("mixer_freq_hz", C.c_double),
        ("demod_usb", C.c_int32), ("late_decimate", C.c_int32), ("filter_bw_hz", C.c_int32),
        ("gain", C.c_float), ("cstyle", C.c_int32), ("scalecomp", C.c_int32), ("parent_id", C.c_int32),
        ("samples_per_buffer", C.c_int32), ("topic", C.c_char * 8),
    ]


def desc_to_c(d) -> VfoDescC:
    """topology.VfoDesc -> struct sdrx_vfo_desc"""
    return VfoDescC(fs=d.fs, decimate_count=d.decimate_count, mixer_freq_hz=float(d.mixer_freq),
                    demod_usb=int(d.demod_usb), late_decimate=d.late_decimate, filter_bw_hz=int(d.filter_bw),
                    gain=float(d.gain), cstyle=d.cstyle, scalecomp=d.scalecomp, parent_id=d.parent,
                    samples_per_buffer=d.samples_per_buffer, topic=d.topic.encode()[:7])


class StatsC(C.Structure):
    """struct sdrx_stats"""
    _fields_ = [
        ("n_vfos", C.c_int32), ("n_leaves", C.c_int32), ("n_levels", C.c_int32), ("exact", C.c_int32),
        ("algorithmic_bytes_per_frame", C.c_int64), ("vfo_samples_per_frame", C.c_int64),
        ("device_bytes", C.c_int64), ("frames", C.c_int64), ("mix_chunks_per_frame", C.c_int64),
        ("dc_blocks", C.c_int64), ("dc_fallback_blocks", C.c_int64), ("dc_retried_blocks", C.c_int64),
    ]


class SpectrumInfoC(C.Structure):
    """struct sdrx_spectrum_info"""
    _fields_ = [("updates", C.c_int64), ("n_in", C.c_int32), ("reserved", C.c_int32),
                ("maxval", C.c_double), ("aveval", C.c_double)]


class MeterC(C.Structure):
    """struct sdrx_meter"""
    _fields_ = [("frame", C.c_int64), ("sum_sq", C.c_uint64), ("n_values", C.c_uint32), ("clipped", C.c_uint32),
                ("peak", C.c_float), ("reserved", C.c_uint32)]


class SquelchStateC(C.Structure):
    """struct sdrx_squelch_state"""
    _fields_ = [("frame", C.c_int64), ("thr_sum_sq", C.c_uint64), ("hang_frames", C.c_uint32), ("hang_left", C.c_uint32),
                ("open", C.c_int32), ("reserved", C.c_uint32)]


class SquelchAutoStateC(C.Structure):
    """struct sdrx_squelch_auto_state"""
    _fields_ = [("frame", C.c_int64), ("floor_sum_sq", C.c_uint64), ("thr_eff_sum_sq", C.c_uint64), ("ratio_q8", C.c_uint32),
                ("window_frames", C.c_uint32), ("floor_valid", C.c_uint32), ("reserved", C.c_uint32)]


class AgcCfgC(C.Structure):
    """struct sdrx_agc_cfg"""
    _fields_ = [("lo_ms", C.c_uint32), ("hi_ms", C.c_uint32), ("silent_ms", C.c_uint32), ("hold_frames", C.c_uint32),
                ("up", C.c_float), ("down", C.c_float), ("gain_min", C.c_float), ("gain_max", C.c_float)]


class AgcStateC(C.Structure):
    """struct sdrx_agc_state"""
    _fields_ = [("frame", C.c_int64), ("gain_used", C.c_float), ("gain_next", C.c_float), ("action", C.c_int32),
                ("quiet_run", C.c_uint32), ("cfg", AgcCfgC)]


class ActiveStateC(C.Structure):
    """struct sdrx_active_state"""
    _fields_ = [("since_frame", C.c_int64), ("active", C.c_int32), ("reserved", C.c_uint32)]


class DriftLevelC(C.Structure):
    """struct sdrx_drift_level"""
    _fields_ = [("frame", C.c_int64), ("peak", C.c_double), ("left", C.c_double), ("right", C.c_double), ("zero", C.c_double),
                ("shift", C.c_int32), ("max_shift", C.c_int32), ("measured", C.c_int32), ("captured", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class ScanCfgC(C.Structure):
    """struct sdrx_scan_cfg"""
    _fields_ = [("cell_bins", C.c_int32), ("frames", C.c_int32), ("floor_permille", C.c_int32), ("ratio_q8", C.c_uint32),
                ("min_cells", C.c_int32), ("reserved", C.c_int32 * 3)]


class ScanHitC(C.Structure):
    """struct sdrx_scan_hit"""
    _fields_ = [("first_cell", C.c_int32), ("n_cells", C.c_int32), ("peak_cell", C.c_int32), ("reserved", C.c_int32),
                ("peak_pwr", C.c_double), ("reserved_d", C.c_double)]


class ScanLevelC(C.Structure):
    """struct sdrx_scan_level"""
    _fields_ = [("frame", C.c_int64), ("floor", C.c_double), ("thr", C.c_double), ("n_hits", C.c_int32), ("n_stored", C.c_int32),
                ("n_hot", C.c_int32), ("integrated", C.c_int32), ("frames", C.c_int32), ("cell_bins", C.c_int32),
                ("measured", C.c_int32), ("complete", C.c_int32), ("reserved", C.c_int32 * 2)]


class WatchLevelC(C.Structure):
    """struct sdrx_watch_level"""
    _fields_ = [("frame", C.c_int64), ("band_pwr", C.c_double), ("total_pwr", C.c_double), ("first_bin", C.c_int32),
                ("n_bins", C.c_int32), ("segments", C.c_int32), ("watched", C.c_int32), ("reserved", C.c_int32 * 2)]


class WakeCfgC(C.Structure):
    """struct sdrx_wake_cfg"""
    _fields_ = [("min_band_pwr", C.c_double), ("contrast_q8", C.c_uint32), ("hold_frames", C.c_uint32), ("on", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class WakeStateC(C.Structure):
    """struct sdrx_wake_state"""
    _fields_ = [("frame", C.c_int64), ("since_frame", C.c_int64), ("active", C.c_int32), ("hot", C.c_int32),
                ("hold_left", C.c_uint32), ("controlled", C.c_int32)]


class AdcArmC(C.Structure):
    """struct sdrx_adc_arm"""
    _fields_ = [("sum", C.c_int64), ("sum_sq", C.c_uint64), ("min", C.c_int32), ("max", C.c_int32), ("at_lo", C.c_uint32),
                ("at_hi", C.c_uint32), ("longest_rail_run", C.c_uint32), ("reserved", C.c_uint32)]


class AdcMeterC(C.Structure):
    """struct sdrx_adc_meter"""
    _fields_ = [("frame", C.c_int64), ("n_complex", C.c_uint32), ("fmt", C.c_int32), ("measured", C.c_uint32),
                ("reserved", C.c_uint32), ("i", AdcArmC), ("q", AdcArmC), ("sum_iq", C.c_int64), ("bits", C.c_uint32 * 17),
                ("reserved2", C.c_uint32)]


class ResamplerInfoC(C.Structure):
    """struct sdrx_resampler_info"""
    _fields_ = [("fs_in", C.c_int32), ("fs_out", C.c_int32), ("L", C.c_int32), ("M", C.c_int32), ("taps_per_phase", C.c_int32),
                ("in_frame", C.c_int32), ("out_frame", C.c_int32), ("reserved", C.c_int32), ("delay_out_samples", C.c_double),
                ("passband_hz", C.c_double)]


class FrontInfoC(C.Structure):
    """struct sdrx_front_info"""
    _fields_ = [("real_input", C.c_int32), ("stages", C.c_int32), ("K", C.c_int32), ("N", C.c_int32), ("in_frame", C.c_int32),
                ("out_frame", C.c_int32), ("reserved", C.c_int32 * 2), ("tw", C.c_double), ("alias_free", C.c_double)]


class BlankerCfgC(C.Structure):
    """struct sdrx_blanker_cfg"""
    _fields_ = [("ratio", C.c_float), ("floor", C.c_float), ("rank_q16", C.c_int32), ("guard", C.c_int32), ("reserved", C.c_int32 * 4)]


class BlankerRecordC(C.Structure):
    """struct sdrx_blanker_record"""
    _fields_ = [("frame", C.c_int64), ("n_complex", C.c_uint32), ("measured", C.c_uint32), ("thr_bits", C.c_uint32), ("ref_bin", C.c_int32),
                ("next_ref_bin", C.c_int32), ("hits", C.c_uint32), ("blanked", C.c_uint32), ("runs", C.c_uint32), ("carry_in", C.c_uint32),
                ("reserved", C.c_uint32 * 5)]


class IqCfgC(C.Structure):
    """struct sdrx_iq_cfg"""
    _fields_ = [("mu", C.c_float), ("min_power", C.c_float), ("c0", C.c_float), ("d0", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class IqRecordC(C.Structure):
    """struct sdrx_iq_record"""
    _fields_ = [("frame", C.c_int64), ("n_complex", C.c_uint32), ("measured", C.c_uint32), ("adapted", C.c_uint32), ("rejected", C.c_uint32),
                ("c_bits", C.c_uint32), ("d_bits", C.c_uint32), ("next_c_bits", C.c_uint32), ("next_d_bits", C.c_uint32), ("sum_i", C.c_int64),
                ("sum_q", C.c_int64), ("sum_iq", C.c_int64), ("sum_ii", C.c_uint64), ("sum_qq", C.c_uint64), ("reserved", C.c_uint32 * 4)]


class ShiftCfgC(C.Structure):
    """struct sdrx_shift_cfg"""
    _fields_ = [("inc", C.c_uint32), ("phase0", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class ShiftRecordC(C.Structure):
    """struct sdrx_shift_record"""
    _fields_ = [("frame", C.c_int64), ("n_complex", C.c_uint32), ("applied", C.c_uint32), ("phase", C.c_uint32), ("inc", C.c_uint32),
                ("next_phase", C.c_uint32), ("next_inc", C.c_uint32), ("reserved", C.c_uint32 * 8)]


class NotchCfgC(C.Structure):
    """struct sdrx_notch_cfg"""
    _fields_ = [("n_tones", C.c_uint32), ("flags", C.c_uint32), ("max_pull", C.c_uint32), ("reserved0", C.c_uint32), ("mu", C.c_float),
                ("afc_gain", C.c_float), ("min_coherence", C.c_float), ("reserved1", C.c_uint32), ("inc0", C.c_uint32 * 8), ("reserved", C.c_uint32 * 8)]


class DetectCfgC(C.Structure):
    """struct sdrx_detect_cfg"""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32 * 3)]


class PostfilterCfgC(C.Structure):
    """struct sdrx_postfilter_cfg"""
    _fields_ = [("decim", C.c_int32), ("ntaps", C.c_int32), ("reserved", C.c_int32 * 2)]


class PostfilterInfoC(C.Structure):
    """struct sdrx_postfilter_info"""
    _fields_ = [("decim", C.c_int32), ("ntaps", C.c_int32), ("out_len", C.c_int32), ("reserved", C.c_int32),
                ("delay_samples", C.c_double), ("pass_hz", C.c_double), ("stop_hz", C.c_double)]


class NotchToneC(C.Structure):
    """struct sdrx_notch_tone"""
    _fields_ = [("inc", C.c_uint32), ("inc_next", C.c_uint32), ("a_re_bits", C.c_uint32), ("a_im_bits", C.c_uint32), ("coherent", C.c_uint32),
                ("adapted", C.c_uint32), ("clamped", C.c_uint32), ("rejected", C.c_uint32), ("s_re", C.c_double), ("s_im", C.c_double),
                ("p", C.c_double), ("e", C.c_double)]


class NotchRecordC(C.Structure):
    """struct sdrx_notch_record"""
    _fields_ = [("frame", C.c_int64), ("n_complex", C.c_uint32), ("n_tones", C.c_uint32), ("blocks", C.c_uint32), ("reserved", C.c_uint32 * 3),
                ("tone", NotchToneC * 8)]


PUBLISH_FN =C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_char), C.c_uint32, C.c_void_p, C.c_uint32)

# every symbol include/sdrx.h declares: (restype, argtypes)
_vp, _i = C.c_void_p, C.c_int
SYMBOLS = {
    "sdrx_abi_version": (_i, []),
    "sdrx_build_id": (C.c_char_p, []),
    "sdrx_create": (_i, [C.POINTER(_vp), _i]),
    "sdrx_destroy": (_i, [_vp]),
    "sdrx_last_error": (C.c_char_p, [_vp]),
    "sdrx_add_vfo": (_i, [_vp, C.POINTER(VfoDescC), C.POINTER(_i)]),
    "sdrx_set_option": (_i, [_vp, C.c_char_p, _i]),
    "sdrx_finalize": (_i, [_vp]),
    "sdrx_set_publish_callback": (_i, [_vp, PUBLISH_FN, _vp]),
    "sdrx_check_vfo": (_i, [C.POINTER(VfoDescC), C.c_char_p, C.c_size_t]),
    "sdrx_process": (_i, [_vp, _vp, _i]),
    "sdrx_process_u8": (_i, [_vp, _vp, _i, _i]),
    "sdrx_process_fmt": (_i, [_vp, _vp, _i, _i, _i]),
    "sdrx_process_device": (_i, [_vp, _vp, _i]),
    "sdrx_submit": (_i, [_vp, _vp, _i]),
    "sdrx_submit_u8": (_i, [_vp, _vp, _i, _i]),
    "sdrx_submit_device": (_i, [_vp, _vp, _i]),
    "sdrx_submit_fmt": (_i, [_vp, _vp, _i, _i, _i]),
    "sdrx_process_device_fmt": (_i, [_vp, _vp, _i, _i, _i]),
    "sdrx_submit_device_fmt": (_i, [_vp, _vp, _i, _i, _i]),
    "sdrx_wait": (_i, [_vp]),
    "sdrx_in_flight": (_i, [_vp]),
    "sdrx_fetch": (_i, [_vp]),
    "sdrx_sync": (_i, [_vp]),
    "sdrx_set_stream": (_i, [_vp, _vp]),
    "sdrx_get_output": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "sdrx_get_stream": (_i, [_vp, _i, _vp, _i, C.POINTER(_i)]),
    "sdrx_set_tap": (_i, [_vp, _i]),
    "sdrx_add_tap": (_i, [_vp, _i]),
    "sdrx_get_raw": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "sdrx_get_prequant": (_i, [_vp, _i, _vp, _i, C.POINTER(_i)]),
    "sdrx_get_taps": (_i, [_vp, _i, _i, _vp, _i, C.POINTER(_i)]),
    "sdrx_get_nco": (_i, [_vp, _i, C.c_long, C.c_long, _vp]),
    "sdrx_set_mixer_freqs": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_set_gains": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_get_meters": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_set_squelch": (_i, [_vp, _vp, _vp, _vp, _i]),
    "sdrx_get_squelch": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_get_egress": (_i, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "sdrx_group_set_squelch": (_i, [_vp, _vp, _vp, _vp, _i]),
    "sdrx_group_get_squelch": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_group_get_egress": (_i, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "sdrx_get_preroll": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)]),
    "sdrx_get_preroll_count": (_i, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "sdrx_group_get_preroll": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)]),
    "sdrx_group_get_preroll_count": (_i, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "sdrx_set_squelch_auto": (_i, [_vp, _vp, _vp, _vp, _i]),
    "sdrx_get_squelch_auto": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_group_set_squelch_auto": (_i, [_vp, _vp, _vp, _vp, _i]),
    "sdrx_group_get_squelch_auto": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_set_agc": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_get_agc": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_group_set_agc": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_group_get_agc": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_set_active": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_get_active": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_group_set_active": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_group_get_active": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_get_catchup": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_group_get_catchup": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_set_watch": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_get_watch": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_get_watch_psd": (_i, [_vp, _i, _vp, C.POINTER(C.c_int64)]),
    "sdrx_group_set_watch": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_group_get_watch": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_group_get_watch_psd": (_i, [_vp, _i, _vp, C.POINTER(C.c_int64)]),
    "sdrx_set_drift": (_i, [_vp, _i, _vp, _i]),
    "sdrx_get_drift": (_i, [_vp, _i, C.POINTER(DriftLevelC)]),
    "sdrx_get_drift_profile": (_i, [_vp, _i, _vp, C.POINTER(C.c_int64)]),
    "sdrx_group_set_drift": (_i, [_vp, _i, _vp, _i]),
    "sdrx_group_get_drift": (_i, [_vp, _i, C.POINTER(DriftLevelC)]),
    "sdrx_group_get_drift_profile": (_i, [_vp, _i, _vp, C.POINTER(C.c_int64)]),
    "sdrx_set_scan": (_i, [_vp, _i, C.POINTER(ScanCfgC)]),
    "sdrx_get_scan": (_i, [_vp, _i, C.POINTER(ScanLevelC)]),
    "sdrx_get_scan_hits": (_i, [_vp, _i, _vp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "sdrx_get_scan_cells": (_i, [_vp, _i, _vp, C.POINTER(C.c_int64)]),
    "sdrx_group_set_scan": (_i, [_vp, _i, C.POINTER(ScanCfgC)]),
    "sdrx_group_get_scan": (_i, [_vp, _i, C.POINTER(ScanLevelC)]),
    "sdrx_group_get_scan_hits": (_i, [_vp, _i, _vp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "sdrx_group_get_scan_cells": (_i, [_vp, _i, _vp, C.POINTER(C.c_int64)]),
    "sdrx_set_wake": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_get_wake": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_group_set_wake": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_group_get_wake": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_get_adc_meter": (_i, [_vp, C.POINTER(AdcMeterC)]),
    "sdrx_group_get_adc_meter": (_i, [_vp, C.POINTER(AdcMeterC)]),
    "sdrx_resampler_design": (_i, [C.c_int32, C.c_int32, C.c_int32, C.c_double, _vp, C.c_int32, C.POINTER(ResamplerInfoC)]),
    "sdrx_set_resampler": (_i, [_vp, C.c_int32, _vp, C.c_int32]),
    "sdrx_get_resampler": (_i, [_vp, C.POINTER(ResamplerInfoC), _vp, C.c_int32]),
    "sdrx_get_resampler_input": (_i, [_vp, _vp, C.c_int32]),
    "sdrx_front_design": (_i, [C.c_int32, C.c_double, _vp, C.c_int32, C.POINTER(FrontInfoC)]),
    "sdrx_set_front": (_i, [_vp, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_double]),
    "sdrx_get_front": (_i, [_vp, C.POINTER(FrontInfoC), _vp, C.c_int32]),
    "sdrx_set_blanker": (_i, [_vp, C.POINTER(BlankerCfgC)]),
    "sdrx_get_blanker": (_i, [_vp, C.POINTER(BlankerCfgC), C.POINTER(BlankerRecordC)]),
    "sdrx_get_blanker_input": (_i, [_vp, _vp, C.c_int32]),
    "sdrx_set_iq_balance": (_i, [_vp, C.POINTER(IqCfgC)]),
    "sdrx_get_iq_balance": (_i, [_vp, C.POINTER(IqCfgC), C.POINTER(IqRecordC)]),
    "sdrx_set_shift": (_i, [_vp, C.POINTER(ShiftCfgC)]),
    "sdrx_get_shift": (_i, [_vp, C.POINTER(ShiftCfgC), C.POINTER(ShiftRecordC)]),
    "sdrx_shift_tables": (None, [_vp]),
    "sdrx_shift_inc": (_i, [C.c_double, C.c_double, C.POINTER(C.c_uint32)]),
    "sdrx_shift_hz": (C.c_double, [C.c_double, C.c_uint32]),
    "sdrx_set_notch": (_i, [_vp, C.POINTER(NotchCfgC)]),
    "sdrx_get_notch": (_i, [_vp, C.POINTER(NotchCfgC), C.POINTER(NotchRecordC)]),
    "sdrx_set_detector": (_i, [_vp, _i, C.POINTER(DetectCfgC)]),
    "sdrx_get_detector": (_i, [_vp, _i, C.POINTER(DetectCfgC)]),
    "sdrx_set_postfilter": (_i, [_vp, _i, C.POINTER(PostfilterCfgC), _vp]),
    "sdrx_get_postfilter": (_i, [_vp, _i, C.POINTER(PostfilterInfoC), _vp, C.c_int32]),
    "sdrx_postfilter_design": (_i, [C.c_double, C.c_double, C.c_int32, C.c_double, _vp, C.c_int32, C.POINTER(PostfilterInfoC)]),
    "sdrx_set_spectrum": (_i, [_vp, _i, _i]),
    "sdrx_get_spectrum": (_i, [_vp, _i, C.POINTER(SpectrumInfoC), _vp, _vp, _vp]),
    "sdrx_get_spectrum_levels": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "sdrx_submit_shared": (_i, [_vp, _vp]),
    "sdrx_process_shared": (_i, [_vp, _vp]),
    "sdrx_submit_if_same": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_process_if_same": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_group_create": (_i, [C.POINTER(_vp), C.POINTER(_i), _i]),
    "sdrx_group_destroy": (_i, [_vp]),
    "sdrx_group_last_error": (C.c_char_p, [_vp]),
    "sdrx_group_size": (_i, [_vp]),
    "sdrx_group_add_vfo": (_i, [_vp, C.POINTER(VfoDescC), C.POINTER(_i)]),
    "sdrx_group_set_option": (_i, [_vp, C.c_char_p, _i]),
    "sdrx_group_set_publish_callback": (_i, [_vp, PUBLISH_FN, _vp]),
    "sdrx_group_finalize": (_i, [_vp]),
    "sdrx_group_process": (_i, [_vp, _vp, _i]),
    "sdrx_group_submit": (_i, [_vp, _vp, _i]),
    "sdrx_group_submit_u8": (_i, [_vp, _vp, _i, _i]),
    "sdrx_group_process_u8": (_i, [_vp, _vp, _i, _i]),
    "sdrx_group_submit_fmt": (_i, [_vp, _vp, _i, _i, _i]),
    "sdrx_group_process_fmt": (_i, [_vp, _vp, _i, _i, _i]),
    "sdrx_group_peer_access": (_i, [_vp]),
    "sdrx_group_submit_device": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_group_process_device": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_group_wait": (_i, [_vp]),
    "sdrx_group_in_flight": (_i, [_vp]),
    "sdrx_group_sync": (_i, [_vp]),
    "sdrx_group_get_output": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "sdrx_group_locate": (_i, [_vp, _i, C.POINTER(_i), C.POINTER(_i)]),
    "sdrx_group_member": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_i)]),
    "sdrx_group_set_mixer_freqs": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_group_set_gains": (_i, [_vp, _vp, _vp, _i]),
    "sdrx_group_get_meters": (_i, [_vp, _vp, _i, _vp]),
    "sdrx_get_stats": (_i, [_vp, C.POINTER(StatsC)]),
    "sdrx_enable_kernel_timing": (_i, [_vp, _i]),
    "sdrx_get_kernel_times": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sdrx_kernel_name": (C.c_char_p, [_i]),
}

_lib = None


def build(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 build of libsdrx.so, in-tree (sdrreceiver_amd/csrc/Makefile)."""
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
    subprocess.check_call(["make", "-C", CSRC], stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib() -> C.CDLL:
    """The loaded library.  Raises if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: the HIP extension must be built "
                              f"(python -c 'import __graft_entry__ as g; g.build()' or make -C {CSRC}); "
                              "there is no CPU fallback")
        # PyTorch wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.so.1 -- the same
        # SONAMEs as /opt/rocm's, so whichever copy a process loads first serves everything in it.
        # libsdrx.so runs on either; torch cannot initialise on top of the newer system runtime
        # ("no ROCm-capable device is detected").  So when torch is installed it loads its copy
        # first, and a process may use the library and torch in any order afterwards.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(L, name)  # AttributeError if the header and the library ever diverge
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib
