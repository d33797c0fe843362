"""ctypes binding of libzflac_hip.so (include/zflac_hip.h).

The library is built in-tree by zflac_amd/build.py (hipcc --offload-arch=gfx950). If it
is missing this module raises ImportError-like RuntimeError: there is no fallback.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZFLAC_HIP_LIB selects another build of the same library (timing experiments)
lib_path = os.environ.get("ZFLAC_HIP_LIB") or os.path.join(_HERE, "libzflac_hip.so")


class zflac_info(ctypes.Structure):
    _fields_ = [("channels", ctypes.c_uint8), ("bits_per_sample", ctypes.c_uint8),
                ("sample_kind", ctypes.c_uint8), ("reserved", ctypes.c_uint8),
                ("sample_rate", ctypes.c_uint32), ("n_samples", ctypes.c_uint64),
                ("samples_bytes", ctypes.c_uint64)]


class zflac_stream(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("len", ctypes.c_size_t)]


class zflac_timings(ctypes.Structure):
    _fields_ = [("scan_ms", ctypes.c_double), ("decode_ms", ctypes.c_double), ("verify_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double), ("frames", ctypes.c_uint64), ("input_bytes", ctypes.c_uint64),
                ("output_bytes", ctypes.c_uint64), ("samples", ctypes.c_uint64), ("walk_ms", ctypes.c_double),
                ("md5_ms", ctypes.c_double), ("plan_ms", ctypes.c_double), ("upload_ms", ctypes.c_double),
                ("run_wall_ms", ctypes.c_double), ("read_ms", ctypes.c_double), ("host_md5_ms", ctypes.c_double),
                ("crc16_ms", ctypes.c_double), ("rest_launches", ctypes.c_uint32), ("sequential_streams", ctypes.c_uint32)]


class zflac_export_desc(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_uint8), ("layout", ctypes.c_uint8),
                ("channels", ctypes.c_uint16), ("frames", ctypes.c_uint64), ("starts", ctypes.POINTER(ctypes.c_uint64))]


class zflac_resample_desc(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_uint8), ("layout", ctypes.c_uint8),
                ("channels", ctypes.c_uint16), ("frames", ctypes.c_uint64), ("starts", ctypes.POINTER(ctypes.c_uint64)),
                ("sample_rate", ctypes.c_uint32), ("zeros", ctypes.c_uint16), ("reserved", ctypes.c_uint16),
                ("rolloff", ctypes.c_double), ("beta", ctypes.c_double)]


class zflac_mix_desc(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("matrix", ctypes.POINTER(ctypes.c_float) * 8)]


class zflac_mel_desc(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_uint8), ("layout", ctypes.c_uint8),
                ("scale", ctypes.c_uint8), ("center", ctypes.c_uint8), ("n_fft", ctypes.c_uint16),
                ("hop", ctypes.c_uint16), ("n_bins", ctypes.c_uint16), ("reserved", ctypes.c_uint16),
                ("floor", ctypes.c_float), ("window", ctypes.POINTER(ctypes.c_float)),
                ("filters", ctypes.POINTER(ctypes.c_float))]


class zflac_mel_run_desc(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("pad", ctypes.c_uint8), ("norm", ctypes.c_uint8),
                ("reserved", ctypes.c_uint16), ("wave_device", ctypes.c_void_p), ("rows", ctypes.c_uint64),
                ("wave_frames", ctypes.c_uint64), ("row_stride", ctypes.c_uint64), ("lengths_device", ctypes.c_void_p),
                ("first_frame", ctypes.c_uint64), ("frames", ctypes.c_uint64), ("dst_device", ctypes.c_void_p),
                ("dst_bytes", ctypes.c_size_t), ("row_max_device", ctypes.c_void_p), ("range", ctypes.c_float),
                ("add", ctypes.c_float), ("mul", ctypes.c_float), ("reserved2", ctypes.c_uint32)]


class zflac_mel_frame_desc(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("win_length", ctypes.c_uint16), ("framing", ctypes.c_uint8),
                ("remove_dc", ctypes.c_uint8), ("preemphasis", ctypes.c_float), ("sample_scale", ctypes.c_float),
                ("reserved", ctypes.c_uint32)]


class zflac_mel_cmvn_desc(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("mode", ctypes.c_uint8), ("ddof", ctypes.c_uint8),
                ("reserved", ctypes.c_uint16), ("feat_device", ctypes.c_void_p), ("rows", ctypes.c_uint64),
                ("frames", ctypes.c_uint64), ("valid_device", ctypes.c_void_p), ("mean_device", ctypes.c_void_p),
                ("std_device", ctypes.c_void_p), ("eps", ctypes.c_float), ("pad_value", ctypes.c_float)]


class zflac_cepstra_desc(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("in_dtype", ctypes.c_uint8), ("out_dtype", ctypes.c_uint8),
                ("layout", ctypes.c_uint8), ("delta_order", ctypes.c_uint8), ("n_in", ctypes.c_uint16),
                ("n_out", ctypes.c_uint16), ("delta_window", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 3),
                ("matrix", ctypes.POINTER(ctypes.c_float))]


class zflac_cepstra_project_desc(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("src_device", ctypes.c_void_p),
                ("dst_device", ctypes.c_void_p), ("rows", ctypes.c_uint64), ("frames", ctypes.c_uint64)]


class zflac_cepstra_delta_desc(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("src_device", ctypes.c_void_p),
                ("dst_device", ctypes.c_void_p), ("rows", ctypes.c_uint64), ("frames", ctypes.c_uint64),
                ("valid_device", ctypes.c_void_p), ("pad_value", ctypes.c_float), ("reserved2", ctypes.c_uint32)]


# every symbol include/zflac_hip.h declares, with (restype, argtypes)
_P = ctypes.c_void_p
SIGNATURES = {
    "zflac_hip_open": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(_P),
                                      ctypes.POINTER(zflac_info)]),
    "zflac_hip_open_ex": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                         ctypes.POINTER(_P), ctypes.POINTER(zflac_info)]),
    "zflac_hip_read": (ctypes.c_int, [_P, _P, ctypes.c_size_t]),
    "zflac_hip_close": (None, [_P]),
    "zflac_hip_batch_create": (ctypes.c_int, [ctypes.POINTER(zflac_stream), ctypes.c_size_t, ctypes.c_int,
                                              ctypes.c_int, ctypes.POINTER(_P)]),
    "zflac_hip_batch_run": (ctypes.c_int, [_P]),
    "zflac_hip_batch_submit": (ctypes.c_int, [_P]),
    "zflac_hip_batch_wait": (ctypes.c_int, [_P]),
    "zflac_hip_batch_ready": (ctypes.c_int, [_P]),
    "zflac_hip_batch_info": (ctypes.c_int, [_P, ctypes.c_size_t, ctypes.POINTER(zflac_info)]),
    "zflac_hip_batch_read": (ctypes.c_int, [_P, ctypes.c_size_t, _P, ctypes.c_size_t, ctypes.c_int]),
    "zflac_hip_batch_md5": (ctypes.c_int, [_P, ctypes.c_size_t, ctypes.c_char_p]),
    "zflac_hip_batch_device_samples": (_P, [_P, ctypes.c_size_t]),
    "zflac_hip_batch_timings": (ctypes.c_int, [_P, ctypes.POINTER(zflac_timings)]),
    "zflac_hip_batch_timings_ex": (ctypes.c_int, [_P, ctypes.POINTER(zflac_timings), ctypes.c_size_t]),
    "zflac_hip_abi_version": (ctypes.c_int, []),
    "zflac_hip_batch_export": (ctypes.c_int, [_P, ctypes.POINTER(zflac_export_desc), _P, ctypes.c_size_t,
                                              ctypes.POINTER(ctypes.c_uint64), _P]),
    "zflac_hip_batch_export_ms": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_double)]),
    "zflac_hip_batch_export_resampled": (ctypes.c_int, [_P, ctypes.POINTER(zflac_resample_desc), _P, ctypes.c_size_t,
                                                        ctypes.POINTER(ctypes.c_uint64), _P]),
    "zflac_hip_batch_export_mixed": (ctypes.c_int, [_P, ctypes.POINTER(zflac_export_desc),
                                                    ctypes.POINTER(zflac_mix_desc), _P, ctypes.c_size_t,
                                                    ctypes.POINTER(ctypes.c_uint64), _P]),
    "zflac_hip_batch_export_resampled_mixed": (ctypes.c_int, [_P, ctypes.POINTER(zflac_resample_desc),
                                                              ctypes.POINTER(zflac_mix_desc), _P, ctypes.c_size_t,
                                                              ctypes.POINTER(ctypes.c_uint64), _P]),
    "zflac_hip_resampled_frames": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]),
    "zflac_hip_batch_resample_tables": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64),
                                                       ctypes.POINTER(ctypes.c_uint64)]),
    "zflac_hip_mel_create": (ctypes.c_int, [ctypes.POINTER(zflac_mel_desc), ctypes.c_int, ctypes.POINTER(_P)]),
    "zflac_hip_mel_run": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                         ctypes.c_uint64, _P, ctypes.c_size_t, _P]),
    "zflac_hip_mel_run_ex": (ctypes.c_int, [_P, ctypes.POINTER(zflac_mel_run_desc), _P]),
    "zflac_hip_mel_frames": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]),
    "zflac_hip_mel_destroy": (None, [_P]),
    "zflac_hip_mel_create_ex": (ctypes.c_int, [ctypes.POINTER(zflac_mel_desc), ctypes.c_uint32, ctypes.c_int,
                                               ctypes.POINTER(_P)]),
    "zflac_hip_mel_math": (ctypes.c_int, [_P]),
    "zflac_hip_mel_create_framed": (ctypes.c_int, [ctypes.POINTER(zflac_mel_desc), ctypes.POINTER(zflac_mel_frame_desc),
                                                   ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(_P)]),
    "zflac_hip_mel_plan_frames": (ctypes.c_uint64, [_P, ctypes.c_uint64]),
    "zflac_hip_mel_cmvn": (ctypes.c_int, [_P, ctypes.POINTER(zflac_mel_cmvn_desc), _P]),
    "zflac_hip_cepstra_create": (ctypes.c_int, [ctypes.POINTER(zflac_cepstra_desc), ctypes.c_int, ctypes.POINTER(_P)]),
    "zflac_hip_cepstra_destroy": (None, [_P]),
    "zflac_hip_cepstra_features": (ctypes.c_uint32, [_P]),
    "zflac_hip_cepstra_delta_scales": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float), ctypes.c_uint32]),
    "zflac_hip_cepstra_project": (ctypes.c_int, [_P, ctypes.POINTER(zflac_cepstra_project_desc), _P]),
    "zflac_hip_cepstra_cmvn": (ctypes.c_int, [_P, ctypes.POINTER(zflac_mel_cmvn_desc), _P]),
    "zflac_hip_cepstra_deltas": (ctypes.c_int, [_P, ctypes.POINTER(zflac_cepstra_delta_desc), _P]),
    "zflac_hip_batch_decode_buckets": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint32),
                                                      ctypes.POINTER(ctypes.c_uint32)]),
    "zflac_hip_batch_front": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "zflac_hip_batch_md5_source": (ctypes.c_int, [_P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]),
    "zflac_hip_batch_md5_stats": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint32),
                                                 ctypes.POINTER(ctypes.c_uint64)]),
    "zflac_hip_batch_size": (ctypes.c_size_t, [_P]),
    "zflac_hip_batch_destroy": (None, [_P]),
    "zflac_hip_error_name": (ctypes.c_char_p, [ctypes.c_int]),
    "zflac_hip_device_count": (ctypes.c_int, []),
    "zflac_hip_version": (ctypes.c_char_p, []),
    "zflac_hip_build_id": (ctypes.c_char_p, []),
}

FLAG_TIMING = 1
FLAG_FORCE_SLOW = 2
FLAG_DEVICE_MD5 = 4
FLAG_CHECK_CRC16 = 8  # beyond zflac (src/zflac.zig:548-551 ignores the trailer)
FLAG_WALK_LANE = 16
FLAG_WALK_WAVE = 32
FLAG_FRONT_SCAN = 64  # force the frame-table front of every class: k_scan ...
FLAG_FRONT_HOP = 128  # ... or k_hop (where the streams allow it)
# zflac_hip_batch_export: element type and layout of the dense tensor
EXPORT_F32 = 0
EXPORT_F16 = 1
EXPORT_BF16 = 2
EXPORT_I32 = 3
LAYOUT_PLANAR = 0
LAYOUT_INTERLEAVED = 1
MIX_MAX_CHANNELS = 8  # zflac_mix_desc: C and n of a matrix, at most
# zflac_mel_desc: scale and layout of the features
MEL_POWER = 0
MEL_LOG10 = 1
MEL_LN = 2
MEL_BINS_FIRST = 0
MEL_FRAMES_FIRST = 1
# zflac_hip_mel_create_ex: the arithmetic of the DFT (ZFLAC_MEL_MATH_*)
MEL_MATH_F32 = 0
MEL_MATH_BF16X6 = 1
MEL_MATH_BF16X3 = 2
# zflac_mel_run_desc: padding and normalisation of a run (ZFLAC_PAD_*, ZFLAC_NORM_*)
PAD_ZEROS = 0
PAD_REFLECT = 1
PAD_MIRROR = 2  # a ZFLAC_FRAMING_KALDI_CENTER plan only
# zflac_mel_frame_desc: where a frame starts and how frames are counted (ZFLAC_FRAMING_*)
FRAMING_STFT = 0
FRAMING_SNIP = 1
FRAMING_KALDI_CENTER = 2
# zflac_mel_cmvn_desc (ZFLAC_CMVN_*)
CMVN_MEAN = 0
CMVN_MEAN_VAR = 1
NORM_NONE = 0
NORM_ROW_MAX = 1
# zflac_hip_batch_decode_buckets: one bit per k_decode history bucket (ZFLAC_BUCKET_*)
BUCKET_8 = 1
BUCKET_4 = 2
BUCKET_16 = 4
BUCKET_32 = 8
BUCKET_MIX_8 = 16
BUCKET_MIX_32 = 32
BUCKET_12 = 64
BUCKET_ALL = 127
# zflac_hip_batch_front: what built the frame table (ZFLAC_FRONT_*), ORed over the batch's classes
FRONT_SCAN = 1
FRONT_HOP = 2
# zflac_hip_batch_md5_source: where a stream's digest came from (ZFLAC_MD5_SRC_*)
MD5_SRC_NONE = 0
MD5_SRC_PIPELINED = 1
MD5_SRC_SYNC = 2
MD5_SRC_HOST_RECHECK = 3
# zflac_hip_batch_md5_stats: one bit per hash kernel (ZFLAC_MD5_K_*)
MD5_K_COOP = 1
MD5_K_MULTI = 2
MD5_K_LANE = 4

_lib = None


def load():
    """Load libzflac_hip.so (building it first if sources are newer)."""
    global _lib
    if _lib is None:
        if not os.path.exists(lib_path):
            try:
                from . import build as _build

                _build.build()
            except Exception as e:  # noqa: BLE001
                raise RuntimeError(f"libzflac_hip.so is missing and could not be built: {e}") from e
        lib = ctypes.CDLL(lib_path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib
