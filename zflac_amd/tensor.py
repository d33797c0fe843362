"""Decoded batches as dense torch tensors on the GPU (zflac_hip_batch_export, k_export; at one
sample rate with sample_rate=: zflac_hip_batch_export_resampled, k_resample; with the channels
mixed on the device with mix=: zflac_hip_batch_export_mixed / _export_resampled_mixed).

    import torch                      # before zflac_amd loads its library (see below)
    from zflac_amd import Batch, tensor

    b = Batch(streams); b.run()
    x, lengths = tensor.export(b)     # x: [stream, channel, time] float32 on cuda:<device>

This module is not imported by `zflac_amd/__init__`: torch stays optional.

One HIP runtime per process. torch bundles its own libamdhip64.so; libzflac_hip.so links
against the ROCm install's. Imported first, torch's copy is the one libzflac_hip.so binds to
and the process has a single runtime. Loaded first, libzflac_hip.so maps the ROCm install's
copy and a later `import torch` maps a second one: a stream handle or a device pointer of
one runtime means nothing to the other. So this module imports torch at its top, and every
export first checks the process's mappings and refuses to pass anything across two runtimes.
"""
from __future__ import annotations

import ctypes
import os
import re

import torch

from . import _lib, errors
from .api import Batch

_DTYPES = {torch.float32: _lib.EXPORT_F32, torch.float16: _lib.EXPORT_F16, torch.bfloat16: _lib.EXPORT_BF16,
           torch.int32: _lib.EXPORT_I32}
_LAYOUTS = {"planar": _lib.LAYOUT_PLANAR, "interleaved": _lib.LAYOUT_INTERLEAVED}


def hip_runtimes() -> list[str]:
    """The distinct libamdhip64 files mapped into this process."""
    found = set()
    with open("/proc/self/maps") as f:
        for line in f:
            sep, path = line.rstrip("\n").partition("/")[1:]
            if sep and re.match(r"libamdhip64\.so", os.path.basename(path)):
                found.add(os.path.realpath(sep + path))
    return sorted(found)


class _dl_phdr_info(ctypes.Structure):
    _fields_ = [("dlpi_addr", ctypes.c_size_t), ("dlpi_name", ctypes.c_char_p), ("dlpi_phdr", ctypes.c_void_p),
                ("dlpi_phnum", ctypes.c_uint16), ("dlpi_adds", ctypes.c_ulonglong), ("dlpi_subs", ctypes.c_ulonglong)]


_PHDR_CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.POINTER(_dl_phdr_info), ctypes.c_size_t, ctypes.c_void_p)


def _loads_so_far():
    """The dynamic linker's count of objects loaded and unloaded so far (dl_iterate_phdr's
    dlpi_adds / dlpi_subs), or None where it cannot be had."""
    seen = []

    def first(info, size, _data):
        if size >= ctypes.sizeof(_dl_phdr_info):
            seen.append((info.contents.dlpi_adds, info.contents.dlpi_subs))
        return 1  # the counters are the same in every entry

    try:
        ctypes.CDLL(None).dl_iterate_phdr(_PHDR_CB(first), None)
    except (AttributeError, OSError):
        return None
    return seen[0] if seen else None


_checked_at = None  # _loads_so_far() when /proc/self/maps was last read and held one runtime


def check_single_runtime() -> None:
    """Raise unless torch and libzflac_hip.so share one HIP runtime. Reading /proc/self/maps
    costs about a millisecond, more than the export itself; it is read again whenever the
    dynamic linker has loaded or unloaded anything since the last clean reading."""
    global _checked_at
    now = _loads_so_far()
    if now is not None and now == _checked_at:
        return
    if len(hip_runtimes()) > 1:
        raise RuntimeError("import torch before zflac_amd loads its library")
    _checked_at = now


def mix_preset(name: str) -> dict:
    """The matrices `mix="mono"` and `mix="stereo"` stand for: {n: [channels][n] float32 weights}
    for streams of n channels, as nested lists of numpy.float32 values in FLAC's channel order.
    Pure Python, no GPU.

    "mono" (channels = 1): n = 2..8 average their channels, one row of float32(1/n); mono streams
    have no matrix (the plain export's row).
    "stereo" (channels = 2), a = float32(sqrt(0.5)): a mono stream goes to both outputs with weight
    1; stereo streams have no matrix; 3..8 channels fold down to left / right: the front pair with
    weight 1, centre, back and side channels of the same side with a (the back centre of 7
    channels with 0.5 to both), LFE dropped. Nothing is normalised: a sum may exceed 1.0."""
    import numpy as np

    f = np.float32
    if name == "mono":
        return {n: [[f(1.0 / n)] * n] for n in range(2, 9)}
    if name == "stereo":
        a, o, z, h = f(np.sqrt(0.5)), f(1.0), f(0.0), f(0.5)
        return {
            1: [[o], [o]],
            3: [[o, z, a], [z, o, a]],                                  # L R C
            4: [[o, z, a, z], [z, o, z, a]],                            # FL FR BL BR
            5: [[o, z, a, a, z], [z, o, a, z, a]],                      # FL FR FC BL BR
            6: [[o, z, a, z, a, z], [z, o, a, z, z, a]],                # FL FR FC LFE BL BR
            7: [[o, z, a, z, h, a, z], [z, o, a, z, h, z, a]],          # FL FR FC LFE BC SL SR
            8: [[o, z, a, z, a, z, a, z], [z, o, a, z, z, a, z, a]],    # FL FR FC LFE BL BR SL SR
        }
    raise ValueError(f"unknown mix preset {name!r}: 'mono' or 'stereo'")


_PRESET_CHANNELS = {"mono": 1, "stereo": 2}


def _mix_desc(mix, channels):
    """zflac_mix_desc of `mix` (a dict {n: [channels, n] array-like}) and the arrays it points to."""
    import numpy as np

    if channels > _lib.MIX_MAX_CHANNELS:
        raise ValueError(f"a mix takes channels <= {_lib.MIX_MAX_CHANNELS}")
    desc = _lib.zflac_mix_desc(ctypes.sizeof(_lib.zflac_mix_desc), 0)
    keep = []
    for n, m in mix.items():
        if not isinstance(n, int) or not 1 <= n <= _lib.MIX_MAX_CHANNELS:
            raise ValueError(f"mix: channel counts are 1..{_lib.MIX_MAX_CHANNELS}, not {n!r}")
        arr = np.ascontiguousarray(m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m, dtype=np.float32)
        if arr.shape != (channels, n):
            raise ValueError(f"mix[{n}] has shape {arr.shape}, expected {(channels, n)}")
        keep.append(arr)
        desc.matrix[n - 1] = arr.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    return desc, keep


def export(batch: Batch, frames=None, channels=None, starts=None, dtype=torch.float32, layout="planar", out=None,
           stream=None, sample_rate=None, resample_zeros=16, resample_rolloff=0.85,
           resample_beta=8.555504641634386, mix=None):
    """The last run of `batch` as one dense tensor -> (tensor, lengths).

    tensor: [B, channels, frames] (layout="planar") or [B, frames, channels] ("interleaved") of
    float32 / float16 / bfloat16 (sample * 2^-(container bits - 1)) or int32 (the container
    value) on cuda:<batch device>. Row i holds frames [starts[i], starts[i] + frames) of
    stream i; frames past its end, channels it does not have and rows of streams that ended in
    an error are zero. lengths: int64 [B] on the same device, the valid frames of each row.
    frames defaults to the longest valid length, channels to the largest channel count of the OK
    streams. The export is enqueued on `stream` (default: torch's current stream of the device),
    so torch work on that stream is ordered after it; nothing is synchronised.

    sample_rate: every row resampled to this rate on the device (zflac_hip_batch_export_resampled,
    k_resample: a Kaiser-windowed sinc of `resample_zeros` zero crossings a side, cutoff
    `resample_rolloff` of the lower Nyquist rate, window shape `resample_beta`), so that streams of
    any rates share one time base. frames, starts and lengths then count frames at sample_rate,
    and dtype is a float type. A stream already at sample_rate is exported as without it.

    mix: the channels of each stream mixed on the device (zflac_hip_batch_export_mixed; with
    sample_rate, mixed first and then filtered). A dict {n: array-like [channels, n]}: streams of n
    channels get output channel c = sum_j mix[n][c][j] * source channel j (f32, fused
    multiply-adds in ascending j); channel counts not in the dict keep the fit rule above.
    Coefficients are 0 or 2^-64 <= |m| <= 2^64, channels <= 8, dtype a float type. Or "mono" /
    "stereo": mix_preset(name), with channels defaulting to (and required to be) 1 / 2. The
    presets do not normalise: a "stereo" sum may exceed 1.0."""
    check_single_runtime()
    if dtype not in _DTYPES:
        raise TypeError(f"dtype must be one of {sorted(map(str, _DTYPES))}")
    if mix is not None:
        if dtype == torch.int32:
            raise TypeError("a mixed export is float32, float16 or bfloat16")
        if isinstance(mix, str):
            preset = mix_preset(mix)
            if channels is None:
                channels = _PRESET_CHANNELS[mix]
            if int(channels) != _PRESET_CHANNELS[mix]:
                raise ValueError(f"mix={mix!r} takes channels={_PRESET_CHANNELS[mix]}")
            mix = preset
        elif not isinstance(mix, dict):
            raise TypeError("mix is a dict {n: [channels, n] weights}, 'mono' or 'stereo'")
    if sample_rate is not None:
        if dtype == torch.int32:
            raise TypeError("a resampled export is float32, float16 or bfloat16")
        sample_rate = int(sample_rate)
        if not 1 <= sample_rate <= 1048575:
            raise ValueError("1 <= sample_rate <= 1048575")
    if layout not in _LAYOUTS:
        raise ValueError("layout must be 'planar' or 'interleaved'")
    n = len(batch)
    dev = torch.device("cuda", batch.device)
    h_starts = None
    if starts is not None:
        vals = [int(s) for s in (starts.tolist() if hasattr(starts, "tolist") else starts)]
        if len(vals) != n or any(s < 0 for s in vals):
            raise ValueError("starts: one non-negative frame index per stream")
        h_starts = (ctypes.c_uint64 * n)(*vals)
    if frames is None or channels is None:
        longest, widest = 0, 0
        for i in range(n):
            rc, inf = batch.info(i)
            if rc == errors.InvalidArgument.code:
                raise errors.InvalidArgument("export needs a completed run of the batch")
            if rc or not inf.channels:
                continue
            nf = inf.n_samples // inf.channels
            if sample_rate is not None:
                nf = batch._L.zflac_hip_resampled_frames(nf, inf.sample_rate, sample_rate)
            longest = max(longest, nf - (h_starts[i] if h_starts is not None else 0))
            widest = max(widest, inf.channels)
        frames = max(longest, 1) if frames is None else frames
        channels = max(widest, 1) if channels is None else channels
    frames, channels = int(frames), int(channels)
    if frames < 1 or not 1 <= channels <= 0xFFFF:
        raise ValueError("frames >= 1 and 1 <= channels <= 65535")
    shape = (n, channels, frames) if layout == "planar" else (n, frames, channels)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    else:
        if not isinstance(out, torch.Tensor) or out.device != dev:
            raise ValueError(f"out must be a tensor on {dev}")
        if out.dtype != dtype:
            raise TypeError(f"out.dtype is {out.dtype}, expected {dtype}")
        if tuple(out.shape) != shape:
            raise ValueError(f"out.shape is {tuple(out.shape)}, expected {shape}")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    if not stream.cuda_stream:
        # the null stream has no handle to pass: the library then exports on the batch's own
        # stream and returns when the tensor is complete; work queued on `out` goes first
        stream.synchronize()
    valid = (ctypes.c_uint64 * max(n, 1))()
    mix_desc, mix_arrays = _mix_desc(mix, channels) if mix is not None else (None, None)
    if sample_rate is None:
        desc = _lib.zflac_export_desc(ctypes.sizeof(_lib.zflac_export_desc), _DTYPES[dtype], _LAYOUTS[layout],
                                      channels, frames, h_starts)
        name = "zflac_hip_batch_export"
    else:
        desc = _lib.zflac_resample_desc(ctypes.sizeof(_lib.zflac_resample_desc), _DTYPES[dtype], _LAYOUTS[layout],
                                        channels, frames, h_starts, sample_rate, int(resample_zeros), 0,
                                        float(resample_rolloff), float(resample_beta))
        name = "zflac_hip_batch_export_resampled"
    args = (out.data_ptr() or None, out.numel() * out.element_size(), valid, stream.cuda_stream or None)
    if mix_desc is None:
        rc = getattr(batch._L, name)(batch._h, ctypes.byref(desc), *args)
    else:  # (the library has read the matrices when the call returns)
        rc = getattr(batch._L, name + "_mixed")(batch._h, ctypes.byref(desc), ctypes.byref(mix_desc), *args)
        del mix_arrays
    if n == 0 and rc == errors.InvalidArgument.code:
        rc = 0  # an empty tensor has no address to hand over
    errors.check(rc, "batch_export")
    lengths = torch.tensor(list(valid)[:n], dtype=torch.int64).to(dev)
    return out, lengths


def decode_to_tensor(streams, device: int = 0, **kw):
    """Decode `streams` on `device` and export them -> (tensor, lengths, infos); infos[i] is
    (error name, channels, sample_rate, bits_per_sample) of stream i as decoded. Keyword arguments
    as for export(): with sample_rate= every row of the tensor is at that rate. The tensor is
    complete when this returns."""
    check_single_runtime()
    b = Batch(streams, device)
    try:
        b.run()
        infos = []
        for i in range(len(b)):
            rc, inf = b.info(i)
            infos.append((errors.NAMES.get(rc, "Unknown"), inf.channels, inf.sample_rate, inf.bits_per_sample))
        x, lengths = export(b, **kw)
        (kw.get("stream") or torch.cuda.current_stream(x.device)).synchronize()
        return x, lengths, infos
    finally:
        b.close()  # waits for the export on the host
