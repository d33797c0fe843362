"""Decoded batches as dense torch tensors on the GPU (zflac_hip_batch_export, k_export; at one
sample rate with sample_rate=: zflac_hip_batch_export_resampled, k_resample).

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


def export(batch: Batch, frames=None, channels=None, starts=None, dtype=torch.float32, layout="planar", out=None,
           stream=None, sample_rate=None, resample_zeros=16, resample_rolloff=0.85,
           resample_beta=8.555504641634386):
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
    and dtype is a float type. A stream already at sample_rate is exported as without it."""
    check_single_runtime()
    if dtype not in _DTYPES:
        raise TypeError(f"dtype must be one of {sorted(map(str, _DTYPES))}")
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
    if sample_rate is None:
        desc = _lib.zflac_export_desc(ctypes.sizeof(_lib.zflac_export_desc), _DTYPES[dtype], _LAYOUTS[layout],
                                      channels, frames, h_starts)
        call = batch._L.zflac_hip_batch_export
    else:
        desc = _lib.zflac_resample_desc(ctypes.sizeof(_lib.zflac_resample_desc), _DTYPES[dtype], _LAYOUTS[layout],
                                        channels, frames, h_starts, sample_rate, int(resample_zeros), 0,
                                        float(resample_rolloff), float(resample_beta))
        call = batch._L.zflac_hip_batch_export_resampled
    rc = call(batch._h, ctypes.byref(desc), out.data_ptr() or None, out.numel() * out.element_size(), valid,
              stream.cuda_stream or None)
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
