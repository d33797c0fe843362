"""Decoded batches as dense torch tensors on the GPU (zflac_hip_batch_export, k_export; at one
sample rate with sample_rate=: zflac_hip_batch_export_resampled, k_resample; with the channels
mixed on the device with mix=: zflac_hip_batch_export_mixed / _export_resampled_mixed), and
log-mel features of such a tensor in one more launch (MelSpectrogram, decode_to_features:
zflac_hip_mel_run, k_mel; with reflect padding, per-row lengths and the row-max clamp, Whisper's
front end: zflac_hip_mel_run_ex, MelSpectrogram.whisper()).

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


def mel_filters(sample_rate, n_fft, n_mels, f_min=0.0, f_max=None, mel_scale="slaney", norm="slaney"):
    """A triangular mel filterbank -> numpy float32 [n_mels, n_fft // 2 + 1]. Pure numpy, no GPU.

    The mel scale, f in Hz:
      "htk":    mel(f) = 2595 log10(1 + f / 700),            f(mel) = 700 (10^(mel / 2595) - 1)
      "slaney": mel(f) = 3 f / 200 for f < 1000, else 15 + 27 ln(f / 1000) / ln(6.4)
                f(mel) = 200 mel / 3 for mel < 15, else 1000 exp((mel - 15) ln(6.4) / 27)
    n_mels + 2 points p_0 .. p_{n_mels + 1} lie equally spaced in mel from mel(f_min) to mel(f_max)
    (f_max defaults to sample_rate / 2) and are taken back to Hz. With f_k = k sample_rate / n_fft
    the frequency of bin k, filter m is the triangle over [p_m, p_{m + 2}] with its peak, 1, at
    p_{m + 1}:
      w[m][k] = max(0, min((f_k - p_m) / (p_{m + 1} - p_m), (p_{m + 2} - f_k) / (p_{m + 2} - p_{m + 1})))
    norm="slaney" scales row m by 2 / (p_{m + 2} - p_m) (unit area per filter); norm=None leaves the
    peaks at 1. Everything is computed in float64 and rounded once. (sample_rate 16000, n_fft 400,
    n_mels 80 with the defaults are the filters Whisper's front end uses.)"""
    import numpy as np

    n_fft, n_mels = int(n_fft), int(n_mels)
    if n_fft < 2 or n_fft % 2 or n_mels < 1:
        raise ValueError("n_fft even and >= 2, n_mels >= 1")
    f_max = sample_rate / 2.0 if f_max is None else float(f_max)
    f_min = float(f_min)
    if not 0.0 <= f_min < f_max:
        raise ValueError("0 <= f_min < f_max")
    if mel_scale == "htk":
        def to_mel(f):
            return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)

        def to_hz(m):
            return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)
    elif mel_scale == "slaney":
        step = np.log(6.4) / 27.0

        def to_mel(f):
            f = np.asarray(f, dtype=np.float64)
            return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) / step)

        def to_hz(m):
            m = np.asarray(m, dtype=np.float64)
            return np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * np.exp((m - 15.0) * step))
    else:
        raise ValueError("mel_scale is 'slaney' or 'htk'")
    if norm not in ("slaney", None):
        raise ValueError("norm is 'slaney' or None")
    p = to_hz(np.linspace(to_mel(f_min), to_mel(f_max), n_mels + 2))
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sample_rate) / n_fft)
    lower = (f[None, :] - p[:-2, None]) / (p[1:-1] - p[:-2])[:, None]
    upper = (p[2:, None] - f[None, :]) / (p[2:] - p[1:-1])[:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    if norm == "slaney":
        w *= (2.0 / (p[2:] - p[:-2]))[:, None]
    return w.astype(np.float32)


def kaldi_window(name, win_length):
    """Kaldi's frame windows -> numpy float32 [win_length], with c[n] = cos(2 pi n / (win_length - 1)):
      "povey"        (0.5 - 0.5 c[n]) ** 0.85
      "hanning"      0.5 - 0.5 c[n]
      "hamming"      0.54 - 0.46 c[n]
      "rectangular"  1
    (symmetric windows: the first and last samples of "hanning" and "povey" are 0). Computed in
    float64 and rounded once; win_length = 1 gives [1] for every name."""
    import numpy as np

    nw = int(win_length)
    if nw < 1:
        raise ValueError("win_length >= 1")
    if name not in ("povey", "hanning", "hamming", "rectangular"):
        raise ValueError("window is 'povey', 'hanning', 'hamming' or 'rectangular'")
    if nw == 1 or name == "rectangular":
        return np.ones(nw, dtype=np.float32)
    c = np.cos(2.0 * np.pi * np.arange(nw, dtype=np.float64) / (nw - 1))
    if name == "hamming":
        return (0.54 - 0.46 * c).astype(np.float32)
    h = np.maximum(0.5 - 0.5 * c, 0.0)
    return (h ** 0.85 if name == "povey" else h).astype(np.float32)


def kaldi_mel_filters(sample_rate, n_fft, n_mels, low_freq=20.0, high_freq=0.0):
    """Kaldi's mel filterbank (triangles in the mel domain, no VTLN) -> numpy float32
    [n_mels, n_fft // 2 + 1]. mel(f) = 1127 ln(1 + f / 700); a high_freq <= 0 is added to the
    Nyquist frequency. With D = (mel(high) - mel(low)) / (n_mels + 1), filter m has left =
    mel(low) + m D, centre = left + D, right = centre + D; bin k < n_fft / 2 at mel_k =
    mel(k sample_rate / n_fft) strictly inside (left, right) weighs (mel_k - left) / D up to the
    centre and (right - mel_k) / D beyond it. The Nyquist column is 0 (Kaldi has n_fft / 2 bins).
    Computed in float64 and rounded once."""
    import numpy as np

    n_fft, n_mels = int(n_fft), int(n_mels)
    if n_fft < 2 or n_fft % 2 or n_mels < 1:
        raise ValueError("n_fft even and >= 2, n_mels >= 1")
    nyquist = 0.5 * float(sample_rate)
    low, high = float(low_freq), float(high_freq)
    if high <= 0.0:
        high += nyquist
    if not (0.0 <= low < high <= nyquist):
        raise ValueError("0 <= low_freq < high_freq <= sample_rate / 2")

    def mel(f):
        return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)

    mel_lo, mel_hi = mel(low), mel(high)
    delta = (mel_hi - mel_lo) / (n_mels + 1)
    left = (mel_lo + np.arange(n_mels, dtype=np.float64) * delta)[:, None]
    centre, right = left + delta, left + 2.0 * delta
    mk = mel(np.arange(n_fft // 2, dtype=np.float64) * (float(sample_rate) / n_fft))[None, :]
    w = np.where(mk <= centre, (mk - left) / delta, (right - mk) / delta)
    w = np.where((mk > left) & (mk < right), w, 0.0)
    out = np.zeros((n_mels, n_fft // 2 + 1), dtype=np.float32)
    out[:, :n_fft // 2] = w.astype(np.float32)
    return out


def dct_matrix(n_ceps, n_mels, norm="ortho", lifter=0.0):
    """The DCT-II rows that take n_mels log-mel bins to n_ceps cepstra -> numpy float32
    [n_ceps, n_mels]. norm="ortho" (Kaldi, torchaudio's and librosa's default): row 0 is
    sqrt(1 / M), row k sqrt(2 / M) cos(pi k (m + 1/2) / M), M = n_mels; norm=None: 2 cos(...) for
    every row (torchaudio's create_dct(norm=None)). lifter Q > 0 folds Kaldi's cepstral lifter
    1 + (Q / 2) sin(pi k / Q) into row k (0: none). Computed in float64 and rounded once."""
    import math as _math

    import numpy as np

    n_ceps, n_mels, lifter = int(n_ceps), int(n_mels), float(lifter)
    if not (1 <= n_mels <= 256 and 1 <= n_ceps <= n_mels):
        raise ValueError("1 <= n_ceps <= n_mels <= 256")
    if norm not in ("ortho", None):
        raise ValueError("norm is 'ortho' or None")
    if not (_math.isfinite(lifter) and lifter >= 0.0):
        raise ValueError("lifter finite and >= 0")
    k = np.arange(n_ceps, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    d = np.cos(np.pi * k * (m + 0.5) / n_mels)
    if norm == "ortho":
        d *= np.sqrt(2.0 / n_mels)
        d[0] = np.sqrt(1.0 / n_mels)
    else:
        d *= 2.0
    if lifter > 0.0:
        d *= 1.0 + 0.5 * lifter * np.sin(np.pi * k / lifter)
    return d.astype(np.float32)


def delta_scales(order, window):
    """Kaldi's delta taps (DeltaFeatures) -> numpy float64 [2 order window + 1], tap j = -order W ..
    order W: s_0 = [1], s_o = s_{o-1} convolved with [j / sum_{|i| <= W} i^2, j = -W..W]. Order 1,
    W = 2: [-2, -1, 0, 1, 2] / 10; order 2: [4, 4, 1, -4, -10, -4, 1, 4, 4] / 100."""
    import numpy as np

    order, window = int(order), int(window)
    if not (0 <= order <= 3 and 1 <= window <= 5):
        raise ValueError("0 <= order <= 3, 1 <= window <= 5")
    j = np.arange(-window, window + 1, dtype=np.float64)
    step = j / np.sum(j * j)
    s = np.ones(1, dtype=np.float64)
    for _ in range(order):
        s = np.convolve(s, step)
    return s


_MEL_SCALES = {"power": _lib.MEL_POWER, "log10": _lib.MEL_LOG10, "ln": _lib.MEL_LN}
_MEL_LAYOUTS = {"bins_first": _lib.MEL_BINS_FIRST, "frames_first": _lib.MEL_FRAMES_FIRST}
_MEL_PADS = {"zeros": _lib.PAD_ZEROS, "reflect": _lib.PAD_REFLECT, "mirror": _lib.PAD_MIRROR}
_MEL_FRAMINGS = {"stft": _lib.FRAMING_STFT, "snip": _lib.FRAMING_SNIP, "kaldi_center": _lib.FRAMING_KALDI_CENTER}
_MEL_CMVN = {"mean": _lib.CMVN_MEAN, "mean_var": _lib.CMVN_MEAN_VAR}
_MEL_MATHS = {"f32": _lib.MEL_MATH_F32, "bf16x6": _lib.MEL_MATH_BF16X6, "bf16x3": _lib.MEL_MATH_BF16X3}


class MelSpectrogram:
    """Log-mel features of f32 waveforms on the GPU in one launch (zflac_hip_mel_run, k_mel).

        mel = MelSpectrogram(16000)                     # n_fft 400, hop 160, 80 mel bins, log10
        feats, feat_lengths = mel(x, lengths)           # x: [B, T] or [B, C, T] float32 on cuda
        mel = MelSpectrogram.whisper()                  # reflect padding and (max(x, M - 8) + 4) / 4

    window: "hann" (periodic, 0.5 - 0.5 cos(2 pi n / n_fft)) or n_fft values. filters: an array
    [n_bins, n_fft // 2 + 1], or None for mel_filters(sample_rate, n_fft, n_mels, **filter_kw).
    scale: "log10" or "ln" of max(v, floor), or "power" (the sums themselves; floor is not used).
    center: frame t starts at sample t hop - n_fft / 2 (else at t hop).

    pad: "zeros" (the default): samples outside a row are zero, and there is no reflect padding:
    the first and last n_fft / (2 hop) frames differ from torch.stft's default. "reflect" (needs
    center=True; zflac_hip_mel_run_ex, ZFLAC_PAD_REFLECT): the row is reflected once about its
    first and its last sample, which is torch.stft's pad_mode="reflect" and numpy.pad's "reflect".
    reflect_at says where a row ends: "length" (the default) at its entry of `lengths`, so a
    batch of rows of different lengths is reflected row by row and nothing past a row's length is
    read; "end" at T, the end of the (zero-filled) tensor row, `lengths` then only giving
    feature_lengths.
    normalize: None, or (range, add, mul): every element becomes (max(x, M - range) + add) * mul
    in f32, M the maximum of its row ([n_bins, frames] of one batch row and channel, as this call
    computes them) before rounding to dtype; a log scale only. The maxima of the last call are
    mel.last_row_max ([B] or [B, C] float32), or the third result with return_row_max=True.
    With the defaults a call is one zflac_hip_mel_run, as before.
    math: the arithmetic of the DFT (zflac_hip_mel_create_ex). "f32" (the default): f32 on the
    matrix cores, as ever. "bf16x6" / "bf16x3": both operands split into bfloat16 pieces, six or
    three piece products kept, on the 16 times faster bf16 matrix cores (k_mel_split): a sum is
    within 3 * 2^-24 (f32-grade) or 2^-14 (about 84 dB) of sum |c| |x| of the full product; a bin
    further than that below its frame's loudest content is noise under "bf16x3". mel.math reads
    the plan's mode back from the library.

    Framed plans (zflac_hip_mel_create_framed; with every argument below at its default the plan is
    zflac_hip_mel_create_ex's, as before). win_length: the frame length Nw <= n_fft, the frame
    zero-extended to the n_fft-point DFT; `window` then has Nw values ("hann": periodic over Nw; or
    a kaldi_window name). framing: "stft" (torch.stft with the window centred in the DFT), "snip"
    (Kaldi, snip_edges=True: frame t at t hop, (n - Nw) // hop + 1 frames) or "kaldi_center"
    (snip_edges=False: frame t at t hop + hop // 2 - Nw // 2, (n + hop // 2) // hop frames); the
    Kaldi framings need center=False, and all need hop <= Nw. Per frame, in Kaldi's order:
    sample_scale (32768 takes [-1, 1) to Kaldi's 16-bit scale), remove_dc (subtract the frame's
    mean), preemphasis a (y[0] = (1 - a) f[0], y[n] = f[n] - a f[n - 1]), the window. All of it is
    folded into the plan's tables and costs nothing per run. pad="mirror" ("kaldi_center" only)
    mirrors a row about its ends with the edge sample repeated, as Kaldi does.
    cmvn: None, "mean" or "mean_var": behind the features, every (row, bin) is normalised over the
    row's feature_lengths valid frames (zflac_hip_mel_cmvn, k_mel_cmvn): (x - mean) / (std + cmvn_eps),
    std with cmvn_ddof 0 or 1, frames past the valid ones set to cmvn_pad. The statistics of the
    last call are mel.last_mean and mel.last_std ([B, (C,) n_bins] float32).

    Cepstra and dynamic features (a cepstra plan of the library beside the mel plan; without these
    arguments a call is exactly what it was). mfcc: None, a cepstra count (the matrix is
    dct_matrix(mfcc, n_bins, dct_norm, lifter)) or an array [n_out, n_bins]: every frame's bins are
    projected by it (zflac_hip_cepstra_project, k_mel_dct). The mel plan then writes float32
    whatever `dtype` is, so the projection reads unrounded log-mels. deltas: None or (order 1..3,
    window 1..5): Kaldi's add-deltas (zflac_hip_cepstra_deltas, k_mel_delta) appends the 1st ..
    order-th derivatives, block o at features o C .. o C + C - 1, over the row's feature_lengths
    valid frames (the clamp is at the first frame of the call and at the last valid one); frames
    past them hold cmvn_pad. A call enqueues, in order: the mel run, the projection, cmvn over
    the base features (the cepstra if projected, else the bins; last_mean / last_std have that
    many columns), the deltas. dtype is the final tensor's and mel.n_features its feature count.
    Not provided: dither, use_energy / raw_energy, VTLN, pre-emphasis over the whole waveform,
    frame splicing and low-frame-rate stacking.
    The object owns a plan of the library: close() it, or use it in `with`."""

    @classmethod
    def whisper(cls, n_mels=80, device=0, dtype=torch.float32, math="f32"):
        """Whisper's front end: 16 kHz, n_fft 400, hop 160, the periodic Hann window, the Slaney
        filterbank, log10 with floor 1e-10, reflect padding at the end of the row, and
        (max(x, M - 8) + 4) / 4. Whisper's rows are 30 s (480,000 samples, zero-filled behind the
        audio) and it drops the STFT's last frame: call the plan with frames=3000, which also
        keeps that frame out of M. The result is the encoder's input [B, n_mels, 3000]."""
        return cls(16000, 400, 160, n_mels, scale="log10", floor=1e-10, center=True, dtype=dtype, device=device,
                   pad="reflect", normalize=(8.0, 4.0, 0.25), reflect_at="end", math=math)

    @classmethod
    def kaldi_fbank(cls, sample_rate=16000, num_mel_bins=80, frame_length_ms=25.0, frame_shift_ms=10.0, snip_edges=True,
                    preemphasis=0.97, remove_dc=True, window="povey", low_freq=20.0, high_freq=0.0, math="f32",
                    dtype=torch.float32, cmvn=None, device=0, mfcc=None, lifter=0.0, dct_norm="ortho", deltas=None,
                    **cmvn_kw):
        """Kaldi's compute-fbank-feats (kaldifeat, torchaudio.compliance.kaldi.fbank, lhotse) for
        waveforms in [-1, 1): frames of frame_length_ms every frame_shift_ms in the next power-of-two
        DFT, the samples scaled by 32768, DC removal, pre-emphasis and the window per frame,
        kaldi_mel_filters, ln with the floor 2^-23 (FLT_EPSILON), [B, (C,) frames, num_mel_bins].
        snip_edges=False centres the frames and mirrors the row's ends. Dither is 0; use_energy,
        raw_energy and VTLN are not provided."""
        nw = int(sample_rate * frame_length_ms / 1000.0)
        hop = int(sample_rate * frame_shift_ms / 1000.0)
        n_fft = 2
        while n_fft < nw:
            n_fft *= 2
        return cls(sample_rate, n_fft, hop, num_mel_bins, window=window,
                   filters=kaldi_mel_filters(sample_rate, n_fft, num_mel_bins, low_freq, high_freq), scale="ln",
                   floor=2.0 ** -23, center=False, dtype=dtype, layout="frames_first", device=device,
                   pad="zeros" if snip_edges else "mirror", math=math, win_length=nw,
                   framing="snip" if snip_edges else "kaldi_center", remove_dc=remove_dc, preemphasis=preemphasis,
                   sample_scale=32768.0, cmvn=cmvn, mfcc=mfcc, lifter=lifter, dct_norm=dct_norm, deltas=deltas,
                   **cmvn_kw)

    @classmethod
    def kaldi_mfcc(cls, sample_rate=16000, num_mel_bins=23, num_ceps=13, cepstral_lifter=22.0, use_energy=False,
                   **fbank_kw):
        """Kaldi's compute-mfcc-feats (kaldifeat's Mfcc, torchaudio.compliance.kaldi.mfcc) with
        use_energy=False: kaldi_fbank(sample_rate, num_mel_bins, **fbank_kw), then the orthonormal
        DCT to num_ceps cepstra with the lifter 1 + (Q / 2) sin(pi k / Q), Q = cepstral_lifter
        (0: none), [B, (C,) frames, num_ceps]. cmvn= normalises the cepstra; deltas=(2, 2) appends
        add-deltas' columns behind that. use_energy / raw_energy (C0 replaced by the frame's log
        energy) is not provided: C0 is the DCT's row 0."""
        if use_energy:
            raise ValueError("use_energy=True is not provided: C0 is the DCT's row 0, not the frame's log energy")
        for k in ("mfcc", "lifter", "dct_norm"):
            if k in fbank_kw:
                raise TypeError(f"kaldi_mfcc() sets {k}; use num_ceps and cepstral_lifter")
        return cls.kaldi_fbank(sample_rate, num_mel_bins, mfcc=int(num_ceps), lifter=cepstral_lifter, **fbank_kw)

    def __init__(self, sample_rate, n_fft=400, hop=160, n_mels=80, window="hann", filters=None, scale="log10",
                 floor=1e-10, center=True, dtype=torch.float32, layout="bins_first", device=0, pad="zeros",
                 normalize=None, reflect_at="length", math="f32", win_length=None, framing="stft", remove_dc=False,
                 preemphasis=0.0, sample_scale=1.0, cmvn=None, cmvn_eps=1e-5, cmvn_ddof=0, cmvn_pad=0.0, mfcc=None,
                 lifter=0.0, dct_norm="ortho", deltas=None, **filter_kw):
        import math as _math

        import numpy as np

        self._h = self._c = None
        if math not in _MEL_MATHS:
            raise ValueError("math is 'f32', 'bf16x6' or 'bf16x3'")
        if deltas is not None:
            try:
                deltas = tuple(int(v) for v in deltas)
            except TypeError:
                raise ValueError("deltas is None or (order, window)") from None
            if len(deltas) != 2 or not (1 <= deltas[0] <= 3 and 1 <= deltas[1] <= 5):
                raise ValueError("deltas is None or (order 1..3, window 1..5)")
        self.deltas = deltas
        check_single_runtime()
        if pad not in _MEL_PADS:
            raise ValueError("pad is 'zeros', 'reflect' or 'mirror'")
        if pad == "reflect" and not center:
            raise ValueError("pad='reflect' needs center=True")
        if framing not in _MEL_FRAMINGS:
            raise ValueError("framing is 'stft', 'snip' or 'kaldi_center'")
        if framing != "stft" and center:
            raise ValueError(f"framing={framing!r} needs center=False")
        if pad == "mirror" and framing != "kaldi_center":
            raise ValueError("pad='mirror' needs framing='kaldi_center'")
        preemphasis, sample_scale = float(preemphasis), float(sample_scale)
        if not (_math.isfinite(preemphasis) and 0.0 <= preemphasis <= 1.0):
            raise ValueError("0 <= preemphasis <= 1")
        if not (_math.isfinite(sample_scale) and 2.0 ** -64 <= abs(sample_scale) <= 2.0 ** 64):
            raise ValueError("2^-64 <= |sample_scale| <= 2^64")
        if cmvn is not None and cmvn not in _MEL_CMVN:
            raise ValueError("cmvn is None, 'mean' or 'mean_var'")
        cmvn_eps, cmvn_pad = float(cmvn_eps), float(cmvn_pad)
        if not (_math.isfinite(cmvn_eps) and cmvn_eps >= 0.0) or not _math.isfinite(cmvn_pad) or cmvn_ddof not in (0, 1):
            raise ValueError("cmvn_eps finite and >= 0, cmvn_pad finite, cmvn_ddof 0 or 1")
        self.cmvn, self.cmvn_eps, self.cmvn_ddof, self.cmvn_pad = cmvn, cmvn_eps, int(cmvn_ddof), cmvn_pad
        self.last_mean = self.last_std = None
        if reflect_at not in ("length", "end"):
            raise ValueError("reflect_at is 'length' or 'end'")
        if normalize is not None:
            normalize = tuple(float(v) for v in normalize)
            if len(normalize) != 3 or not all(_math.isfinite(v) for v in normalize) or normalize[0] < 0 or normalize[2] == 0:
                raise ValueError("normalize is (range >= 0, add, mul != 0), all finite")
            if scale == "power":
                raise ValueError("normalize needs a log scale")
        self.pad, self.normalize, self.reflect_at = pad, normalize, reflect_at
        self.last_row_max = None
        self._keep = None
        if dtype not in _DTYPES or dtype == torch.int32:
            raise TypeError("dtype is float32, float16 or bfloat16")
        if scale not in _MEL_SCALES:
            raise ValueError("scale is 'log10', 'ln' or 'power'")
        if layout not in _MEL_LAYOUTS:
            raise ValueError("layout is 'bins_first' or 'frames_first'")
        n_fft, hop = int(n_fft), int(hop)
        if not (2 <= n_fft <= 2048 and n_fft % 2 == 0 and 1 <= hop <= n_fft):
            raise ValueError("n_fft even in 2..2048, 1 <= hop <= n_fft")
        nw = n_fft if win_length is None else int(win_length)
        if not 1 <= nw <= n_fft:
            raise ValueError("1 <= win_length <= n_fft")
        self.framed = nw != n_fft or framing != "stft" or bool(remove_dc) or preemphasis != 0.0 or sample_scale != 1.0
        if self.framed and hop > nw:
            raise ValueError("hop <= win_length")
        if isinstance(window, str):
            if window == "hann":
                w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nw, dtype=np.float64) / nw)).astype(np.float32)
            elif window in ("povey", "hanning", "hamming", "rectangular"):
                w = kaldi_window(window, nw)
            else:
                raise ValueError("window is 'hann', a kaldi_window name or an array of win_length values")
        else:
            w = np.ascontiguousarray(window.detach().cpu().numpy() if isinstance(window, torch.Tensor) else window,
                                     dtype=np.float32)
        if w.shape != (nw,):
            raise ValueError(f"window has shape {w.shape}, expected {(nw,)}")
        if filters is None:
            fb = mel_filters(sample_rate, n_fft, n_mels, **filter_kw)
        else:
            if filter_kw:
                raise TypeError(f"with filters=, unexpected {sorted(filter_kw)}")
            fb = np.ascontiguousarray(filters.detach().cpu().numpy() if isinstance(filters, torch.Tensor) else filters,
                                      dtype=np.float32)
        if fb.ndim != 2 or fb.shape[1] != n_fft // 2 + 1 or not 1 <= fb.shape[0] <= 256:
            raise ValueError(f"filters have shape {fb.shape}, expected (1..256, {n_fft // 2 + 1})")
        self.sample_rate, self.n_fft, self.hop, self.n_bins = sample_rate, n_fft, hop, int(fb.shape[0])
        self.center, self.dtype, self.layout, self.scale, self.device = bool(center), dtype, layout, scale, int(device)
        self.floor = 0.0 if scale == "power" else float(floor)
        self.window, self.filters = w, fb
        self.win_length, self.framing, self.remove_dc = nw, framing, bool(remove_dc)
        self.preemphasis, self.sample_scale = preemphasis, sample_scale
        if mfcc is None:
            if lifter != 0.0:
                raise ValueError("lifter needs mfcc")
            T = None
        elif isinstance(mfcc, (int, np.integer)) and not isinstance(mfcc, bool):
            T = dct_matrix(mfcc, self.n_bins, dct_norm, lifter)
        else:
            if lifter != 0.0:
                raise ValueError("with a matrix for mfcc, fold the lifter into it")
            T = np.ascontiguousarray(mfcc.detach().cpu().numpy() if isinstance(mfcc, torch.Tensor) else mfcc, dtype=np.float32)
            if T.ndim != 2 or T.shape[1] != self.n_bins or not 1 <= T.shape[0] <= 256:
                raise ValueError(f"mfcc has shape {T.shape}, expected (1..256, {self.n_bins})")
            if not np.isfinite(T).all():
                raise ValueError("mfcc: every value finite")
        self.dct = T
        self.n_base = self.n_bins if T is None else int(T.shape[0])  # what cmvn normalises and the deltas extend
        self.n_features = self.n_base * (1 + (deltas[0] if deltas else 0))
        mel_dtype = dtype if T is None else torch.float32  # the projection reads unrounded log-mels
        self._L = _lib.load()
        if T is not None or deltas:
            cd = _lib.zflac_cepstra_desc(ctypes.sizeof(_lib.zflac_cepstra_desc), _DTYPES[mel_dtype], _DTYPES[dtype],
                                         _MEL_LAYOUTS[layout], deltas[0] if deltas else 0, self.n_bins, self.n_base,
                                         deltas[1] if deltas else 0, (ctypes.c_uint8 * 3)(),
                                         None if T is None else T.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
            c = ctypes.c_void_p()
            errors.check(self._L.zflac_hip_cepstra_create(ctypes.byref(cd), self.device, ctypes.byref(c)), "cepstra_create")
            self._c = c
        self._mel_dtype = mel_dtype
        dtype = mel_dtype  # of the mel plan below; self.dtype is the final tensor's
        desc = _lib.zflac_mel_desc(ctypes.sizeof(_lib.zflac_mel_desc), _DTYPES[dtype], _MEL_LAYOUTS[layout],
                                   _MEL_SCALES[scale], int(self.center), n_fft, hop, self.n_bins, 0, self.floor,
                                   w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                   fb.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        self._h = ctypes.c_void_p()
        if self.framed:
            fd = _lib.zflac_mel_frame_desc(ctypes.sizeof(_lib.zflac_mel_frame_desc), nw, _MEL_FRAMINGS[framing],
                                           int(self.remove_dc), preemphasis, sample_scale, 0)
            errors.check(self._L.zflac_hip_mel_create_framed(ctypes.byref(desc), ctypes.byref(fd), _MEL_MATHS[math],
                                                             self.device, ctypes.byref(self._h)), "mel_create_framed")
            return
        errors.check(self._L.zflac_hip_mel_create_ex(ctypes.byref(desc), _MEL_MATHS[math], self.device,
                                                     ctypes.byref(self._h)), "mel_create_ex")

    @property
    def math(self):
        """The plan's arithmetic as the library reports it (zflac_hip_mel_math): "f32", "bf16x6" or "bf16x3"."""
        code = self._L.zflac_hip_mel_math(self._h)
        return next(k for k, v in _MEL_MATHS.items() if v == code)

    def mel_frames(self, n_samples):
        """Frames of a row of n_samples under the plan's framing (zflac_hip_mel_plan_frames): an
        int, or a tensor for a tensor."""
        if isinstance(n_samples, torch.Tensor):
            n = n_samples.to(torch.int64)
            if self.framing == "snip":
                return torch.where(n >= self.win_length, (n - self.win_length) // self.hop + 1, torch.zeros_like(n))
            if self.framing == "kaldi_center":
                return (n + self.hop // 2) // self.hop
            if self.center:
                return torch.where(n > 0, n // self.hop + 1, torch.zeros_like(n))
            return torch.where(n >= self.n_fft, (n - self.n_fft) // self.hop + 1, torch.zeros_like(n))
        if self._h is None:
            raise ValueError("the plan is closed")
        return int(self._L.zflac_hip_mel_plan_frames(self._h, int(n_samples)))

    def __call__(self, x, lengths=None, frames=None, first_frame=0, out=None, stream=None, return_row_max=False):
        """x: contiguous float32 [B, T] or [B, C, T] on cuda:<device>; lengths: valid samples per
        batch row (default T) -> (features, feature_lengths). features: [B, (C,) n_bins, frames]
        (layout="bins_first") or [B, (C,) frames, n_bins], frame j of it being feature frame
        first_frame + j; frames defaults to mel_frames(T) - first_frame. feature_lengths: int64
        [B], clamp(mel_frames(lengths) - first_frame, 0, frames). Enqueued on `stream` (default:
        torch's current stream of the device); nothing is synchronised. return_row_max=True:
        -> (features, feature_lengths, row_max), row_max float32 [B] or [B, C] (see the class)."""
        check_single_runtime()
        if self._h is None:
            raise ValueError("the plan is closed")
        dev = torch.device("cuda", self.device)
        if not isinstance(x, torch.Tensor) or x.device != dev or x.dtype != torch.float32:
            raise TypeError(f"x must be a float32 tensor on {dev}")
        if x.dim() not in (2, 3) or not x.is_contiguous():
            raise ValueError("x must be contiguous [B, T] or [B, C, T]")
        T = int(x.shape[-1])
        first_frame = int(first_frame)
        if first_frame < 0:
            raise ValueError("first_frame >= 0")
        if frames is None:
            frames = max(self.mel_frames(T) - first_frame, 1)
        frames = int(frames)
        if frames < 1:
            raise ValueError("frames >= 1")
        lead = tuple(x.shape[:-1])
        shape = lead + ((self.n_features, frames) if self.layout == "bins_first" else (frames, self.n_features))
        if out is None:
            out = torch.empty(shape, dtype=self.dtype, device=dev)
        else:
            if not isinstance(out, torch.Tensor) or out.device != dev:
                raise ValueError(f"out must be a tensor on {dev}")
            if out.dtype != self.dtype:
                raise TypeError(f"out.dtype is {out.dtype}, expected {self.dtype}")
            if tuple(out.shape) != shape:
                raise ValueError(f"out.shape is {tuple(out.shape)}, expected {shape}")
            if not out.is_contiguous():
                raise ValueError("out must be contiguous")
        if lengths is None:
            lengths = torch.full((int(x.shape[0]),), T, dtype=torch.int64, device=dev)
        else:
            lengths = torch.as_tensor(lengths, dtype=torch.int64).to(dev)
            if tuple(lengths.shape) != (int(x.shape[0]),):
                raise ValueError("lengths: one per batch row")
        feature_lengths = torch.clamp(self.mel_frames(lengths) - first_frame, 0, frames)
        rows = 1
        for n in lead:
            rows *= int(n)
        ex = self.pad != "zeros" or self.normalize is not None or return_row_max
        row_max = torch.empty(lead, dtype=torch.float32, device=dev) if ex else None
        self.last_row_max = row_max
        self.last_mean = self.last_std = None
        if rows == 0:
            return (out, feature_lengths, row_max) if return_row_max else (out, feature_lengths)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        if not stream.cuda_stream:
            stream.synchronize()  # the null stream has no handle: the plan's own stream, complete on return
        feat = out  # what the mel run writes: the result, or the bins a cepstra plan goes on from
        if self._c is not None:
            feat = torch.empty(lead + ((self.n_bins, frames) if self.layout == "bins_first" else (frames, self.n_bins)),
                               dtype=self._mel_dtype, device=dev)
        if not ex:
            rc = self._L.zflac_hip_mel_run(self._h, x.data_ptr(), rows, T, T, first_frame, frames, feat.data_ptr(),
                                           feat.numel() * feat.element_size(), stream.cuda_stream or None)
            errors.check(rc, "mel_run")
            self._finish(feat, out, lead, rows, frames, feature_lengths, stream)
            return out, feature_lengths
        per_row = None
        if self.reflect_at == "length":  # one length per row of the launch: [B, C, T] has C rows per entry
            per_row = lengths.clamp(min=0).repeat_interleave(rows // int(x.shape[0])).contiguous()
        rng, add, mul = self.normalize or (0.0, 0.0, 0.0)
        d = _lib.zflac_mel_run_desc(ctypes.sizeof(_lib.zflac_mel_run_desc), _MEL_PADS[self.pad],
                                    _lib.NORM_NONE if self.normalize is None else _lib.NORM_ROW_MAX, 0, x.data_ptr(), rows,
                                    T, T, None if per_row is None else per_row.data_ptr(), first_frame, frames,
                                    feat.data_ptr(), feat.numel() * feat.element_size(), row_max.data_ptr(), rng, add, mul, 0)
        rc = self._L.zflac_hip_mel_run_ex(self._h, ctypes.byref(d), stream.cuda_stream or None)
        errors.check(rc, "mel_run_ex")
        self._keep = per_row  # read by the launch: alive until the next call, and not reused before `stream` is past it
        for t in (per_row, row_max):
            if t is not None and stream.cuda_stream:
                t.record_stream(stream)
        self._finish(feat, out, lead, rows, frames, feature_lengths, stream)
        return (out, feature_lengths, row_max) if return_row_max else (out, feature_lengths)

    def _finish(self, feat, out, lead, rows, frames, feature_lengths, stream):
        """What follows the mel run that wrote `feat`. Without a cepstra plan feat is out and this is
        the cmvn step. With one: the projection, cmvn over the base features, the deltas, ending in out."""
        if self._c is None:
            self._cmvn(out, lead, rows, frames, feature_lengths, stream)
            return
        st = stream.cuda_stream or None
        base, temps = feat, [feat]
        if self.dct is not None:
            base = out
            if self.deltas:
                base = torch.empty(feat.shape[:-2] + ((self.n_base, frames) if self.layout == "bins_first" else
                                                      (frames, self.n_base)), dtype=self.dtype, device=out.device)
                temps.append(base)
            d = _lib.zflac_cepstra_project_desc(ctypes.sizeof(_lib.zflac_cepstra_project_desc), 0, feat.data_ptr(),
                                                base.data_ptr(), rows, frames)
            errors.check(self._L.zflac_hip_cepstra_project(self._c, ctypes.byref(d), st), "cepstra_project")
        self._cmvn(base, lead, rows, frames, feature_lengths, stream, projected=self.dct is not None)
        if self.deltas:
            valid = feature_lengths.repeat_interleave(rows // int(feature_lengths.shape[0])).contiguous()
            d = _lib.zflac_cepstra_delta_desc(ctypes.sizeof(_lib.zflac_cepstra_delta_desc), 0, base.data_ptr(),
                                              out.data_ptr(), rows, frames, valid.data_ptr(), self.cmvn_pad, 0)
            errors.check(self._L.zflac_hip_cepstra_deltas(self._c, ctypes.byref(d), st), "cepstra_deltas")
            temps.append(valid)
        self._keep_ceps = temps  # as _keep: read by the launches
        for t in temps:
            if stream.cuda_stream:
                t.record_stream(stream)

    def _cmvn(self, out, lead, rows, frames, feature_lengths, stream, projected=False):
        """zflac_hip_mel_cmvn (zflac_hip_cepstra_cmvn over projected features) over the features just
        enqueued, feature_lengths as the valid frames."""
        if self.cmvn is None:
            return
        dev = out.device
        valid = feature_lengths.repeat_interleave(rows // int(feature_lengths.shape[0])).contiguous()
        mean = torch.empty(lead + (self.n_base if projected else self.n_bins,), dtype=torch.float32, device=dev)
        std = torch.empty_like(mean)
        d = _lib.zflac_mel_cmvn_desc(ctypes.sizeof(_lib.zflac_mel_cmvn_desc), _MEL_CMVN[self.cmvn], self.cmvn_ddof, 0,
                                     out.data_ptr(), rows, frames, valid.data_ptr(), mean.data_ptr(), std.data_ptr(),
                                     self.cmvn_eps, self.cmvn_pad)
        if projected:
            errors.check(self._L.zflac_hip_cepstra_cmvn(self._c, ctypes.byref(d), stream.cuda_stream or None), "cepstra_cmvn")
        else:
            errors.check(self._L.zflac_hip_mel_cmvn(self._h, ctypes.byref(d), stream.cuda_stream or None), "mel_cmvn")
        self._keep_cmvn = valid  # as _keep: read by the launch
        for t in (valid, mean, std):
            if stream.cuda_stream:
                t.record_stream(stream)
        self.last_mean, self.last_std = mean, std

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.zflac_hip_mel_destroy(self._h)  # waits for the device
            self._h = None
        if getattr(self, "_c", None) is not None:
            self._L.zflac_hip_cepstra_destroy(self._c)
            self._c = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def decode_to_features(streams, mel: MelSpectrogram, device: int = 0, mix="mono", **export_kw):
    """Decode `streams`, export them at mel.sample_rate with the channels mixed (decode_to_tensor,
    float32) and take the features of that tensor -> (features, feature_lengths, infos). features:
    [B, channels, n_bins, frames]; the row of a stream that ended in an error is the constant an
    all-zero row gives, with length 0. Complete when this returns."""
    if mel.device != device:
        raise ValueError(f"the plan is on device {mel.device}, not {device}")
    if export_kw.get("dtype", torch.float32) != torch.float32 or export_kw.get("layout", "planar") != "planar":
        raise TypeError("the features are taken from a planar float32 export")
    x, lengths, infos = decode_to_tensor(streams, device, sample_rate=mel.sample_rate, mix=mix, **export_kw)
    stream = export_kw.get("stream") or torch.cuda.current_stream(x.device)
    feats, feature_lengths = mel(x, lengths, stream=stream)
    stream.synchronize()
    return feats, feature_lengths, infos


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
