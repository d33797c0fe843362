#!/usr/bin/env python3
"""Time the log-mel features (k_mel) against the torch composition they replace, in one process.

    python tools/bench_mel.py [--baseline-lib PATH] [--rows 1250] [--samples 131072] [--iters 20] [--warmup 3] [--out profiles/mel_bench.json]

The waveform is uniform noise of the shape the C5 shard has as mono at 16 kHz (1,250 rows of
131,072 samples, float32, generated on the device from a seed). Whisper's front end: n_fft 400,
hop 160, 80 Slaney mel bins, log10, centred. Every iteration times, with torch CUDA events on one
side stream and alternating,

    k_mel        MelSpectrogram.__call__ into a preallocated tensor (one launch)
    torch        torch.stft(center=True, pad_mode="constant") -> abs()**2 -> filters @ P -> clamp -> log10
    k_mel_base   zflac_hip_mel_run of the same plan on --baseline-lib (a build of the parent commit), if given,
                 beside k_mel_abi, the same call on this build (no Python wrapper around either)

and reports the median of each (min and max beside it). k_mel's time is also given as a fraction
of the f32 matrix peak: 2 * frames * (N * 2 K' + K' * n_bins') FLOP, with the padded sizes the
kernel really multiplies (K' = 224 bins, n_bins' = 128 filters), over 157.3 TFLOP/s. The intervals
hold the host side of the Python call too. Where torch.stft is not usable on the build, the file
says so instead of a time. The two results are compared on the frames that zero and constant
padding agree on (all of them: both pad with zeros)."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import torch  # before zflac_amd loads its library (zflac_amd/tensor.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zflac_amd  # noqa: E402
from zflac_amd import _lib, errors, tensor  # noqa: E402

F32_MATRIX_PEAK = 157.3e12  # FLOP/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--rows", type=int, default=1250)
    ap.add_argument("--samples", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mel_bench.json"))
    a = ap.parse_args()
    assert zflac_amd.device_count() > 0, "no HIP device is visible"
    dev = torch.device("cuda", 0)
    N, hop, n_mels, floor = 400, 160, 80, 1e-10
    side = torch.cuda.Stream(dev)
    mel = tensor.MelSpectrogram(16000, N, hop, n_mels, floor=floor)
    with torch.cuda.stream(side):
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.rand((a.rows, a.samples), generator=g, device=dev, dtype=torch.float32) * 2 - 1
        frames = mel.mel_frames(a.samples)
        out = torch.empty((a.rows, n_mels, frames), dtype=torch.float32, device=dev)
        window = torch.from_numpy(mel.window).to(dev)
        filters = torch.from_numpy(mel.filters).to(dev)
    side.synchronize()

    def k_mel():
        return mel(x, out=out, stream=side)[0]

    abi = {}  # library -> plan, for the two direct legs
    if a.baseline_lib:
        base = ctypes.CDLL(a.baseline_lib)
        base.zflac_hip_build_id.restype, base.zflac_hip_build_id.argtypes = ctypes.c_char_p, []
        d = _lib.zflac_mel_desc(ctypes.sizeof(_lib.zflac_mel_desc), _lib.EXPORT_F32, _lib.MEL_BINS_FIRST, _lib.MEL_LOG10, 1, N,
                                hop, n_mels, 0, floor, mel.window.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                mel.filters.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        for name, lib in (("k_mel_base", base), ("k_mel_abi", _lib.load())):
            for fn in ("zflac_hip_mel_create", "zflac_hip_mel_run", "zflac_hip_mel_destroy"):
                getattr(lib, fn).restype, getattr(lib, fn).argtypes = _lib.SIGNATURES[fn]
            abi[name] = (lib, ctypes.c_void_p())
            errors.check(lib.zflac_hip_mel_create(ctypes.byref(d), 0, ctypes.byref(abi[name][1])), name)

    def abi_run(lib, plan):
        def fn():
            rc = lib.zflac_hip_mel_run(plan, x.data_ptr(), a.rows, a.samples, a.samples, 0, frames, out.data_ptr(),
                                       out.numel() * 4, side.cuda_stream)
            assert rc == 0, rc
        return fn

    def composition():
        s = torch.stft(x, N, hop, window=window, center=True, pad_mode="constant", return_complex=True)
        return torch.clamp(torch.matmul(filters, s.abs() ** 2), min=floor).log10()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        r = fn()
        e1.record(side)
        side.synchronize()
        return e0.elapsed_time(e1), r

    stft_error = None
    with torch.cuda.stream(side):
        try:
            ref = composition()
            side.synchronize()
        except Exception as e:  # noqa: BLE001  (reported, not hidden)
            stft_error, ref = f"{type(e).__name__}: {e}", None
        variants = {"k_mel": k_mel} if ref is None else {"k_mel": k_mel, "torch": composition}
        variants.update({name: abi_run(*lp) for name, lp in abi.items()})
        times = {k: [] for k in variants}
        for it in range(a.warmup + a.iters):
            for name, fn in variants.items():
                ms, r = timed(fn)
                del r
                if it >= a.warmup:
                    times[name].append(ms)
        diff = None
        if ref is not None:
            diff = float((k_mel() - ref).abs().max().item())
    K_pad, bins_pad = -(-(N // 2 + 1) // 32) * 32, 128
    flop = 2 * a.rows * frames * (N * 2 * K_pad + K_pad * bins_pad)

    def stats(ts):
        return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}

    res = {"build_id": zflac_amd.build_id(), "device": torch.cuda.get_device_name(0), "rows": a.rows, "samples": a.samples,
           "n_fft": N, "hop": hop, "n_mels": n_mels, "frames": frames, "iters": a.iters, "warmup": a.warmup,
           "flop_padded": flop, "f32_matrix_peak_flop_per_s": F32_MATRIX_PEAK, "floor_ms_at_peak": flop / F32_MATRIX_PEAK * 1e3,
           "k_mel": stats(times["k_mel"]), "torch_stft_error": stft_error, "max_abs_log10_difference": diff}
    res["k_mel"]["fraction_of_f32_matrix_peak"] = flop / (res["k_mel"]["median_ms"] * 1e-3) / F32_MATRIX_PEAK
    if "torch" in times:
        res["torch"] = stats(times["torch"])
        res["torch_over_k_mel"] = res["torch"]["median_ms"] / res["k_mel"]["median_ms"]
    if abi:
        res["baseline_build_id"] = base.zflac_hip_build_id().decode()
        res["k_mel_base"], res["k_mel_abi"] = stats(times["k_mel_base"]), stats(times["k_mel_abi"])
        b, n = res["k_mel_base"], res["k_mel_abi"]
        res["k_mel_abi_median_within_baseline_range"] = b["min_ms"] <= n["median_ms"] <= b["max_ms"]
    for lib, plan in abi.values():
        lib.zflac_hip_mel_destroy(plan)
    mel.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
