#!/usr/bin/env python3
"""Time zflac_hip_mel_run_ex (reflect padding, per-row lengths, the row-max clamp) beside
zflac_hip_mel_run, beside a baseline build of the library, and beside the torch composition that
does the same work, in one process.

    python tools/bench_mel_reflect.py [--baseline-lib PATH] [--rows 1250] [--samples 131072]
                                      [--iters 20] [--warmup 3] [--out profiles/mel_reflect_bench.json]

The shape is tools/bench_mel.py's: uniform noise, 1,250 rows of 131,072 samples, n_fft 400, hop 160,
80 Slaney mel bins, log10, centred, 820 frames per row, f32 out. Every iteration times each variant
once, in turn, with torch CUDA events on one side stream; the C entry points are called through
ctypes directly (no tensor allocation inside an interval):

    run_baseline        zflac_hip_mel_run of --baseline-lib (a build of the parent commit), if given
    ex_*_baseline       the three ex_reflect* legs below on --baseline-lib, where it has zflac_hip_mel_run_ex
    run                 zflac_hip_mel_run of this build
    ex_default          zflac_hip_mel_run_ex, the all-default descriptor (the same kernel as run)
    ex_zeros_lengths    ... ZFLAC_PAD_ZEROS with lengths_device, every length T: k_mel_ex with no edge tile
    ex_reflect          ... ZFLAC_PAD_REFLECT
    ex_reflect_lengths  ... and per-row lengths drawn uniformly from [T / 2, T]
    ex_reflect_row_max  ... ZFLAC_PAD_REFLECT and ZFLAC_NORM_ROW_MAX (8, 4, 0.25): fill + k_mel_ex + k_mel_norm
    torch_log           torch.stft(reflect) -> abs()**2 -> filters @ P -> clamp -> log10
    torch               ... -> amax -> maximum -> (x + 4) / 4

and reports min / median / max of each. `run` passes when its median lies within run_baseline's own
min .. max of this session (boxes differ by a few per cent; only a same-session spread is a margin)."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch  # before zflac_amd loads its library (zflac_amd/tensor.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zflac_amd  # noqa: E402
from zflac_amd import _lib, errors, tensor  # noqa: E402


def baseline_library(path):
    """The entry points of an older build that this tool needs; zflac_hip_mel_run_ex where it has it."""
    lib = ctypes.CDLL(path)
    for name in ("zflac_hip_mel_create", "zflac_hip_mel_run", "zflac_hip_mel_run_ex", "zflac_hip_mel_destroy",
                 "zflac_hip_build_id"):
        fn = getattr(lib, name, None)
        if fn is None:
            continue
        if name == "zflac_hip_build_id":
            fn.restype, fn.argtypes = ctypes.c_char_p, []
        else:
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--rows", type=int, default=1250)
    ap.add_argument("--samples", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mel_reflect_bench.json"))
    a = ap.parse_args()
    assert zflac_amd.device_count() > 0, "no HIP device is visible"
    tensor.check_single_runtime()
    dev = torch.device("cuda", 0)
    N, hop, n_mels, floor, norm = 400, 160, 80, 1e-10, (8.0, 4.0, 0.25)
    T, rows = a.samples, a.rows
    L = _lib.load()
    window = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)
    filters = tensor.mel_filters(16000, N, n_mels)
    d = _lib.zflac_mel_desc(ctypes.sizeof(_lib.zflac_mel_desc), _lib.EXPORT_F32, _lib.MEL_BINS_FIRST, _lib.MEL_LOG10, 1, N, hop,
                            n_mels, 0, floor, window.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                            filters.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    plan = ctypes.c_void_p()
    errors.check(L.zflac_hip_mel_create(ctypes.byref(d), 0, ctypes.byref(plan)), "mel_create")
    base, base_plan = None, ctypes.c_void_p()
    if a.baseline_lib:
        base = baseline_library(a.baseline_lib)
        errors.check(base.zflac_hip_mel_create(ctypes.byref(d), 0, ctypes.byref(base_plan)), "baseline mel_create")

    side = torch.cuda.Stream(dev)
    frames = int(L.zflac_hip_mel_frames(T, N, hop, 1))
    with torch.cuda.stream(side):
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.rand((rows, T), generator=g, device=dev, dtype=torch.float32) * 2 - 1
        lengths = torch.randint(T // 2, T + 1, (rows,), generator=g, device=dev, dtype=torch.int64)
        full_lengths = torch.full((rows,), T, device=dev, dtype=torch.int64)
        out = torch.empty((rows, n_mels, frames), dtype=torch.float32, device=dev)
        row_max = torch.empty((rows,), dtype=torch.float32, device=dev)
        tw, tf = torch.from_numpy(window).to(dev), torch.from_numpy(filters).to(dev)
    side.synchronize()
    st = side.cuda_stream

    def run_of(lib, handle):
        def fn():
            rc = lib.zflac_hip_mel_run(handle, x.data_ptr(), rows, T, T, 0, frames, out.data_ptr(), out.numel() * 4, st)
            assert rc == 0, rc
        return fn

    def ex_of(pad, lengths, with_norm, lib=None, handle=None):
        lib, handle = lib or L, handle or plan
        r, ad, mu = norm if with_norm else (0.0, 0.0, 0.0)
        desc = _lib.zflac_mel_run_desc(ctypes.sizeof(_lib.zflac_mel_run_desc), pad,
                                       _lib.NORM_ROW_MAX if with_norm else _lib.NORM_NONE, 0, x.data_ptr(), rows, T, T,
                                       None if lengths is None else lengths.data_ptr(), 0, frames, out.data_ptr(),
                                       out.numel() * 4, row_max.data_ptr() if with_norm else None, r, ad, mu, 0)

        def fn():
            rc = lib.zflac_hip_mel_run_ex(handle, ctypes.byref(desc), st)
            assert rc == 0, rc
        return fn

    def composition_log():
        s = torch.stft(x, N, hop, window=tw, center=True, pad_mode="reflect", return_complex=True)
        return torch.clamp(torch.matmul(tf, s.abs() ** 2), min=floor).log10()

    def composition():
        logs = composition_log()
        return (torch.maximum(logs, logs.amax(dim=(1, 2), keepdim=True) - 8.0) + 4.0) / 4.0

    variants = {}
    if base is not None:
        variants["run_baseline"] = run_of(base, base_plan)
    variants["run"] = run_of(L, plan)
    variants["ex_default"] = ex_of(_lib.PAD_ZEROS, None, False)
    variants["ex_zeros_lengths"] = ex_of(_lib.PAD_ZEROS, full_lengths, False)
    variants["ex_reflect"] = ex_of(_lib.PAD_REFLECT, None, False)
    variants["ex_reflect_lengths"] = ex_of(_lib.PAD_REFLECT, lengths, False)
    variants["ex_reflect_row_max"] = ex_of(_lib.PAD_REFLECT, None, True)
    ex_baseline = base is not None and hasattr(base, "zflac_hip_mel_run_ex")
    if ex_baseline:  # k_mel_ex and k_mel_norm of the baseline build, each beside its own leg
        variants["ex_reflect_baseline"] = ex_of(_lib.PAD_REFLECT, None, False, base, base_plan)
        variants["ex_reflect_lengths_baseline"] = ex_of(_lib.PAD_REFLECT, lengths, False, base, base_plan)
        variants["ex_reflect_row_max_baseline"] = ex_of(_lib.PAD_REFLECT, None, True, base, base_plan)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        r = fn()
        e1.record(side)
        side.synchronize()
        return e0.elapsed_time(e1), r

    stft_error, diff = None, None
    with torch.cuda.stream(side):
        try:
            ref = composition()
            side.synchronize()
            variants["ex_reflect_row_max"]()
            side.synchronize()
            diff = float((out - ref).abs().max().item())
            del ref
            variants["torch_log"] = composition_log
            variants["torch"] = composition
        except Exception as e:  # noqa: BLE001  (reported, not hidden)
            stft_error = f"{type(e).__name__}: {e}"
        times = {k: [] for k in variants}
        for it in range(a.warmup + a.iters):
            for name, fn in variants.items():
                ms, r = timed(fn)
                del r
                if it >= a.warmup:
                    times[name].append(ms)

    def stats(ts):
        return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}

    res = {"build_id": zflac_amd.build_id(), "baseline_build_id": base.zflac_hip_build_id().decode() if base else None,
           "device": torch.cuda.get_device_name(0), "rows": rows, "samples": T, "n_fft": N, "hop": hop, "n_mels": n_mels,
           "frames": frames, "tiles_per_row": -(-frames // 128), "iters": a.iters, "warmup": a.warmup, "norm": list(norm),
           "torch_stft_error": stft_error, "max_abs_difference_row_max_vs_torch": diff}
    for name, ts in times.items():
        res[name] = stats(ts)
    if base is not None:
        b, n = res["run_baseline"], res["run"]
        res["run_median_within_baseline_spread"] = b["min_ms"] <= n["median_ms"] <= b["max_ms"] or n["median_ms"] < b["min_ms"]
    if ex_baseline:
        for name in ("ex_reflect", "ex_reflect_lengths", "ex_reflect_row_max"):
            b, n = res[name + "_baseline"], res[name]
            res[name + "_median_within_baseline_range"] = b["min_ms"] <= n["median_ms"] <= b["max_ms"]
    L.zflac_hip_mel_destroy(plan)
    if base is not None:
        base.zflac_hip_mel_destroy(base_plan)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
