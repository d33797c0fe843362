#!/usr/bin/env python3
"""Time the split-bf16 feature plans (zflac_hip_mel_create_ex, k_mel_split) beside the f32 plan,
beside a baseline build of the library, and beside the torch compositions that do the same work, in
one process.

    python tools/bench_mel_bf16.py [--baseline-lib PATH] [--rows 1250] [--samples 131072]
                                   [--iters 20] [--warmup 3] [--out profiles/mel_bf16_bench.json]
                                   [--only NAME[,NAME]]   (the counters-only profile runs one variant)

The shape and the protocol are tools/bench_mel_reflect.py's: uniform noise, 1,250 rows of 131,072
samples, n_fft 400, hop 160, 80 Slaney mel bins, log10, centred, 820 frames per row, f32 out. Every
iteration times each variant once, in turn, with torch CUDA events on one side stream; the C entry
points are called through ctypes directly (no tensor allocation inside an interval):

    run_baseline          zflac_hip_mel_run of --baseline-lib (a build of the parent commit), if given
    *_baseline            the bf16x6, bf16x3 and bf16x6_reflect_row_max legs below on --baseline-lib, where
                          it has split plans
    f32                   zflac_hip_mel_run of a ZFLAC_MEL_MATH_F32 plan of this build (k_mel)
    bf16x6                ... of a ZFLAC_MEL_MATH_BF16X6 plan (k_mel_split, six piece products)
    bf16x3                ... of a ZFLAC_MEL_MATH_BF16X3 plan (three)
    bf16x6_reflect_row_max  zflac_hip_mel_run_ex, ZFLAC_PAD_REFLECT and ZFLAC_NORM_ROW_MAX (8, 4, 0.25)
    torch_log             torch.stft(reflect) -> abs()**2 -> filters @ P -> clamp -> log10
    torch                 ... -> amax -> maximum -> (x + 4) / 4

and reports min / median / max of each, each split plan's share of its MFMA floor (1.25 ms for six
terms, 0.81 ms for three: the first product at 12 or 6 cycles per sample of k against 32, the rest
of k_mel's 2.71 ms unchanged), and the worst absolute difference in log10 between each math's
reflect run and torch_log."""
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

MFMA_FLOOR_MS = {"bf16x6": 1.25, "bf16x3": 0.81}


def baseline_library(path):
    """The entry points of an older build that this tool needs; the split plans' where it has them."""
    lib = ctypes.CDLL(path)
    for name in ("zflac_hip_mel_create", "zflac_hip_mel_create_ex", "zflac_hip_mel_run", "zflac_hip_mel_run_ex",
                 "zflac_hip_mel_destroy", "zflac_hip_build_id"):
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
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mel_bf16_bench.json"))
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
    plans = {}
    for name, math in (("f32", _lib.MEL_MATH_F32), ("bf16x6", _lib.MEL_MATH_BF16X6), ("bf16x3", _lib.MEL_MATH_BF16X3)):
        plans[name] = ctypes.c_void_p()
        errors.check(L.zflac_hip_mel_create_ex(ctypes.byref(d), math, 0, ctypes.byref(plans[name])), "mel_create_ex")
    base, base_plan = None, ctypes.c_void_p()
    if a.baseline_lib:
        base = baseline_library(a.baseline_lib)
        errors.check(base.zflac_hip_mel_create(ctypes.byref(d), 0, ctypes.byref(base_plan)), "baseline mel_create")
    base_split = {}  # k_mel_split of the baseline build, where it has split plans
    if base is not None and hasattr(base, "zflac_hip_mel_create_ex") and hasattr(base, "zflac_hip_mel_run_ex"):
        for name, math in (("bf16x6", _lib.MEL_MATH_BF16X6), ("bf16x3", _lib.MEL_MATH_BF16X3)):
            base_split[name] = ctypes.c_void_p()
            errors.check(base.zflac_hip_mel_create_ex(ctypes.byref(d), math, 0, ctypes.byref(base_split[name])),
                         "baseline mel_create_ex")

    side = torch.cuda.Stream(dev)
    frames = int(L.zflac_hip_mel_frames(T, N, hop, 1))
    with torch.cuda.stream(side):
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.rand((rows, T), generator=g, device=dev, dtype=torch.float32) * 2 - 1
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

    def ex_of(handle, with_norm, lib=None):
        lib = lib or L
        r, ad, mu = norm if with_norm else (0.0, 0.0, 0.0)
        desc = _lib.zflac_mel_run_desc(ctypes.sizeof(_lib.zflac_mel_run_desc), _lib.PAD_REFLECT,
                                       _lib.NORM_ROW_MAX if with_norm else _lib.NORM_NONE, 0, x.data_ptr(), rows, T, T, None, 0,
                                       frames, out.data_ptr(), out.numel() * 4, row_max.data_ptr() if with_norm else None, r,
                                       ad, mu, 0)

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
    for name in plans:
        if name in base_split:
            variants[name + "_baseline"] = run_of(base, base_split[name])
        variants[name] = run_of(L, plans[name])
    if base_split:
        variants["bf16x6_reflect_row_max_baseline"] = ex_of(base_split["bf16x6"], True, base)
    variants["bf16x6_reflect_row_max"] = ex_of(plans["bf16x6"], True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        r = fn()
        e1.record(side)
        side.synchronize()
        return e0.elapsed_time(e1), r

    stft_error, diffs = None, {}
    with torch.cuda.stream(side):
        if a.only is None:
            try:
                ref = composition_log()
                side.synchronize()
                for name in plans:
                    ex_of(plans[name], False)()
                    side.synchronize()
                    diffs[name] = float((out - ref).abs().max().item())
                del ref
                variants["torch_log"] = composition_log
                variants["torch"] = composition
            except Exception as e:  # noqa: BLE001  (reported, not hidden)
                stft_error = f"{type(e).__name__}: {e}"
        else:
            variants = {k: v for k, v in variants.items() if k in a.only.split(",")}
            assert variants, "--only names no variant"
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
           "torch_stft_error": stft_error, "max_abs_log10_difference_reflect_vs_torch_log": diffs}
    for name, ts in times.items():
        res[name] = stats(ts)
    for name, floor_ms in MFMA_FLOOR_MS.items():
        if name in res:
            res[name]["mfma_floor_ms"] = floor_ms
            res[name]["share_of_mfma_floor"] = floor_ms / res[name]["median_ms"]
    if base is not None and "f32" in res and "run_baseline" in res:
        b, n = res["run_baseline"], res["f32"]
        res["f32_median_within_baseline_spread"] = n["median_ms"] <= b["max_ms"]
        if "bf16x6" in res:
            res["bf16x6_range_below_baseline_range"] = res["bf16x6"]["max_ms"] < b["min_ms"]
    for name in ("bf16x6", "bf16x3", "bf16x6_reflect_row_max"):
        if name in res and name + "_baseline" in res:
            b, n = res[name + "_baseline"], res[name]
            res[name + "_median_within_baseline_range"] = b["min_ms"] <= n["median_ms"] <= b["max_ms"]
    if "bf16x6" in res and "bf16x3" in res:
        res["bf16x3_median_not_above_bf16x6"] = res["bf16x3"]["median_ms"] <= res["bf16x6"]["median_ms"]
    for h in plans.values():
        L.zflac_hip_mel_destroy(h)
    if base is not None:
        base.zflac_hip_mel_destroy(base_plan)
    for h in base_split.values():
        base.zflac_hip_mel_destroy(h)
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
