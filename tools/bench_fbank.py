#!/usr/bin/env python3
"""Time the framed (Kaldi filterbank) feature plans and the CMVN kernel beside what a user had to
do before them, beside a baseline build of the library, and beside torch compositions of the same
work, in one process.

    python tools/bench_fbank.py [--baseline-lib PATH] [--rows 1250] [--samples 131072]
                                [--iters 20] [--warmup 3] [--out profiles/fbank_bench.json]

The protocol is tools/bench_mel_bf16.py's: uniform noise, 1,250 rows of 131,072 samples, every
iteration times each variant once, in turn, with torch CUDA events on one side stream; the C entry
points are called through ctypes directly (no tensor allocation inside an interval). The turn
starts one variant later in every iteration, so that no variant always runs behind the same one
(a build that always follows its twin measures the state the twin left behind).

    kaldi_f32 / _bf16x6 / _bf16x3   zflac_hip_mel_run of MelSpectrogram.kaldi_fbank()'s plan: 512-point DFT,
                          400-sample frames every 160, snip framing, DC removal, pre-emphasis 0.97,
                          the povey window, x 32768, 80 Kaldi mel bins, ln, frames first
    kaldi_*_base          the three kaldi_* legs on --baseline-lib, where it has framed plans
    padded_f32 / _bf16x6 / _bf16x3  the same filters through a plan of zflac_hip_mel_create_ex with the window
                          zero-padded to 512 (no DC removal or pre-emphasis: it cannot express
                          them): what the first product costs over 512 samples instead of 400
    whisper_baseline      zflac_hip_mel_run of Whisper's plan (400 / 160 / 80, log10, centred) of
                          --baseline-lib (a build of the parent commit), if given
    whisper_f32           ... of this build (k_mel, unchanged)
    whisper_bf16x6_base / whisper_bf16x6   likewise for the split plan (k_mel_split)
    whisper_reflect_f32_base / whisper_reflect_f32 / whisper_reflect_bf16x6_base / whisper_reflect_bf16x6
                          zflac_hip_mel_run_ex of the same plans with ZFLAC_PAD_REFLECT (k_mel_ex, k_mel_split)
    torch_fbank           unfold -> x 32768 -> minus mean -> pre-emphasis -> window -> rfft(512) ->
                          |.|^2 -> filters -> clamp -> log
    cmvn / torch_cmvn     zflac_hip_mel_cmvn (mean_var) over the Kaldi features with per-row valid
                          lengths against torch's masked mean / std / normalise
    cmvn_bins_first / torch_cmvn_bins_first   the same over a [row][bin][frame] tensor of the same size
                          (817 f32 frames per bin: three (row, bin) starts in four are off a 16-byte boundary)

and reports min / median / max of each, whether the unchanged Whisper plans' medians lie inside the
baseline's min..max of the same run, the ratio of the folded plan to the padded one (400 / 512 of
the first product is expected), and the worst |ln| difference of the Kaldi plans to torch_fbank."""
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

MATHS = (("f32", _lib.MEL_MATH_F32), ("bf16x6", _lib.MEL_MATH_BF16X6), ("bf16x3", _lib.MEL_MATH_BF16X3))


def baseline_library(path):
    """The entry points of an older build that this tool needs (it lacks the newer ones)."""
    lib = ctypes.CDLL(path)
    for name in ("zflac_hip_mel_create_ex", "zflac_hip_mel_create_framed", "zflac_hip_mel_run", "zflac_hip_mel_run_ex",
                 "zflac_hip_mel_destroy", "zflac_hip_build_id"):
        fn = getattr(lib, name, None)
        if fn is None:
            continue
        if name == "zflac_hip_build_id":
            fn.restype, fn.argtypes = ctypes.c_char_p, []
        else:
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--rows", type=int, default=1250)
    ap.add_argument("--samples", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fbank_bench.json"))
    a = ap.parse_args()
    assert zflac_amd.device_count() > 0, "no HIP device is visible"
    tensor.check_single_runtime()
    dev = torch.device("cuda", 0)
    T, rows = a.samples, a.rows
    L = _lib.load()
    N, Nw, hop, bins, floor, pre, gain = 512, 400, 160, 80, 2.0 ** -23, 0.97, 32768.0
    povey = tensor.kaldi_window("povey", Nw)
    padded_window = np.zeros(N, np.float32)
    padded_window[(N - Nw) // 2:(N - Nw) // 2 + Nw] = povey
    kfilters = tensor.kaldi_mel_filters(16000, N, bins)
    sz = ctypes.sizeof(_lib.zflac_mel_desc)
    kd = _lib.zflac_mel_desc(sz, _lib.EXPORT_F32, _lib.MEL_FRAMES_FIRST, _lib.MEL_LN, 0, N, hop, bins, 0, floor, fptr(povey),
                             fptr(kfilters))
    fd = _lib.zflac_mel_frame_desc(ctypes.sizeof(_lib.zflac_mel_frame_desc), Nw, _lib.FRAMING_SNIP, 1, pre, gain, 0)
    pd = _lib.zflac_mel_desc(sz, _lib.EXPORT_F32, _lib.MEL_FRAMES_FIRST, _lib.MEL_LN, 0, N, hop, bins, 0, floor,
                             fptr(padded_window), fptr(kfilters))
    hann = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(400, dtype=np.float64) / 400)).astype(np.float32)
    wfilters = tensor.mel_filters(16000, 400, 80)
    wd = _lib.zflac_mel_desc(sz, _lib.EXPORT_F32, _lib.MEL_BINS_FIRST, _lib.MEL_LOG10, 1, 400, 160, 80, 0, 1e-10, fptr(hann),
                             fptr(wfilters))
    kaldi, padded, whisper = {}, {}, {}
    for name, math in MATHS:
        kaldi[name], padded[name] = ctypes.c_void_p(), ctypes.c_void_p()
        errors.check(L.zflac_hip_mel_create_framed(ctypes.byref(kd), ctypes.byref(fd), math, 0, ctypes.byref(kaldi[name])),
                     "mel_create_framed")
        errors.check(L.zflac_hip_mel_create_ex(ctypes.byref(pd), math, 0, ctypes.byref(padded[name])), "mel_create_ex")
    bd = _lib.zflac_mel_desc(sz, _lib.EXPORT_F32, _lib.MEL_BINS_FIRST, _lib.MEL_LN, 0, N, hop, bins, 0, floor, fptr(povey),
                             fptr(kfilters))
    bins_first = ctypes.c_void_p()
    errors.check(L.zflac_hip_mel_create_framed(ctypes.byref(bd), ctypes.byref(fd), _lib.MEL_MATH_F32, 0,
                                               ctypes.byref(bins_first)), "mel_create_framed")
    for name, math in MATHS[:2]:
        whisper[name] = ctypes.c_void_p()
        errors.check(L.zflac_hip_mel_create_ex(ctypes.byref(wd), math, 0, ctypes.byref(whisper[name])), "mel_create_ex")
    base, base_plans = None, {}
    if a.baseline_lib:
        base = baseline_library(a.baseline_lib)
        for name, math in MATHS[:2]:
            base_plans[name] = ctypes.c_void_p()
            errors.check(base.zflac_hip_mel_create_ex(ctypes.byref(wd), math, 0, ctypes.byref(base_plans[name])),
                         "baseline mel_create_ex")
    base_kaldi = {}  # the framed plans of the baseline build, where it has them
    if base is not None and hasattr(base, "zflac_hip_mel_create_framed"):
        for name, math in MATHS:
            base_kaldi[name] = ctypes.c_void_p()
            errors.check(base.zflac_hip_mel_create_framed(ctypes.byref(kd), ctypes.byref(fd), math, 0,
                                                          ctypes.byref(base_kaldi[name])), "baseline mel_create_framed")

    side = torch.cuda.Stream(dev)
    kframes = int(L.zflac_hip_mel_plan_frames(kaldi["f32"], T))
    pframes = int(L.zflac_hip_mel_frames(T, N, hop, 0))
    wframes = int(L.zflac_hip_mel_frames(T, 400, 160, 1))
    with torch.cuda.stream(side):
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.rand((rows, T), generator=g, device=dev, dtype=torch.float32) * 2 - 1
        kout = torch.empty((rows, kframes, bins), dtype=torch.float32, device=dev)
        wout = torch.empty((rows, 80, wframes), dtype=torch.float32, device=dev)
        bout = torch.empty((rows, bins, kframes), dtype=torch.float32, device=dev)
        valid = (kframes - (torch.arange(rows, device=dev) * 37) % (kframes // 2)).to(torch.int64)
        tw, tf = torch.from_numpy(povey).to(dev), torch.from_numpy(kfilters).to(dev)
    side.synchronize()
    st = side.cuda_stream

    def run_of(lib, handle, out, frames):
        def fn():
            rc = lib.zflac_hip_mel_run(handle, x.data_ptr(), rows, T, T, 0, frames, out.data_ptr(), out.numel() * 4, st)
            assert rc == 0, rc
        return fn

    rd = _lib.zflac_mel_run_desc(ctypes.sizeof(_lib.zflac_mel_run_desc), _lib.PAD_REFLECT, _lib.NORM_NONE, 0, x.data_ptr(), rows,
                                 T, T, None, 0, wframes, wout.data_ptr(), wout.numel() * 4, None, 0.0, 0.0, 0.0, 0)

    def reflect_of(lib, handle):
        def fn():
            rc = lib.zflac_hip_mel_run_ex(handle, ctypes.byref(rd), st)
            assert rc == 0, rc
        return fn

    cd = _lib.zflac_mel_cmvn_desc(ctypes.sizeof(_lib.zflac_mel_cmvn_desc), _lib.CMVN_MEAN_VAR, 0, 0, kout.data_ptr(), rows,
                                  kframes, valid.data_ptr(), None, None, 1e-5, 0.0)

    def cmvn():
        rc = L.zflac_hip_mel_cmvn(kaldi["f32"], ctypes.byref(cd), st)
        assert rc == 0, rc

    def torch_cmvn():
        mask = (torch.arange(kframes, device=dev)[None, :] < valid[:, None])[:, :, None]
        n = valid.clamp(min=1)[:, None, None].to(torch.float32)
        mean = (kout * mask).sum(dim=1, keepdim=True) / n
        var = (((kout - mean) * mask) ** 2).sum(dim=1, keepdim=True) / n
        return torch.where(mask, (kout - mean) / (var.sqrt() + 1e-5), torch.zeros((), device=dev))

    bcd = _lib.zflac_mel_cmvn_desc(ctypes.sizeof(_lib.zflac_mel_cmvn_desc), _lib.CMVN_MEAN_VAR, 0, 0, bout.data_ptr(), rows,
                                   kframes, valid.data_ptr(), None, None, 1e-5, 0.0)

    def cmvn_bins_first():
        rc = L.zflac_hip_mel_cmvn(bins_first, ctypes.byref(bcd), st)
        assert rc == 0, rc

    def torch_cmvn_bins_first():
        mask = (torch.arange(kframes, device=dev)[None, :] < valid[:, None])[:, None, :]
        n = valid.clamp(min=1)[:, None, None].to(torch.float32)
        mean = (bout * mask).sum(dim=2, keepdim=True) / n
        var = (((bout - mean) * mask) ** 2).sum(dim=2, keepdim=True) / n
        return torch.where(mask, (bout - mean) / (var.sqrt() + 1e-5), torch.zeros((), device=dev))

    def torch_fbank():
        f = x.unfold(1, Nw, hop) * gain                       # [rows, frames, Nw]
        f = f - f.mean(dim=2, keepdim=True)
        y = torch.cat(((1.0 - pre) * f[:, :, :1], f[:, :, 1:] - pre * f[:, :, :-1]), dim=2) * tw
        p = torch.fft.rfft(y, n=N, dim=2).abs() ** 2
        return torch.clamp(torch.matmul(p, tf.t()), min=floor).log()

    variants = {}
    for name, _ in MATHS:
        if name in base_kaldi:
            variants[f"kaldi_{name}_base"] = run_of(base, base_kaldi[name], kout, kframes)
        variants["kaldi_" + name] = run_of(L, kaldi[name], kout, kframes)
        variants["padded_" + name] = run_of(L, padded[name], kout[:, :pframes].contiguous() if pframes != kframes else kout, pframes)
    if base is not None:
        variants["whisper_baseline"] = run_of(base, base_plans["f32"], wout, wframes)
    variants["whisper_f32"] = run_of(L, whisper["f32"], wout, wframes)
    if base is not None:
        variants["whisper_bf16x6_base"] = run_of(base, base_plans["bf16x6"], wout, wframes)
    variants["whisper_bf16x6"] = run_of(L, whisper["bf16x6"], wout, wframes)
    for name in ("f32", "bf16x6"):
        if base is not None:
            variants[f"whisper_reflect_{name}_base"] = reflect_of(base, base_plans[name])
        variants[f"whisper_reflect_{name}"] = reflect_of(L, whisper[name])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        r = fn()
        e1.record(side)
        side.synchronize()
        return e0.elapsed_time(e1), r

    torch_error, diffs = None, {}
    with torch.cuda.stream(side):
        try:
            ref = torch_fbank()
            side.synchronize()
            for name, _ in MATHS:
                variants["kaldi_" + name]()
                side.synchronize()
                diffs[name] = float((kout - ref).abs().max().item())
            del ref
            variants["torch_fbank"] = torch_fbank
        except Exception as e:  # noqa: BLE001  (reported, not hidden)
            torch_error = f"{type(e).__name__}: {e}"
        variants["kaldi_f32"]()  # the features the CMVN variants read; cmvn normalises them in place again and again
        variants["cmvn"] = cmvn
        variants["torch_cmvn"] = torch_cmvn
        run_of(L, bins_first, bout, kframes)()
        variants["cmvn_bins_first"] = cmvn_bins_first
        variants["torch_cmvn_bins_first"] = torch_cmvn_bins_first
        times = {k: [] for k in variants}
        names = list(variants)
        for it in range(a.warmup + a.iters):
            k = it % len(names)  # the turn starts one variant later every iteration: no variant always follows the same one
            for name in names[k:] + names[:k]:
                ms, r = timed(variants[name])
                del r
                if it >= a.warmup:
                    times[name].append(ms)

    def stats(ts):
        return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}

    res = {"build_id": zflac_amd.build_id(), "baseline_build_id": base.zflac_hip_build_id().decode() if base else None,
           "device": torch.cuda.get_device_name(0), "rows": rows, "samples": T, "n_fft": N, "win_length": Nw, "hop": hop,
           "n_mels": bins, "kaldi_frames": kframes, "padded_frames": pframes, "whisper_frames": wframes, "iters": a.iters,
           "warmup": a.warmup, "torch_error": torch_error, "max_abs_ln_difference_vs_torch_fbank": diffs}
    for name, ts in times.items():
        res[name] = stats(ts)
    for name, _ in MATHS:
        res[f"kaldi_over_padded_{name}"] = res["kaldi_" + name]["median_ms"] / res["padded_" + name]["median_ms"]
    if base is not None:
        for new, old in [("whisper_f32", "whisper_baseline"), ("whisper_bf16x6", "whisper_bf16x6_base"),
                         ("whisper_reflect_f32", "whisper_reflect_f32_base"),
                         ("whisper_reflect_bf16x6", "whisper_reflect_bf16x6_base")] + [
                             (f"kaldi_{name}", f"kaldi_{name}_base") for name in base_kaldi]:
            res[new + "_median_within_baseline_range"] = res[old]["min_ms"] <= res[new]["median_ms"] <= res[old]["max_ms"]
            res[new + "_median_not_above_baseline_max"] = res[new]["median_ms"] <= res[old]["max_ms"]
    if "torch_fbank" in res:
        res["torch_fbank_over_kaldi_f32"] = res["torch_fbank"]["median_ms"] / res["kaldi_f32"]["median_ms"]
    res["torch_cmvn_over_cmvn"] = res["torch_cmvn"]["median_ms"] / res["cmvn"]["median_ms"]
    res["torch_cmvn_over_cmvn_bins_first"] = res["torch_cmvn_bins_first"]["median_ms"] / res["cmvn_bins_first"]["median_ms"]
    for h in list(kaldi.values()) + list(padded.values()) + list(whisper.values()) + [bins_first]:
        L.zflac_hip_mel_destroy(h)
    for h in list(base_plans.values()) + list(base_kaldi.values()):
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
