#!/usr/bin/env python3
"""Time the dense device export (k_export) on the C5 shard against the torch composition a
user would otherwise write, in one process.

    python tools/bench_export.py [--streams 1250] [--iters 50] [--warmup 5] [--out profiles/export_bench.json]

The shard is bench.make_shard's (1,250 stereo 16-bit streams of 32 x 4,096 frames). It is decoded
once; then every iteration times, with torch CUDA events on the export's stream, one export of
each variant (planar f32, planar f16, interleaved f32) and one run of the comparator

    x.to(torch.float32).mul_(2**-15).permute(0, 2, 1).contiguous()

over the same samples held as one int16 [B, T, C] tensor (built once, outside the timed
region). Reported per variant: min / median / max milliseconds and the fraction of the 8.0 TB/s
HBM peak that (bytes read + bytes written, from the shapes) / time amounts to. Those intervals
hold the host side of a call from Python as well (the device idles while the call is prepared), so
each variant is also timed by the library's own HIP events around the table copy and the kernel
("device", synchronous exports through the C call).

    python tools/bench_export.py --resampled [--rate 16000] [--out profiles/resample_bench.json]

times the resampled export (k_resample) instead: the same shard (44.1 kHz) to --rate, planar f32
and planar f16, alternating in every iteration with the plain planar-f32 export (k_export) as
the yardstick, by the same two clocks. It also writes down what the kernel as built reads
from LDS for that many output frames, for comparison with the time.

    python tools/bench_export.py --mixed [--resampled] [--out profiles/mix_bench.json]

times the mixed export to mono (k_export_mixed, or with --resampled k_resample_mixed to --rate:
planar f32, C = 1, the "mono" matrix) against what a user writes without it, alternating in every
iteration: the unmixed planar-f32 export at C = 2, and that export followed by
x.mean(1, keepdim=True). Both clocks as above (the torch mean has only the first). The result goes
under the key "plain" or "resampled" of the output file, beside what the other run left there."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch  # before zflac_amd loads its library (zflac_amd/tensor.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import zflac_amd  # noqa: E402
from zflac_amd import tensor  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=bench.STREAMS_PER_GPU)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resampled", action="store_true", help="time k_resample beside k_export planar f32")
    ap.add_argument("--rate", type=int, default=16000, help="--resampled: the target rate")
    ap.add_argument("--mixed", action="store_true", help="time the mono mix beside the unmixed C = 2 export (+ torch mean)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "mix_bench.json" if a.mixed else
                             "resample_bench.json" if a.resampled else "export_bench.json")
    assert a.iters >= 50, "at least 50 timed exports per variant"

    streams = bench.make_shard(0, 1, a.streams)
    batch = zflac_amd.Batch(streams, timing=True)
    batch.run()
    batch.run()  # the second run has no first-run planning in it
    tm = batch.timings()
    B = len(batch)
    assert all(batch.info(i)[0] == 0 for i in range(B))
    C = 2
    T = bench.FRAMES_PER_STREAM * 4096
    side = torch.cuda.Stream()
    if a.mixed:
        return mixed(a, batch, tm, side)
    if a.resampled:
        return resampled(a, batch, tm, side)

    variants = {
        "planar_f32": dict(dtype=torch.float32, layout="planar"),
        "planar_f16": dict(dtype=torch.float16, layout="planar"),
        "interleaved_f32": dict(dtype=torch.float32, layout="interleaved"),
    }
    outs, nbytes = {}, {}
    src_bytes = B * T * C * 2  # the 16-bit containers k_export reads
    with torch.cuda.stream(side):
        for name, kw in variants.items():
            shape = (B, C, T) if kw["layout"] == "planar" else (B, T, C)
            outs[name] = torch.empty(shape, dtype=kw["dtype"], device="cuda")
            nbytes[name] = src_bytes + outs[name].numel() * outs[name].element_size()
        # the comparator's input: the same samples as int16 [B, T, C]
        x32, lengths = tensor.export(batch, frames=T, channels=C, dtype=torch.int32, layout="interleaved", stream=side)
        x16 = x32.to(torch.int16)
        del x32
    side.synchronize()
    assert lengths.cpu().tolist() == [T] * B
    # to (r 2, w 4) + mul_ (r 4, w 4) + contiguous (r 4, w 4) bytes per element
    nbytes["torch_composition"] = B * T * C * (2 + 4 + 4 + 4 + 4 + 4)

    def comparator():
        return x16.to(torch.float32).mul_(2 ** -15).permute(0, 2, 1).contiguous()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        r = fn()
        e1.record(side)
        side.synchronize()
        return e0.elapsed_time(e1), r

    times = {k: [] for k in list(variants) + ["torch_composition"]}
    with torch.cuda.stream(side):
        for it in range(a.warmup + a.iters):
            for name, kw in variants.items():
                ms, _ = timed(lambda: tensor.export(batch, frames=T, channels=C, out=outs[name], stream=side, **kw))
                if it >= a.warmup:
                    times[name].append(ms)
            ms, y = timed(comparator)
            if it >= a.warmup:
                times["torch_composition"].append(ms)
        same = bool(torch.equal(y, outs["planar_f32"]))
        del y
    assert same, "the export and the torch composition disagree"

    # The device side alone: synchronous exports through the C call on the batch's own stream,
    # timed by the library's HIP events around the table copy and k_export (ZFLAC_FLAG_TIMING).
    import ctypes

    from zflac_amd import _lib

    codes = {torch.float32: _lib.EXPORT_F32, torch.float16: _lib.EXPORT_F16}
    device_ms = {}
    ms = ctypes.c_double()
    for name, kw in variants.items():
        d = _lib.zflac_export_desc(ctypes.sizeof(_lib.zflac_export_desc), codes[kw["dtype"]],
                                   _lib.LAYOUT_PLANAR if kw["layout"] == "planar" else _lib.LAYOUT_INTERLEAVED, C, T, None)
        o = outs[name]
        ts = []
        for it in range(a.warmup + a.iters):
            rc = batch._L.zflac_hip_batch_export(batch._h, ctypes.byref(d), o.data_ptr(), o.numel() * o.element_size(),
                                                 None, None)
            assert rc == 0 and batch._L.zflac_hip_batch_export_ms(batch._h, ctypes.byref(ms)) == 0
            if it >= a.warmup:
                ts.append(ms.value)
        device_ms[name] = ts

    res = {"build_id": zflac_amd.build_id(), "device": torch.cuda.get_device_name(0), "streams": B, "channels": C,
           "frames": T, "iters": a.iters, "warmup": a.warmup, "hbm_peak_bytes_per_s": HBM_PEAK,
           "decode_step_ms": {"total": tm.total_ms, "scan": tm.scan_ms, "walk": tm.walk_ms, "decode": tm.decode_ms,
                              "verify": tm.verify_ms} if tm is not None else None,
           "export_equals_torch_composition": same, "variants": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        res["variants"][name] = {"min_ms": min(ts), "median_ms": med, "max_ms": max(ts), "bytes": nbytes[name],
                                 "hbm_fraction_at_median": nbytes[name] / (med * 1e-3) / HBM_PEAK}
    for name, ts in device_ms.items():
        med = statistics.median(ts)
        res["variants"][name]["device"] = {"min_ms": min(ts), "median_ms": med, "max_ms": max(ts),
                                           "hbm_fraction_at_median": nbytes[name] / (med * 1e-3) / HBM_PEAK}
    v = res["variants"]
    res["planar_f32_not_slower_than_torch"] = v["planar_f32"]["median_ms"] <= v["torch_composition"]["median_ms"]
    batch.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0 if res["planar_f32_not_slower_than_torch"] else 1


LDS_PEAK = 78e12  # bytes/s, aggregate (256 CUs x 128 B/clk x 2.4 GHz)


def resampled(a, batch, tm, side):
    """k_resample (planar f32, planar f16) alternating with k_export planar f32."""
    import ctypes
    import math

    from zflac_amd import _lib

    B, C = len(batch), 2
    T_in = bench.FRAMES_PER_STREAM * 4096
    fin = batch.info(0)[1].sample_rate
    g = math.gcd(fin, a.rate)
    L, M = a.rate // g, fin // g
    s = min(1.0, L / M) * 0.85
    K = 2 * math.ceil(16 / s) + 1
    T = batch._L.zflac_hip_resampled_frames(T_in, fin, a.rate)
    variants = {
        "k_export_planar_f32": dict(dtype=torch.float32, frames=T_in),
        "k_resample_planar_f32": dict(dtype=torch.float32, frames=T, sample_rate=a.rate),
        "k_resample_planar_f16": dict(dtype=torch.float16, frames=T, sample_rate=a.rate),
    }
    outs, nbytes = {}, {}
    with torch.cuda.stream(side):
        for name, kw in variants.items():
            outs[name] = torch.empty((B, C, kw["frames"]), dtype=kw["dtype"], device="cuda")
            nbytes[name] = B * T_in * C * 2 + outs[name].numel() * outs[name].element_size()
    side.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        fn()
        e1.record(side)
        side.synchronize()
        return e0.elapsed_time(e1)

    times = {k: [] for k in variants}
    with torch.cuda.stream(side):
        for it in range(a.warmup + a.iters):
            for name, kw in variants.items():
                ms = timed(lambda: tensor.export(batch, channels=C, out=outs[name], stream=side, **kw))
                if it >= a.warmup:
                    times[name].append(ms)
    # the device side alone: synchronous exports through the C calls, the library's own HIP events
    device_ms = {k: [] for k in variants}
    ms = ctypes.c_double()
    for it in range(a.warmup + a.iters):
        for name, kw in variants.items():
            o = outs[name]
            code = _lib.EXPORT_F32 if kw["dtype"] == torch.float32 else _lib.EXPORT_F16
            if "sample_rate" in kw:
                d = _lib.zflac_resample_desc(ctypes.sizeof(_lib.zflac_resample_desc), code, _lib.LAYOUT_PLANAR, C,
                                             kw["frames"], None, a.rate, 16, 0, 0.85, 8.555504641634386)
                rc = batch._L.zflac_hip_batch_export_resampled(batch._h, ctypes.byref(d), o.data_ptr(),
                                                               o.numel() * o.element_size(), None, None)
            else:
                d = _lib.zflac_export_desc(ctypes.sizeof(_lib.zflac_export_desc), code, _lib.LAYOUT_PLANAR, C,
                                           kw["frames"], None)
                rc = batch._L.zflac_hip_batch_export(batch._h, ctypes.byref(d), o.data_ptr(),
                                                     o.numel() * o.element_size(), None, None)
            assert rc == 0 and batch._L.zflac_hip_batch_export_ms(batch._h, ctypes.byref(ms)) == 0
            if it >= a.warmup:
                device_ms[name].append(ms.value)
    # what the kernel as built reads from LDS: per output frame and tap one tap and C samples
    lds_read = B * T * K * (1 + C) * 4
    res = {"build_id": zflac_amd.build_id(), "device": torch.cuda.get_device_name(0), "streams": B, "channels": C,
           "frames_in": T_in, "rate_in": fin, "rate_out": a.rate, "frames_out": T, "L": L, "M": M, "K": K,
           "iters": a.iters, "warmup": a.warmup, "hbm_peak_bytes_per_s": HBM_PEAK, "lds_peak_bytes_per_s": LDS_PEAK,
           "macs": B * T * C * K, "lds_read_bytes_as_built": lds_read, "lds_read_ms_at_peak": lds_read / LDS_PEAK * 1e3,
           "decode_step_ms": {"total": tm.total_ms, "scan": tm.scan_ms, "walk": tm.walk_ms, "decode": tm.decode_ms,
                              "verify": tm.verify_ms} if tm is not None else None,
           "variants": {}}
    for name in variants:
        ts, ds = times[name], device_ms[name]
        res["variants"][name] = {
            "min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts), "hbm_bytes": nbytes[name],
            "device": {"min_ms": min(ds), "median_ms": statistics.median(ds), "max_ms": max(ds),
                       "hbm_fraction_at_median": nbytes[name] / (statistics.median(ds) * 1e-3) / HBM_PEAK}}
    batch.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


def mixed(a, batch, tm, side):
    """The mono mix (C = 1) alternating with the unmixed C = 2 export, alone and followed by torch's
    mean over the channels; with --resampled all three at --rate."""
    import ctypes

    import numpy as np

    from zflac_amd import _lib

    B = len(batch)
    T_in = bench.FRAMES_PER_STREAM * 4096
    fin = batch.info(0)[1].sample_rate
    rate = a.rate if a.resampled else None
    T = batch._L.zflac_hip_resampled_frames(T_in, fin, rate) if rate else T_in
    kw = dict(frames=T, dtype=torch.float32, layout="planar", stream=side, sample_rate=rate)
    with torch.cuda.stream(side):
        out2 = torch.empty((B, 2, T), dtype=torch.float32, device="cuda")
        out1 = torch.empty((B, 1, T), dtype=torch.float32, device="cuda")
    side.synchronize()
    variants = {
        "unmixed_c2": lambda: tensor.export(batch, channels=2, out=out2, **kw)[0],
        "unmixed_c2_torch_mean": lambda: tensor.export(batch, channels=2, out=out2, **kw)[0].mean(1, keepdim=True),
        "mixed_mono": lambda: tensor.export(batch, channels=1, out=out1, mix="mono", **kw)[0],
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        r = fn()
        e1.record(side)
        side.synchronize()
        return e0.elapsed_time(e1), r

    times = {k: [] for k in variants}
    last = {}
    with torch.cuda.stream(side):
        for it in range(a.warmup + a.iters):
            for name, fn in variants.items():
                ms, last[name] = timed(fn)
                if it >= a.warmup:
                    times[name].append(ms)
        diff = float((last["mixed_mono"] - last["unmixed_c2_torch_mean"]).abs().max().item())
    # the device side alone: synchronous exports through the C calls, the library's own HIP events
    half = np.full((1, 2), 0.5, dtype=np.float32)
    mix = _lib.zflac_mix_desc(ctypes.sizeof(_lib.zflac_mix_desc), 0)
    mix.matrix[1] = half.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    device_ms = {"unmixed_c2": [], "mixed_mono": []}
    ms = ctypes.c_double()
    for it in range(a.warmup + a.iters):
        for name, (o, C, m) in {"unmixed_c2": (out2, 2, None), "mixed_mono": (out1, 1, ctypes.byref(mix))}.items():
            if rate:
                d = _lib.zflac_resample_desc(ctypes.sizeof(_lib.zflac_resample_desc), _lib.EXPORT_F32, _lib.LAYOUT_PLANAR,
                                             C, T, None, rate, 16, 0, 0.85, 8.555504641634386)
                rc = batch._L.zflac_hip_batch_export_resampled_mixed(batch._h, ctypes.byref(d), m, o.data_ptr(),
                                                                     o.numel() * 4, None, None)
            else:
                d = _lib.zflac_export_desc(ctypes.sizeof(_lib.zflac_export_desc), _lib.EXPORT_F32, _lib.LAYOUT_PLANAR, C, T,
                                           None)
                rc = batch._L.zflac_hip_batch_export_mixed(batch._h, ctypes.byref(d), m, o.data_ptr(), o.numel() * 4,
                                                           None, None)
            assert rc == 0 and batch._L.zflac_hip_batch_export_ms(batch._h, ctypes.byref(ms)) == 0
            if it >= a.warmup:
                device_ms[name].append(ms.value)

    def stats(ts):
        return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts)}

    res = {"build_id": zflac_amd.build_id(), "device": torch.cuda.get_device_name(0), "streams": B, "frames_in": T_in,
           "rate_in": fin, "rate_out": rate or fin, "frames_out": T, "iters": a.iters, "warmup": a.warmup,
           "max_abs_mixed_minus_torch_mean": diff, "variants": {}}
    for name in variants:
        res["variants"][name] = stats(times[name])
        if name in device_ms:
            res["variants"][name]["device"] = stats(device_ms[name])
    v = res["variants"]
    for clock, get in (("torch_events", lambda x: x), ("device", lambda x: x["device"])):
        u, m = get(v["unmixed_c2"]), get(v["mixed_mono"])
        res[clock] = {"mixed_over_unmixed_c2": m["median_ms"] / u["median_ms"],
                      "unmixed_c2_spread_ms": u["max_ms"] - u["min_ms"],
                      "mixed_below_unmixed_by_more_than_its_spread":
                          u["median_ms"] - m["median_ms"] > u["max_ms"] - u["min_ms"]}
    res["torch_events"]["mixed_over_unmixed_c2_torch_mean"] = (v["mixed_mono"]["median_ms"] /
                                                               v["unmixed_c2_torch_mean"]["median_ms"])
    res["floor"] = ("half the multiply-adds and half the staged span" if rate else
                    "two thirds of the bytes: (4 + 4) / (4 + 8) per frame of 16-bit stereo")
    batch.close()
    whole = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            whole = json.load(f)
    whole["resampled" if rate else "plain"] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(whole, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
