#!/usr/bin/env python3
"""Time the cepstra plans (k_mel_dct, k_mel_delta and the chain project -> cmvn -> deltas) beside
torch compositions of the same results and beside their byte floors, in one process.

    python tools/bench_cepstra.py [--rows 1250] [--frames 817] [--iters 20] [--warmup 3]
                                  [--out profiles/cepstra_bench.json]

The protocol is tools/bench_fbank.py's: every iteration times each variant once, in turn, with
torch CUDA events on one side stream; the C entry points are called through ctypes directly (no
tensor allocation inside an interval); the turn starts one variant later in every iteration, so
no variant always runs behind the same one. min / median / max per variant.

In both layouts (bf = bins first, ff = frames first), f32:
    dct_80_13 / dct_80_40 / dct_256_256      zflac_hip_cepstra_project
    torch_dct_*                              torch.matmul of the same tensor (T @ x, or x @ T^T)
    delta_13 / delta_80                      zflac_hip_cepstra_deltas, order 2, window 2, per-row lengths
    torch_delta_*                            replicate-clamped gathers at the per-row lengths, the taps
                                             applied to the base features, concatenated, padded
    chain                                    project 80 -> 13, cepstra_cmvn (mean_var), deltas (2, 2)
    torch_chain                              matmul, the masked normalisation bench_fbank.py times, the gathers
    copy                                     torch's device-to-device copy of 512 MiB: the box's copy rate

The byte floor of a kernel is the bytes it must move (its input once, its output once) over the
copy rate measured in the same run; `floor_fraction` is floor / median."""
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

DEV = torch.device("cuda", 0)


class Plan:
    def __init__(self, L, n_in, n_out, layout, matrix, order, window):
        self.L, self.n_in, self.n_out, self.layout, self.order = L, n_in, n_out, layout, order
        self.m = None if matrix is None else np.ascontiguousarray(matrix, dtype=np.float32)
        d = _lib.zflac_cepstra_desc(ctypes.sizeof(_lib.zflac_cepstra_desc), _lib.EXPORT_F32, _lib.EXPORT_F32, layout, order,
                                    n_in, n_out, window, (ctypes.c_uint8 * 3)(),
                                    None if matrix is None else self.m.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        self.h = ctypes.c_void_p()
        errors.check(L.zflac_hip_cepstra_create(ctypes.byref(d), 0, ctypes.byref(self.h)), "cepstra_create")

    def close(self):
        self.L.zflac_hip_cepstra_destroy(self.h)


def shape(layout, rows, C, frames):
    return (rows, C, frames) if layout == 0 else (rows, frames, C)


def torch_deltas(x, layout, valid, scales, pad):
    """x in the layout -> [.., 3 C, ..]: the taps over the base features at replicate-clamped frames."""
    fdim = 2 if layout == 0 else 1
    frames = x.shape[fdim]
    t = torch.arange(frames, device=x.device)
    last = (valid - 1).clamp(min=0)
    blocks = [x]
    for s in scales:
        H = (len(s) - 1) // 2
        acc = torch.zeros_like(x)
        for j in range(-H, H + 1):
            idx = torch.minimum((t[None, :] + j).clamp(min=0), last[:, None])  # [rows, frames]
            if layout == 0:
                g = torch.gather(x, 2, idx[:, None, :].expand_as(x))
            else:
                g = torch.gather(x, 1, idx[:, :, None].expand_as(x))
            acc += float(s[j + H]) * g
        blocks.append(acc)
    out = torch.cat(blocks, dim=1 if layout == 0 else 2)
    mask = t[None, :] < valid[:, None]
    return torch.where(mask[:, None, :] if layout == 0 else mask[:, :, None], out, torch.full_like(out, pad))


def torch_cmvn(x, layout, valid, eps, pad):
    """The masked normalisation tools/bench_fbank.py times: mean / std over the valid frames."""
    fdim = 2 if layout == 0 else 1
    frames = x.shape[fdim]
    mask = torch.arange(frames, device=x.device)[None, :] < valid[:, None]
    mask = mask[:, None, :] if layout == 0 else mask[:, :, None]
    n = valid.clamp(min=1).to(x.dtype).view(-1, 1, 1)
    xm = torch.where(mask, x, torch.zeros_like(x))
    mu = xm.sum(dim=fdim, keepdim=True) / n
    d = torch.where(mask, x - mu, torch.zeros_like(x))
    sigma = torch.sqrt((d * d).sum(dim=fdim, keepdim=True) / n)
    return torch.where(mask, d / (sigma + eps), torch.full_like(x, pad))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1250)
    ap.add_argument("--frames", type=int, default=817)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cepstra_bench.json"))
    a = ap.parse_args()
    assert zflac_amd.device_count() > 0, "no HIP device visible"
    tensor.check_single_runtime()
    L = _lib.load()
    rows, frames = a.rows, a.frames
    g = torch.Generator().manual_seed(3)
    side = torch.cuda.Stream(DEV)
    st = side.cuda_stream
    valid = torch.randint(frames // 2, frames + 1, (rows,), generator=g).to(DEV)
    scales = [tensor.delta_scales(o, 2) for o in (1, 2)]
    variants, bytes_of, keep = {}, {}, []

    def call(fn, *args):
        def run():
            rc = fn(*args)
            assert rc == 0, rc
        return run

    n_copy = 128 * 1024 * 1024  # f32 elements: 512 MiB in, 512 MiB out
    cs, cd = torch.empty(n_copy, device=DEV), torch.empty(n_copy, device=DEV)
    variants["copy"] = lambda: cd.copy_(cs)
    bytes_of["copy"] = 2 * 4 * n_copy
    for layout, tag in ((0, "bf"), (1, "ff")):
        for n_in, n_out in ((80, 13), (80, 40), (256, 256)):
            T = tensor.dct_matrix(n_out, n_in, lifter=22.0)
            p = Plan(L, n_in, n_out, layout, T, 0, 0)
            x = (torch.randn(shape(layout, rows, n_in, frames), generator=g) * 3.0 - 5.0).to(DEV)
            y = torch.empty(shape(layout, rows, n_out, frames), device=DEV)
            d = _lib.zflac_cepstra_project_desc(ctypes.sizeof(_lib.zflac_cepstra_project_desc), 0, x.data_ptr(), y.data_ptr(),
                                                rows, frames)
            name = f"dct_{n_in}_{n_out}_{tag}"
            variants[name] = call(L.zflac_hip_cepstra_project, p.h, ctypes.byref(d), st)
            bytes_of[name] = 4 * rows * frames * (n_in + n_out)
            Tt = torch.from_numpy(T).to(DEV)
            variants["torch_" + name] = (lambda Tt=Tt, x=x: torch.matmul(Tt, x)) if layout == 0 else \
                (lambda Tt=Tt, x=x: torch.matmul(x, Tt.t()))
            keep += [p, x, y, d, Tt]
            ref = variants["torch_" + name]()
            variants[name]()
            torch.cuda.synchronize()
            assert float((ref - y).abs().max()) < 1e-2 * float(ref.abs().max()), name  # tf32-free matmul: close
        for C in (13, 80):
            p = Plan(L, C, C, layout, None, 2, 2)
            x = (torch.randn(shape(layout, rows, C, frames), generator=g) * 3.0 - 5.0).to(DEV)
            y = torch.empty(shape(layout, rows, 3 * C, frames), device=DEV)
            d = _lib.zflac_cepstra_delta_desc(ctypes.sizeof(_lib.zflac_cepstra_delta_desc), 0, x.data_ptr(), y.data_ptr(), rows,
                                              frames, valid.data_ptr(), 0.0, 0)
            name = f"delta_{C}_{tag}"
            variants[name] = call(L.zflac_hip_cepstra_deltas, p.h, ctypes.byref(d), st)
            bytes_of[name] = 4 * rows * frames * 4 * C
            variants["torch_" + name] = lambda x=x, layout=layout: torch_deltas(x, layout, valid, scales, 0.0)
            keep += [p, x, y, d]
            ref = variants["torch_" + name]()
            variants[name]()
            torch.cuda.synchronize()
            assert float((ref - y).abs().max()) < 1e-4, name
        T = tensor.dct_matrix(13, 80, lifter=22.0)
        p = Plan(L, 80, 13, layout, T, 2, 2)
        x = (torch.randn(shape(layout, rows, 80, frames), generator=g) * 3.0 - 5.0).to(DEV)
        base = torch.empty(shape(layout, rows, 13, frames), device=DEV)
        y = torch.empty(shape(layout, rows, 39, frames), device=DEV)
        d1 = _lib.zflac_cepstra_project_desc(ctypes.sizeof(_lib.zflac_cepstra_project_desc), 0, x.data_ptr(), base.data_ptr(),
                                             rows, frames)
        d2 = _lib.zflac_mel_cmvn_desc(ctypes.sizeof(_lib.zflac_mel_cmvn_desc), _lib.CMVN_MEAN_VAR, 0, 0, base.data_ptr(), rows,
                                      frames, valid.data_ptr(), None, None, 1e-5, 0.0)
        d3 = _lib.zflac_cepstra_delta_desc(ctypes.sizeof(_lib.zflac_cepstra_delta_desc), 0, base.data_ptr(), y.data_ptr(), rows,
                                           frames, valid.data_ptr(), 0.0, 0)

        def chain(p=p, d1=d1, d2=d2, d3=d3):
            assert L.zflac_hip_cepstra_project(p.h, ctypes.byref(d1), st) == 0
            assert L.zflac_hip_cepstra_cmvn(p.h, ctypes.byref(d2), st) == 0
            assert L.zflac_hip_cepstra_deltas(p.h, ctypes.byref(d3), st) == 0

        Tt = torch.from_numpy(T).to(DEV)

        def torch_chain(x=x, Tt=Tt, layout=layout):
            c = torch.matmul(Tt, x) if layout == 0 else torch.matmul(x, Tt.t())
            return torch_deltas(torch_cmvn(c, layout, valid, 1e-5, 0.0), layout, valid, scales, 0.0)

        variants[f"chain_{tag}"] = chain
        variants[f"torch_chain_{tag}"] = torch_chain
        # project reads 80 and writes 13; cmvn reads 13 three times at most and writes 13 (floor: once each); deltas read 13, write 39
        bytes_of[f"chain_{tag}"] = 4 * rows * frames * (80 + 13 + 13 + 13 + 13 + 39)
        keep += [p, x, base, y, d1, d2, d3, Tt]
        ref = torch_chain()
        chain()
        torch.cuda.synchronize()
        assert float((ref - y).abs().max()) < 1e-2, f"chain_{tag}"

    names = list(variants)
    times = {n: [] for n in names}
    for it in range(a.warmup + a.iters):
        for k in range(len(names)):
            n = names[(k + it) % len(names)]
            with torch.cuda.stream(side):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                variants[n]()
                e1.record(side)
            e1.synchronize()
            if it >= a.warmup:
                times[n].append(e0.elapsed_time(e1))
    res = {n: {"min_ms": min(t), "median_ms": statistics.median(t), "max_ms": max(t)} for n, t in times.items()}
    rate = bytes_of["copy"] / (res["copy"]["median_ms"] * 1e-3)
    for n, b in bytes_of.items():
        res[n]["bytes"] = b
        if n != "copy":
            res[n]["floor_ms"] = b / rate * 1e3
            res[n]["floor_fraction"] = res[n]["floor_ms"] / res[n]["median_ms"]
    for n in names:
        if "torch_" + n in res:
            res[n]["torch_over_this"] = res["torch_" + n]["median_ms"] / res[n]["median_ms"]
    out = {"rows": rows, "frames": frames, "iters": a.iters, "warmup": a.warmup, "dtype": "f32",
           "copy_rate_TBps": rate / 1e12, "build_id": L.zflac_hip_build_id().decode(),
           "device": torch.cuda.get_device_name(0), "variants": res}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for n in names:
        r = res[n]
        extra = f"  floor {r['floor_fraction']:.2f}" if "floor_fraction" in r else ""
        extra += f"  torch/this {r['torch_over_this']:.2f}" if "torch_over_this" in r else ""
        print(f"{n:24s} {r['min_ms']:8.3f} {r['median_ms']:8.3f} {r['max_ms']:8.3f} ms{extra}")
    for p in keep:
        if isinstance(p, Plan):
            p.close()


if __name__ == "__main__":
    main()
