"""What the GPU tests of the cepstra plans share (tests/test_cepstra.py, test_delta.py,
test_mfcc.py): the plan through ctypes on torch tensors, the stored dtypes, guard-element buffers."""
from __future__ import annotations

import ctypes

import torch  # before zflac_amd loads its library: one HIP runtime per process (zflac_amd/tensor.py)

import numpy as np

from zflac_amd import _lib, errors, tensor

DEV = torch.device("cuda", 0)
F32, F16, BF16 = _lib.EXPORT_F32, _lib.EXPORT_F16, _lib.EXPORT_BF16
TORCH_DT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
U_DT = {F32: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8}  # the output dtype's own rounding, relative
SUB_F16 = 2.0 ** -25                                  # half a spacing of the f16 subnormals, absolute
NAMES = {F32: "f32", F16: "f16", BF16: "bf16"}
GUARD = 7  # elements before and behind a misaligned tensor


def same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    v = torch.int32 if a.element_size() == 4 else torch.int16
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def to_layout(x, layout):
    """[rows, C, frames] -> contiguous in the layout: itself, or [rows, frames, C]."""
    return (x if layout == 0 else x.transpose(1, 2)).contiguous()


def from_layout(x, layout):
    """The [rows, C, frames] view of a tensor stored in the layout."""
    return x if layout == 0 else x.transpose(1, 2)


def out_rounding(ref, dtype):
    return U_DT[dtype] * np.abs(ref) + (SUB_F16 if dtype == F16 else 0.0)


class Cepstra:
    """zflac_hip_cepstra_create / _project / _cmvn / _deltas / _destroy through ctypes, on torch tensors."""

    def __init__(self, n_in, n_out, layout, in_dtype=F32, out_dtype=F32, matrix=None, order=0, window=0):
        tensor.check_single_runtime()
        self.L = _lib.load()
        self.n_in, self.n_out, self.layout, self.in_dtype, self.out_dtype = n_in, n_out, layout, in_dtype, out_dtype
        self.order, self.window = order, window
        self.matrix = None if matrix is None else np.ascontiguousarray(matrix, dtype=np.float32)
        d = _lib.zflac_cepstra_desc(ctypes.sizeof(_lib.zflac_cepstra_desc), in_dtype, out_dtype, layout, order, n_in, n_out,
                                    window, (ctypes.c_uint8 * 3)(),
                                    None if matrix is None else self.matrix.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        self.h = ctypes.c_void_p()
        errors.check(self.L.zflac_hip_cepstra_create(ctypes.byref(d), 0, ctypes.byref(self.h)), "cepstra_create")

    def shape(self, rows, C, frames):
        return (rows, C, frames) if self.layout == 0 else (rows, frames, C)

    def project_ptr(self, src_ptr, dst_ptr, rows, frames, stream=None):
        d = _lib.zflac_cepstra_project_desc(ctypes.sizeof(_lib.zflac_cepstra_project_desc), 0, src_ptr, dst_ptr, rows, frames)
        torch.cuda.synchronize()
        return self.L.zflac_hip_cepstra_project(self.h, ctypes.byref(d), stream)

    def project(self, x):
        """x: stored input in the plan's layout -> the stored output (NaN-filled before the call)."""
        rows = x.shape[0]
        frames = x.shape[2] if self.layout == 0 else x.shape[1]
        out = torch.full(self.shape(rows, self.n_out, frames), float("nan"), dtype=TORCH_DT[self.out_dtype], device=DEV)
        errors.check(self.project_ptr(x.data_ptr(), out.data_ptr(), rows, frames), "cepstra_project")
        torch.cuda.synchronize()
        return out

    def deltas_ptr(self, src_ptr, dst_ptr, rows, frames, valid=None, pad=0.0, stream=None):
        self._valid = None if valid is None else torch.tensor([int(n) for n in valid], dtype=torch.int64, device=DEV)
        d = _lib.zflac_cepstra_delta_desc(ctypes.sizeof(_lib.zflac_cepstra_delta_desc), 0, src_ptr, dst_ptr, rows, frames,
                                          None if valid is None else self._valid.data_ptr(), pad, 0)
        torch.cuda.synchronize()
        return self.L.zflac_hip_cepstra_deltas(self.h, ctypes.byref(d), stream)

    def deltas(self, x, valid=None, pad=0.0):
        rows = x.shape[0]
        frames = x.shape[2] if self.layout == 0 else x.shape[1]
        out = torch.full(self.shape(rows, self.n_out * (self.order + 1), frames), float("nan"),
                         dtype=TORCH_DT[self.out_dtype], device=DEV)
        errors.check(self.deltas_ptr(x.data_ptr(), out.data_ptr(), rows, frames, valid, pad), "cepstra_deltas")
        torch.cuda.synchronize()
        return out

    def cmvn_ptr(self, feat_ptr, rows, frames, mode, ddof, valid=None, eps=1e-5, pad=0.0, mean=None, std=None):
        self._valid = None if valid is None else torch.tensor([int(n) for n in valid], dtype=torch.int64, device=DEV)
        c = _lib.zflac_mel_cmvn_desc(ctypes.sizeof(_lib.zflac_mel_cmvn_desc), mode, ddof, 0, feat_ptr, rows, frames,
                                     None if valid is None else self._valid.data_ptr(),
                                     None if mean is None else mean.data_ptr(), None if std is None else std.data_ptr(), eps, pad)
        torch.cuda.synchronize()
        rc = self.L.zflac_hip_cepstra_cmvn(self.h, ctypes.byref(c), None)
        torch.cuda.synchronize()
        return rc

    def scales(self, order):
        buf = (ctypes.c_float * 64)()
        n = self.L.zflac_hip_cepstra_delta_scales(self.h, order, buf, 64)
        assert n > 0, n
        return np.array(buf[:n], dtype=np.float32)

    def close(self):
        if self.h:
            self.L.zflac_hip_cepstra_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def guard_room(n, dtype, shift):
    """A buffer of guard values with room for n elements `start` elements in -> (buffer, start):
    4, 5, 6 and 8 elements off the allocation's boundary for shift 1, 2, 3 and 5."""
    start = GUARD + shift - 4
    return torch.full((n + 2 * GUARD,), 123.0, dtype=dtype, device=DEV), start


def guarded(x, shift):
    """guard_room holding x's elements."""
    buf, start = guard_room(x.numel(), x.dtype, shift)
    buf[start:start + x.numel()] = x.reshape(-1)
    return buf, start


def guards_intact(buf, start, n):
    return bool((buf[:start] == 123.0).all()) and bool((buf[start + n:] == 123.0).all())
