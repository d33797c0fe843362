"""numpy reference of zflac_hip_batch_export, shared by test_export_abi.py and test_export.py.

Expected values come from the oracle's samples (interleaved, left-justified, container-typed):
f32 = sample * 2^-(container bits - 1) (numpy's int -> float32 conversion rounds to
nearest-even), f16 = that rounded by numpy to half (nearest-even, subnormals kept), bf16 = the
f32 bit pattern rounded to nearest-even in integer arithmetic. Everything is compared as bit
patterns."""
from __future__ import annotations

import numpy as np

CONTAINER_BITS = {np.dtype(np.int8): 8, np.dtype(np.int16): 16, np.dtype(np.int32): 32}
# dtype name -> (numpy dtype the bits are compared as, bytes per element)
BIT_VIEW = {"float32": np.uint32, "float16": np.uint16, "bfloat16": np.uint16, "int32": np.uint32}


def convert_bits(samples: np.ndarray, dtype: str) -> np.ndarray:
    """Bit patterns (BIT_VIEW[dtype]) of the export of container-typed `samples`."""
    bits = CONTAINER_BITS[samples.dtype]
    if dtype == "int32":
        return samples.astype(np.int32).view(np.uint32)
    f = samples.astype(np.float32) * np.float32(2.0 ** -(bits - 1))
    if dtype == "float32":
        return f.view(np.uint32)
    if dtype == "float16":
        return f.astype(np.float16).view(np.uint16)
    u = f.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def expected_row(samples, nch: int, C: int, T: int, start: int, dtype: str, layout: str):
    """(bits [C, T] or [T, C], valid frames) of one row; samples None = an error stream."""
    out = np.zeros((T, C), dtype=BIT_VIEW[dtype])
    valid = 0
    if samples is not None and nch:
        fr = samples.reshape(-1, nch)
        valid = int(min(max(fr.shape[0] - start, 0), T))
        if valid:
            k = min(nch, C)
            out[:valid, :k] = convert_bits(np.ascontiguousarray(fr[start:start + valid, :k]), dtype)
    return (np.ascontiguousarray(out.T) if layout == "planar" else out), valid
