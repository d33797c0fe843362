"""numpy reference of the mixed exports (zflac_hip_batch_export_mixed,
zflac_hip_batch_export_resampled_mixed), written from the definition in include/zflac_hip.h and
independent of the C++: shared by test_mix_abi.py and test_mix.py.

A stream of n channels with the C x n matrix m gives output channel c of frame t
v_c[t] = sum_j m[c][j] x_j[t], x the sample as the plain export's f32 (resample_ref.to_f32). The
library sums in f32 with fused multiply-adds in ascending j from +0; the reference here sums in
float64 (mix64), or, where every product and sum is exact in f32, in integers (mix_exact_bits).
The resampled mixed export filters v_c: resample_ref.resample over mix64's frames."""
from __future__ import annotations

import numpy as np

from . import resample_ref
from .export_ref import CONTAINER_BITS


def mix64(samples: np.ndarray, nch: int, m) -> np.ndarray:
    """[frames, C] float64: every output channel of every frame of interleaved, container-typed
    `samples`, with the coefficients as the f32 values the library is given."""
    m64 = np.asarray(m, dtype=np.float32).astype(np.float64).reshape(-1, nch)
    return resample_ref.to_f32(samples).reshape(-1, nch) @ m64.T


def mix_exact_bits(samples: np.ndarray, nch: int, m, dtype: str) -> np.ndarray:
    """[frames, C] bit patterns of `dtype` for 8- and 16-bit containers and coefficients that are
    multiples of 1/4 of magnitude at most 1: 4 m_j x_j summed in integers (at most 16 + 2 + 3
    bits, exact in f32 at every step of the library's chain), scaled by the exact
    2^-(container bits - 1) / 4, then rounded to f16 / bf16 as the plain export rounds."""
    bits = CONTAINER_BITS[samples.dtype]
    assert bits <= 16
    m4 = np.asarray(m, dtype=np.float64).reshape(-1, nch) * 4.0
    assert np.array_equal(m4, np.round(m4)) and np.abs(m4).max() <= 4
    num = samples.astype(np.int64).reshape(-1, nch) @ m4.astype(np.int64).T
    assert np.abs(num).max() < 2 ** 24
    f = num.astype(np.float32) * np.float32(2.0 ** -(bits + 1))  # (an integer 0 is +0)
    return resample_ref.round_bits(f, dtype).reshape(f.shape)


def mix_tol(m_row, n: int) -> float:
    """|f32 chain - float64 sum| for one output channel of an n-channel stream: n roundings of a
    partial sum bounded by sum_j |m_j| |x_j| with |x| <= 1, and one spare."""
    return (n + 1) * 2.0 ** -24 * float(np.abs(np.asarray(m_row, dtype=np.float64)).sum())


def resample_mix_tol(h64: np.ndarray, m_row, n: int) -> float:
    """The resampler's own bound (resample_ref.tol: K + 4 roundings) scaled by the bound on |v_c|,
    plus the mix's n + 1 roundings carried through the filter."""
    K = h64.shape[1]
    gain = max(1.0, float(np.abs(np.asarray(m_row, dtype=np.float64)).sum()))
    return (K + n + 5) * 2.0 ** -24 * float(np.abs(h64).sum(axis=1).max()) * gain
