"""numpy float64 reference of zflac_hip_batch_export_resampled, written from the filter's
definition (include/zflac_hip.h) and independent of the C++: shared by test_resample_plan.py
and test_resample.py.

A stream of rate fin goes to fout: g = gcd, M = fin / g, L = fout / g, s = min(1, L / M) * rolloff,
W = ceil(Z / s), K = 2 W + 1; y[m] = sum_k h[r][k] x[q - W + k] with q = floor(m M / L),
r = (m M) mod L, x = sample * 2^-(container bits - 1) (rounded to f32 as the plain export
rounds it), zero outside the stream; h = u / sum_k u, u = s sinc(t) kaiser(t),
t = s ((k - W) - r / L). The sums here are float64 over the taps rounded to f32."""
from __future__ import annotations

import math

import numpy as np

from .export_ref import BIT_VIEW, CONTAINER_BITS

ZEROS, ROLLOFF, BETA = 16, 0.85, 8.555504641634386


def ratio(fin: int, fout: int, Z: int = ZEROS, rolloff: float = ROLLOFF):
    g = math.gcd(fin, fout)
    M, L = fin // g, fout // g
    s = min(1.0, L / M) * rolloff
    W = int(math.ceil(Z / s))
    return L, M, W, 2 * W + 1, s


def taps(fin: int, fout: int, Z: int = ZEROS, rolloff: float = ROLLOFF, beta: float = BETA):
    """(L, M, W, K, h64): h64[L, K] in float64, every phase normalised to unit DC gain."""
    L, M, W, K, s = ratio(fin, fout, Z, rolloff)
    k = np.arange(K, dtype=np.float64)[None, :]
    r = np.arange(L, dtype=np.float64)[:, None]
    t = s * ((k - W) - r / L)
    inside = np.abs(t) < Z
    y = np.where(inside, t / Z, 0.0)
    kaiser = np.where(inside, np.i0(beta * np.sqrt(1.0 - y * y)) / np.i0(beta), 0.0)
    u = s * np.sinc(t) * kaiser
    return L, M, W, K, u / u.sum(axis=1, keepdims=True)


def out_frames(n: int, fin: int, fout: int) -> int:
    if not fin or not fout:
        return 0
    g = math.gcd(fin, fout)
    M, L = fin // g, fout // g
    return -((-n * L) // M)


def tol(h64: np.ndarray) -> float:
    """Absolute f32 error bound of a K-term sum of products with |x| <= 1: K roundings of the
    accumulation, one of each tap, two for a last-bit difference between the two double-precision
    table builders, one for the int -> f32 rounding of 32-bit samples."""
    K = h64.shape[1]
    return (K + 4) * 2.0 ** -24 * float(np.abs(h64).sum(axis=1).max())


def to_f32(samples: np.ndarray) -> np.ndarray:
    """Container-typed samples as the plain export's f32, held in float64."""
    bits = CONTAINER_BITS[samples.dtype]
    return (samples.astype(np.float32) * np.float32(2.0 ** -(bits - 1))).astype(np.float64)


def resample(samples: np.ndarray, nch: int, fin: int, fout: int, Z: int = ZEROS, rolloff: float = ROLLOFF,
             beta: float = BETA, table=None, f32_taps: bool = True) -> np.ndarray:
    """[N_out, nch] float64: the whole resampled stream, summed in float64 over the taps rounded
    to f32 as the library stores them (f32_taps=False: the float64 taps, for the tests that pin
    the formulas). samples: interleaved, container-typed (or float64 frames already)."""
    L, M, W, K, h64 = table if table is not None else taps(fin, fout, Z, rolloff, beta)
    h = h64.astype(np.float32).astype(np.float64) if f32_taps else h64
    x = to_f32(samples) if samples.dtype in CONTAINER_BITS else samples.astype(np.float64)
    x = x.reshape(-1, nch)
    n = x.shape[0]
    N = out_frames(n, fin, fout)
    m = np.arange(N, dtype=np.int64)
    q, r = (m * M) // L, (m * M) % L
    # x padded so that q - W + k is always inside: W before, q_max + W - (n - 1) after
    after = int(max((q.max() if N else 0) + W - (n - 1), 0))
    xp = np.concatenate([np.zeros((W, nch)), x, np.zeros((after, nch))])
    out = np.zeros((N, nch))
    step = max(1, (1 << 22) // K)
    for a in range(0, N, step):
        b = min(N, a + step)
        idx = q[a:b, None] + np.arange(K)[None, :]  # (q - W + k) + W
        out[a:b] = np.einsum("mk,mkc->mc", h[r[a:b]], xp[idx])
    return out


def expected_row(resampled, C: int, T: int, start: int, layout: str):
    """(float64 [C, T] or [T, C], valid frames) of one row; resampled: [N, nch] float64 of the
    whole stream, or None for an error stream. Mirrors export_ref.expected_row."""
    out = np.zeros((T, C))
    valid = 0
    if resampled is not None and resampled.shape[1]:
        valid = int(min(max(resampled.shape[0] - start, 0), T))
        if valid:
            k = min(resampled.shape[1], C)
            out[:valid, :k] = resampled[start:start + valid, :k]
    return (np.ascontiguousarray(out.T) if layout == "planar" else out), valid


def round_bits(f32: np.ndarray, dtype: str) -> np.ndarray:
    """Bit patterns of an f32 array rounded to `dtype` as export_ref.convert_bits rounds."""
    f = np.ascontiguousarray(f32, dtype=np.float32)
    if dtype == "float32":
        return f.view(np.uint32)
    if dtype == "float16":
        return f.astype(np.float16).view(np.uint16)
    assert dtype == "bfloat16" and BIT_VIEW[dtype] is np.uint16
    u = f.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
