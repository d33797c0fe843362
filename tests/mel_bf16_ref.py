"""The float64 reference of a split-bf16 feature plan (include/zflac_hip.h, ZFLAC_MEL_MATH_BF16X6 /
_BF16X3), written from the definition with numpy and independent of the library's C++:

  b(v)   v rounded to bfloat16, nearest, ties to even: the integer rule on the f32's bits
  v0 = b(v), v1 = b(v - v0), v2 = b(v - v0 - v1)       (the subtractions are exact in f32)
  re[k] = sum_n sum_{(i,j) kept} c_i[n][k] x_j[n]      kept: i + j <= 2 (six terms) or <= 1 (three)

over the pieces of the f32 tables c = (float)(w cos), s = (float)(-w sin) and of the f32 samples.
Every product of two pieces has 16 significant bits and the float64 sums of a few thousand of them
are exact to 2^-53 of their magnitudes, so re and im are the kept-term sums themselves. Behind
them the reference is tests/mel_ref.py's: P, the filterbank and the propagation of a bound e_re on
re through P and v, with the e_re the caller names.

S[k] = sum_n |c[n][k]| |x[n]| is what the truncation bounds T6 = 3 * 2^-24 S and T3 = 2^-14 S and the
summation bound of the kernel are stated in."""
from __future__ import annotations

import functools

import numpy as np

from . import mel_ref

U = mel_ref.U
TERMS = {6: [(i, j) for i in range(3) for j in range(3) if i + j <= 2], 3: [(0, 0), (0, 1), (1, 0)]}


def bf16(v):
    """float32 array -> the nearest bfloat16 as float32, ties to even."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    low, odd = u & 0xFFFF, (u >> 16) & 1
    up = (low > 0x8000) | ((low == 0x8000) & (odd == 1))
    return ((((u >> 16) + up) << 16) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def pieces(v):
    """float32 array -> [3, ...] float64: v0, v1, v2 with v0 + v1 + v2 == v exactly."""
    r = np.ascontiguousarray(v, dtype=np.float32)
    out = []
    for _ in range(3):
        h = bf16(r)
        nxt = r - h
        assert np.array_equal(nxt.astype(np.float64), r.astype(np.float64) - h.astype(np.float64))  # exact in f32
        out.append(h.astype(np.float64))
        r = nxt
    assert not r.any()
    return np.stack(out)


@functools.lru_cache(maxsize=8)
def _tables(window_bytes, N):
    """The f32 tables c and s [N, K] of the header's definition, and their pieces [3, N, K]."""
    w = np.frombuffer(window_bytes, dtype=np.float32).astype(np.float64)
    n, k = np.arange(N, dtype=np.int64)[:, None], np.arange(N // 2 + 1, dtype=np.int64)[None, :]
    j = (n * k) % N
    ang = 2.0 * np.pi * j.astype(np.float64) / N
    c = (w[:, None] * np.cos(ang)).astype(np.float32)
    s = (-w[:, None] * np.where((2 * j) % N == 0, 0.0, np.sin(ang))).astype(np.float32)
    return c, s, pieces(c), pieces(s)


def spectrum(X, window, terms):
    """X: float32-valued [rows, frames, N] -> (re, im, S_re, S_im), float64 [rows, frames, K]: the kept-term sums
    and S = sum_n |c| |x| for each."""
    w = np.ascontiguousarray(window, dtype=np.float32)
    N = w.size
    c, s, cp, sp = _tables(w.tobytes(), N)
    X32 = np.asarray(X).astype(np.float32)
    assert np.array_equal(X32.astype(np.float64), np.asarray(X, dtype=np.float64))  # the samples are f32 values
    xp = pieces(X32)
    re = sum(xp[j] @ cp[i] for i, j in TERMS[terms])
    im = sum(xp[j] @ sp[i] for i, j in TERMS[terms])
    ax = np.abs(X32.astype(np.float64))
    return re, im, ax @ np.abs(c.astype(np.float64)), ax @ np.abs(s.astype(np.float64))


def propagate(re, im, e_re, e_im, filters):
    """tests/mel_ref.py's propagation of a bound on re and im through P and v -> (v, e_v), [rows, n_bins, frames]."""
    F = np.asarray(filters, dtype=np.float64)
    K = re.shape[-1]
    P = re * re + im * im
    d = 2 * np.abs(re) * e_re + e_re ** 2 + 2 * np.abs(im) * e_im + e_im ** 2
    e_P = d + 3 * U * (P + d)
    aF = np.abs(F).T
    v = P @ F.T
    e_v = e_P @ aF + (K + 1) * U * ((P + e_P) @ aF)
    return v.transpose(0, 2, 1), e_v.transpose(0, 2, 1)


def summation_factor(N, terms):
    """A / S of the kernel's sums: terms * N16 products and two table roundings, each add faithfully rounded
    (2 * 2^-24), over the kept products, whose magnitudes sum to at most S (1 + 2^-7)."""
    N16 = -(-N // 16) * 16
    return (terms * N16 + 2) * 2.0 ** -23 * (1.0 + 2.0 ** -7)


def truncation_factor(terms):
    """T / S: what dropping the products of level i + j > 2 (> 1) can move a sum by."""
    return 3 * 2.0 ** -24 if terms == 6 else 2.0 ** -14


def features_of_frames(X, window, filters, terms, factor=None):
    """-> (v, e_v) with e_re = factor * S (the kernel's summation bound unless given)."""
    N = np.asarray(window).size
    re, im, s_re, s_im = spectrum(X, window, terms)
    f = summation_factor(N, terms) if factor is None else factor
    return propagate(re, im, f * s_re, f * s_im, filters)


def features(x, window, filters, hop, center, first, frames, terms, factor=None):
    """mel_ref.features of a split plan: x [rows, T] -> (v, e_v), float64 [rows, n_bins, frames]."""
    N = np.asarray(window).size
    return features_of_frames(mel_ref.frames_of(x, N, hop, center, first, frames), window, filters, terms, factor)
