"""The float64 reference of the log-mel features (include/zflac_hip.h, "log-mel features"), written
from the definition with numpy's FFT and independent of the library's C++, and the elementwise
error bound of an f32 implementation that sums in any order.

With u = 2^-24, per frame and bin (sums over n) and per filter (sums over k):
  e_re = (N + 2) u sum_n |w[n] cos| |x|            (e_im likewise, with sin)
  e_P  = d + 3 u (P + d),   d = 2 |re| e_re + e_re^2 + 2 |im| e_im + e_im^2
  e_v  = sum_k |F| e_P + (K + 1) u sum_k |F| (P + e_P)
N roundings of a sum of N terms in any order, one for the table entry and one for a last-bit
difference between two table builders. A log output may be off by
  e_v / (ln b max(v - e_v, floor)) + 2^-21 max(1, |out|),
the second term a few ulps for the device's log and its constant multiply."""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24
POWER, LOG10, LN = 0, 1, 2


def hann(N):
    """The periodic Hann window, float32."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)


def mel_frames(n, N, hop, center):
    if center:
        return n // hop + 1 if n else 0
    return (n - N) // hop + 1 if n >= N else 0


@functools.lru_cache(maxsize=4)
def _abs_basis(N):
    n, k = np.arange(N, dtype=np.int64)[:, None], np.arange(N // 2 + 1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((n * k) % N).astype(np.float64) / N
    return np.abs(np.cos(ang)), np.abs(np.sin(ang))


def frames_of(x, N, hop, center, first, frames):
    """x: [rows, T] -> float64 [rows, frames, N]: the samples under feature frames first .. first + frames - 1,
    zero outside the row."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[1]
    idx = (first + np.arange(frames, dtype=np.int64))[:, None] * hop - (N // 2 if center else 0) + np.arange(N, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < T)
    if T == 0:
        return np.zeros((x.shape[0], frames, N))
    return np.where(ok[None], x[:, np.clip(idx, 0, T - 1)], 0.0)


def features(x, window, filters, hop, center, first, frames):
    """-> (v, e_v): float64 [rows, n_bins, frames], the filterbank sums and their bound."""
    w = np.asarray(window, dtype=np.float64)
    F = np.asarray(filters, dtype=np.float64)
    N = w.size
    K = N // 2 + 1
    X = frames_of(x, N, hop, center, first, frames)
    S = np.fft.rfft(X * w, axis=-1)
    re, im = S.real, S.imag
    ac, asn = _abs_basis(N)
    ax = np.abs(X) * np.abs(w)
    e_re = (N + 2) * U * (ax @ ac)
    e_im = (N + 2) * U * (ax @ asn)
    P = re * re + im * im
    d = 2 * np.abs(re) * e_re + e_re ** 2 + 2 * np.abs(im) * e_im + e_im ** 2
    e_P = d + 3 * U * (P + d)
    aF = np.abs(F).T
    v = P @ F.T
    e_v = e_P @ aF + (K + 1) * U * ((P + e_P) @ aF)
    return v.transpose(0, 2, 1), e_v.transpose(0, 2, 1)


def scaled(v, e_v, scale, floor):
    """-> (out, tol) of a scale: POWER is (v, e_v)."""
    if scale == POWER:
        return v, e_v
    log, lnb = (np.log10, np.log(10.0)) if scale == LOG10 else (np.log, 1.0)
    out = log(np.maximum(v, floor))
    tol = e_v / (lnb * np.maximum(v - e_v, floor)) + 2.0 ** -21 * np.maximum(1.0, np.abs(out))
    return out, tol
