"""The float64 reference of the cepstra plans (include/zflac_hip.h: zflac_hip_cepstra_project,
zflac_hip_cepstra_deltas): the projection of every frame's bins by a matrix, and Kaldi's deltas as
one clamped sum over the *base* features. numpy only; tensors are [rows, C, frames]."""
from __future__ import annotations

import numpy as np


def dct_closed_form(n_ceps, n_mels, norm="ortho", lifter=0.0):
    """Entry by entry, from the definition: float64 [n_ceps, n_mels]."""
    d = np.empty((n_ceps, n_mels), dtype=np.float64)
    for k in range(n_ceps):
        for m in range(n_mels):
            c = np.cos(np.pi * k * (m + 0.5) / n_mels)
            if norm == "ortho":
                c *= np.sqrt(1.0 / n_mels) if k == 0 else np.sqrt(2.0 / n_mels)
            else:
                c *= 2.0
            if lifter > 0.0:
                c *= 1.0 + 0.5 * lifter * np.sin(np.pi * k / lifter)
            d[k, m] = c
    return d


def project(T, x):
    """T: [n_out, n_in]; x: [rows, n_in, frames] -> (out, mag) float64 [rows, n_out, frames]:
    sum_m T[k][m] x[m] and sum_m |T[k][m]| |x[m]| (what the error bound scales with)."""
    T, x = np.asarray(T, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return np.einsum("km,rmf->rkf", T, x), np.einsum("km,rmf->rkf", np.abs(T), np.abs(x))


def delta_scales(order, window):
    """Kaldi's taps by the recurrence, element by element: float64 [2 order window + 1]."""
    norm = float(sum(j * j for j in range(-window, window + 1)))
    s = [1.0]
    for _ in range(order):
        nxt = [0.0] * (len(s) + 2 * window)
        for i, v in enumerate(s):
            for j in range(-window, window + 1):
                nxt[i + j + window] += v * (j / norm)
        s = nxt
    return np.array(s, dtype=np.float64)


def deltas(x, order, window, valid=None, pad=0.0, scales=None):
    """x: [rows, C, frames] -> (out, mag) float64 [rows, (order + 1) C, frames]. Block o at
    t < F_i: sum_j s_o[j] x[c][clamp(t + j, 0, F_i - 1)]; at t >= F_i: pad. mag: sum_j |s_o[j]| |x[..]|
    (block 0: 0, it is a copy). scales: the taps per order (default: delta_scales in float64)."""
    x = np.asarray(x, dtype=np.float64)
    rows, C, frames = x.shape
    out = np.full((rows, (order + 1) * C, frames), float(pad), dtype=np.float64)
    mag = np.zeros_like(out)
    for i in range(rows):
        F = frames if valid is None else min(int(valid[i]), frames)
        if F == 0:
            continue
        t = np.arange(F)
        out[i, :C, :F] = x[i, :, :F]
        for o in range(1, order + 1):
            s = delta_scales(o, window) if scales is None else np.asarray(scales[o], dtype=np.float64)
            acc, m = np.zeros((C, F)), np.zeros((C, F))
            for n, j in enumerate(range(-o * window, o * window + 1)):
                v = x[i][:, np.clip(t + j, 0, F - 1)]
                acc += s[n] * v
                m += abs(s[n]) * np.abs(v)
            out[i, o * C:(o + 1) * C, :F] = acc
            mag[i, o * C:(o + 1) * C, :F] = m
    return out, mag


def delta_of_delta(x, window):
    """The order-1 operator applied twice, each time with the index clamped (what
    torchaudio.functional.compute_deltas applied twice computes): [rows, C, frames]."""
    d1 = deltas(x, 1, window)[0][:, x.shape[1]:]
    return deltas(d1, 1, window)[0][:, x.shape[1]:]
