"""The float64 reference of a framed feature plan (include/zflac_hip.h, "Framed plans"), written
from the definition with numpy and independent of the library's C++. It runs the sequential
per-frame pipeline in Kaldi's order,

  f = g x[s0 + n], n < Nw;  f -= mean(f) (remove_dc);  y[0] = (1 - a) f[0], y[n] = f[n] - a f[n - 1];
  z = w y;  z zero-extended to N;  rfft;  P = |Z|^2;  v = filters . P;  the log,

and never forms the folded table to get its values. folded() is the table the library is asked to
build (the header's O(Nw) recipe in float64), used for the error bound and checked against the
pipeline in tests/test_fbank_ref.py.

The bound is tests/mel_ref.py's with Nw for N and the folded |c'| in sum |c'| |x|:
  e_re = (Nw + 2) u sum_n |c'[n][k]| |x[n]|,   u = 2^-24
(Nw roundings of a sum of Nw terms in any order, one for the table entry and one for a last-bit
difference between two table builders), propagated through P and v as there. A split plan's
e_re is (summation_factor(Nw, terms) + truncation_factor(terms) + 2 u) sum |c'| |x|: the kernel's
f32 sums of the kept products, the dropped products (tests/mel_bf16_ref.py), and the f32 rounding
of the table against the float64 c'."""
from __future__ import annotations

import numpy as np

from . import mel_bf16_ref, mel_ref

U = mel_ref.U
STFT, SNIP, KALDI_CENTER = 0, 1, 2
PAD_ZEROS, PAD_REFLECT, PAD_MIRROR = 0, 1, 2


def frame_start(framing, t, N, Nw, hop, center):
    """s0(t): the sample index of n = 0 of frame t."""
    if framing == STFT:
        return t * hop - (N // 2 if center else 0) + (N - Nw) // 2
    if framing == SNIP:
        return t * hop
    return t * hop + hop // 2 - Nw // 2


def plan_frames(framing, n, N, Nw, hop, center):
    if framing == STFT:
        return mel_ref.mel_frames(n, N, hop, center)
    if framing == SNIP:
        return (n - Nw) // hop + 1 if n >= Nw else 0
    return (n + hop // 2) // hop


def rho_reflect(s, n):
    """ZFLAC_PAD_REFLECT's index map (the edge sample is not repeated). s: int array."""
    s = np.asarray(s, dtype=np.int64)
    return np.where(s < 0, -s, np.where(s >= n, 2 * (n - 1) - s, s))


def rho_mirror(s, n):
    """ZFLAC_PAD_MIRROR's index map (the edge sample is repeated). s: int array."""
    s = np.asarray(s, dtype=np.int64)
    return np.where(s < 0, -1 - s, np.where(s >= n, 2 * n - 1 - s, s))


def padded(x, n, s, pad, N):
    """x~[s] of one row x (its first n samples are the signal) at the int array s, float64."""
    s = np.asarray(s, dtype=np.int64)
    if pad == PAD_REFLECT:
        r = rho_reflect(s, n)
        ok = (s >= -(N // 2)) & (s < n + N // 2) & (r >= 0) & (r < n)
    elif pad == PAD_MIRROR:
        r = rho_mirror(s, n)
        ok = (r >= 0) & (r < n)
    else:
        r = s
        ok = (s >= 0) & (s < n)
    if n == 0:
        return np.zeros(s.shape)
    return np.where(ok, np.asarray(x, dtype=np.float64)[np.clip(r, 0, n - 1)], 0.0)


def frames_of(x, lengths, framing, pad, N, Nw, hop, center, first, frames):
    """x: [rows, T]; lengths: per row or None -> float64 [rows, frames, Nw], the (padded) samples under
    feature frames first .. first + frames - 1."""
    x = np.asarray(x)
    T = x.shape[1]
    t = first + np.arange(frames, dtype=np.int64)
    idx = frame_start(framing, t, N, Nw, hop, center)[:, None] + np.arange(Nw, dtype=np.int64)[None, :]
    out = np.empty((x.shape[0], frames, Nw))
    for i in range(x.shape[0]):
        n = T if lengths is None else min(int(lengths[i]), T)
        out[i] = padded(x[i], n, idx, pad, N)
    return out


def operator(X, window, a, remove_dc, g):
    """The frame operator on X [..., Nw], step by step -> z [..., Nw] float64."""
    f = g * np.asarray(X, dtype=np.float64)
    if remove_dc:
        f = f - f.mean(axis=-1, keepdims=True)
    y = np.empty_like(f)
    y[..., 0] = (1.0 - a) * f[..., 0]
    y[..., 1:] = f[..., 1:] - a * f[..., :-1]
    return y * np.asarray(window, dtype=np.float64)


def spectrum(X, window, N, a, remove_dc, g):
    """-> (re, im) float64 [..., K] of the zero-extended operated frames."""
    S = np.fft.rfft(operator(X, window, a, remove_dc, g), n=N, axis=-1)
    return S.real, S.imag


def folded(window, N, a, remove_dc, g):
    """c', s' float64 [Nw, K] by the header's recipe: column k of w cos / -w sin (sine exactly 0 at
    k = 0 and k = N / 2) through the transpose of pre-emphasis, of DC removal, and the scale."""
    w = np.asarray(window, dtype=np.float64)
    Nw = w.size
    n, k = np.arange(Nw, dtype=np.int64)[:, None], np.arange(N // 2 + 1, dtype=np.int64)[None, :]
    j = (n * k) % N
    ang = 2.0 * np.pi * j.astype(np.float64) / N
    out = []
    for u in (w[:, None] * np.cos(ang), -w[:, None] * np.where((2 * j) % N == 0, 0.0, np.sin(ang))):
        v = u.copy()
        if Nw > 1:
            v[:-1] = u[:-1] - a * u[1:]
            v[0] = (1.0 - a) * u[0] - a * u[1]
        else:
            v[0] = (1.0 - a) * u[0]
        if remove_dc:
            v = v - v.mean(axis=0, keepdims=True)
        out.append(v * g)
    return out[0], out[1]


def operator_matrix(window, a, remove_dc, g):
    """diag(w) A, dense float64 [Nw, Nw]: column n is the operated, windowed response to a unit sample at n."""
    Nw = np.asarray(window).size
    return operator(np.eye(Nw), window, a, remove_dc, g).T  # column n: the response to a unit sample at n


def propagate(re, im, e_re, e_im, filters):
    return mel_bf16_ref.propagate(re, im, e_re, e_im, filters)


def features(x, lengths, window, filters, N, hop, center, framing, pad, a, remove_dc, g, first, frames, terms=None):
    """-> (v, e_v): float64 [rows, n_bins, frames], the filterbank sums and their bound. terms: None
    (the f32 plan), 6 or 3 (the split plans)."""
    Nw = np.asarray(window).size
    X = frames_of(x, lengths, framing, pad, N, Nw, hop, center, first, frames)
    re, im = spectrum(X, window, N, a, remove_dc, g)
    c, s = folded(window, N, a, remove_dc, g)
    ax = np.abs(X)
    if terms is None:
        factor = (Nw + 2) * U
    else:
        factor = mel_bf16_ref.summation_factor(Nw, terms) + mel_bf16_ref.truncation_factor(terms) + 2 * U
    return propagate(re, im, factor * (ax @ np.abs(c)), factor * (ax @ np.abs(s)), filters)


scaled = mel_ref.scaled
