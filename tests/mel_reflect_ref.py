"""The reference of zflac_hip_mel_run_ex's padding (include/zflac_hip.h, ZFLAC_PAD_REFLECT), written
from the definition with integer indexing and not with numpy.pad:

  xr[s] = x[rho(s)]  for -N/2 <= s < n + N/2 and 0 <= rho(s) < n, else 0
  rho(s) = -s (s < 0),  2 (n - 1) - s (s >= n),  s otherwise

padded(x, n, N, width) is xr on s = -N/2 .. width - N/2 - 1. A centred frame t of the reflected
row is the uncentred frame t of padded(), so features() feeds tests/mel_ref.py's features with
center = 0 over the padded rows and mel_ref's bound e_v applies as it stands."""
from __future__ import annotations

import numpy as np

from . import mel_ref


def rho(s, n):
    s = np.asarray(s, dtype=np.int64)
    return np.where(s < 0, -s, np.where(s >= n, 2 * (n - 1) - s, s))


def padded(x, n, N, width, reflect=True):
    """x: [T] (only x[:n] is signal) -> float64 [width]: xr[s] (or the zero-extended x[s]) for s = -N/2 + i."""
    x = np.asarray(x, dtype=np.float64)
    n = min(int(n), x.size)
    s = np.arange(width, dtype=np.int64) - N // 2
    r = rho(s, n) if reflect else s
    ok = (s >= -(N // 2)) & (s < n + N // 2) & (r >= 0) & (r < n)
    out = np.zeros(width)
    out[ok] = x[r[ok]]
    return out


def padded_rows(x, lengths, N, hop, first, frames, reflect=True):
    """x: [rows, T] -> float64 [rows, width], wide enough for feature frames first .. first + frames - 1."""
    width = (first + frames - 1) * hop + N
    return np.stack([padded(row, n, N, width, reflect) for row, n in zip(np.asarray(x), lengths)])


def features(x, lengths, window, filters, hop, first, frames, reflect=True):
    """-> (v, e_v) of mel_ref.features for the centred plan with per-row lengths and reflect (or zero) padding."""
    N = np.asarray(window).size
    return mel_ref.features(padded_rows(x, lengths, N, hop, first, frames, reflect), window, filters, hop, 0, first, frames)
