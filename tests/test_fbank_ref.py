"""tests/fbank_ref.py against itself and against values worked by hand, without a GPU: the folded
table reproduces the sequential per-frame pipeline, the frame counts and the two reflections at the
lengths where they change, and the Kaldi windows and filters of zflac_amd.tensor at a tiny size."""
from __future__ import annotations

import numpy as np
import pytest

from . import fbank_ref as R

SHAPES = [(2, 1), (2, 2), (16, 11), (32, 30), (512, 400), (2048, 1201)]


def signals(Nw, frames, seed):
    rng = np.random.default_rng(seed)
    noise = rng.uniform(-1.0, 1.0, (frames, Nw))
    ripple = 0.9 + 1e-3 * np.sin(0.37 * np.arange(frames * Nw)).reshape(frames, Nw)
    return {"noise": noise, "dc_ripple": ripple}


@pytest.mark.parametrize("N,Nw", SHAPES)
@pytest.mark.parametrize("a,dc,g", [(0.0, False, 1.0), (0.97, True, 32768.0), (1.0, False, -0.5), (0.5, True, 1.0)])
def test_folded_table_is_the_sequential_pipeline(N, Nw, a, dc, g):
    """re = x . c', im = x . s' to 1e-11 of sum |c'| |x| (the scale both sides' roundings live on)."""
    w = 0.25 + ((np.arange(Nw) * 37) % 101) / 128.0
    c, s = R.folded(w, N, a, dc, g)
    assert c.shape == s.shape == (Nw, N // 2 + 1)
    for name, X in signals(Nw, 5, N + Nw).items():
        re, im = R.spectrum(X, w, N, a, dc, g)
        for got, want, t in ((X @ c, re, c), (X @ s, im, s)):
            scale = np.abs(X) @ np.abs(t)
            assert np.all(np.abs(got - want) <= 1e-11 * scale + 1e-300), (name, np.max(np.abs(got - want) / (scale + 1e-300)))


@pytest.mark.parametrize("N,Nw", SHAPES)
def test_folded_table_is_the_dense_product(N, Nw):
    """c'[n][k] = sum_m w[m] cos(2 pi m k / N) A[m][n] with A applied densely, column by column."""
    w = 0.25 + ((np.arange(Nw) * 37) % 101) / 128.0
    a, dc, g = 0.97, True, 32768.0
    WA = R.operator_matrix(w, a, dc, g)                      # [m, n]
    m, k = np.arange(Nw)[:, None], np.arange(N // 2 + 1)[None, :]
    ang = 2.0 * np.pi * ((m * k) % N) / N
    c, s = R.folded(w, N, a, dc, g)
    bound = 1e-12 * np.abs(WA).sum(axis=0)[:, None] + 1e-300
    assert np.all(np.abs(WA.T @ np.cos(ang) - c) <= bound)
    assert np.all(np.abs(WA.T @ -np.sin(ang) - s) <= bound)


def lengths_of(Nw):
    return sorted({0, 1, 2, max(Nw // 2 - 1, 0), Nw // 2, max(Nw - 1, 0), Nw, Nw + 1})


@pytest.mark.parametrize("N,Nw,hop", [(2, 1, 1), (16, 11, 3), (32, 30, 7), (512, 400, 160)])
def test_frame_counts(N, Nw, hop):
    for n in lengths_of(Nw) + [20 * hop - 1, 20 * hop, 20 * hop + 1]:
        # snip: the frames that fit; written out as the largest t with t hop + Nw <= n
        fit = [t for t in range(n + 2) if t * hop + Nw <= n]
        assert R.plan_frames(R.SNIP, n, N, Nw, hop, 0) == len(fit)
        # kaldi_center: round(n / hop), halves up for even hop
        assert R.plan_frames(R.KALDI_CENTER, n, N, Nw, hop, 0) == (n + hop // 2) // hop
        assert R.plan_frames(R.STFT, n, N, Nw, hop, 1) == (n // hop + 1 if n else 0)
        assert R.plan_frames(R.STFT, n, N, Nw, hop, 0) == ((n - N) // hop + 1 if n >= N else 0)
    assert R.frame_start(R.SNIP, 3, N, Nw, hop, 0) == 3 * hop
    assert R.frame_start(R.KALDI_CENTER, 0, N, Nw, hop, 0) == hop // 2 - Nw // 2
    assert R.frame_start(R.STFT, 0, N, Nw, hop, 1) == -(N // 2) + (N - Nw) // 2
    assert R.frame_start(R.STFT, 2, N, Nw, hop, 0) == 2 * hop + (N - Nw) // 2


@pytest.mark.parametrize("Nw", [1, 11, 30, 400])
def test_reflections(Nw):
    N = 2 * Nw
    for n in lengths_of(Nw):
        s = np.arange(-N - 2, n + N + 3)
        x = 1.0 + np.arange(max(n, 1), dtype=np.float64)
        mir, ref = R.padded(x, n, s, R.PAD_MIRROR, N), R.padded(x, n, s, R.PAD_REFLECT, N)
        for i, si in enumerate(s):
            # one mirror with the edge sample repeated: ... x1 x0 | x0 x1 ... x[n-1] | x[n-1] x[n-2] ...
            r = -1 - si if si < 0 else (2 * n - 1 - si if si >= n else si)
            assert mir[i] == (x[r] if 0 <= r < n else 0.0), (n, si)
            # one reflection about the edge sample, inside the signal padded by N / 2
            r = -si if si < 0 else (2 * (n - 1) - si if si >= n else si)
            assert ref[i] == (x[r] if 0 <= r < n and -(N // 2) <= si < n + N // 2 else 0.0), (n, si)
    # where one reflection suffices the mirror is numpy's "symmetric", the reflect numpy's "reflect"
    n = Nw + 3
    x = np.arange(1.0, n + 1)
    s = np.arange(-Nw, n + Nw)
    assert np.array_equal(R.padded(x, n, s, R.PAD_MIRROR, N), np.pad(x, Nw, mode="symmetric"))
    assert np.array_equal(R.padded(x, n, s, R.PAD_REFLECT, N), np.pad(x, Nw, mode="reflect"))


def test_kaldi_windows_by_hand():
    from zflac_amd.tensor import kaldi_window

    # Nw = 5: cos(2 pi n / 4) = 1, 0, -1, 0, 1
    assert np.array_equal(kaldi_window("hanning", 5), np.array([0, 0.5, 1, 0.5, 0], dtype=np.float32))
    assert np.array_equal(kaldi_window("hamming", 5), np.array([0.54 - 0.46, 0.54, 0.54 + 0.46, 0.54, 0.54 - 0.46]).astype(np.float32))
    assert np.array_equal(kaldi_window("povey", 5), np.array([0, 0.5 ** 0.85, 1, 0.5 ** 0.85, 0]).astype(np.float32))
    assert np.array_equal(kaldi_window("rectangular", 5), np.ones(5, dtype=np.float32))
    for name in ("povey", "hanning", "hamming", "rectangular"):
        assert np.array_equal(kaldi_window(name, 1), np.ones(1, dtype=np.float32))
        w = kaldi_window(name, 400)
        assert w.dtype == np.float32 and w.shape == (400,) and np.array_equal(w, w[::-1])
    with pytest.raises(ValueError):
        kaldi_window("hann", 5)
    with pytest.raises(ValueError):
        kaldi_window("povey", 0)


def test_kaldi_filters_by_hand():
    from zflac_amd.tensor import kaldi_mel_filters

    # sr 8000, N 16: bins every 500 Hz, k < 8; two filters over [0, 4000] Hz
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)  # noqa: E731
    fb = kaldi_mel_filters(8000, 16, 2, low_freq=0.0, high_freq=0.0)
    assert fb.shape == (2, 9) and fb.dtype == np.float32
    hi = mel(4000.0)
    d = hi / 3.0
    want = np.zeros((2, 9))
    for m in range(2):
        left, centre, right = m * d, (m + 1) * d, (m + 2) * d
        for k in range(8):
            mk = mel(500.0 * k)
            if left < mk < right:
                want[m, k] = (mk - left) / d if mk <= centre else (right - mk) / d
    assert np.array_equal(fb, want.astype(np.float32))
    assert not fb[:, 8].any() and not fb[:, 0].any()      # the Nyquist column; mel(0) is on the left edge, not inside
    # d = 715.4: mel(500) = 607.4 is nearest the first centre, mel(2000) = 1521.4 the second (1430.7)
    assert fb[0].argmax() == 1 and fb[1].argmax() == 4
    assert abs(fb[0, 1] - 607.4 / 715.4) < 1e-3 and abs(fb[1, 4] - (2146.1 - 1521.4) / 715.4) < 1e-3
    assert np.all(fb >= 0) and np.all(fb <= 1)
    # a negative high_freq is an offset from Nyquist; the defaults are Kaldi's 20 Hz .. Nyquist
    assert np.array_equal(kaldi_mel_filters(8000, 16, 2, 0.0, -500.0), kaldi_mel_filters(8000, 16, 2, 0.0, 3500.0))
    k80 = kaldi_mel_filters(16000, 512, 80)
    assert k80.shape == (80, 257) and np.all(k80.sum(axis=1) > 0) and not k80[:, 256].any()
    with pytest.raises(ValueError):
        kaldi_mel_filters(8000, 16, 2, 100.0, 50.0)
