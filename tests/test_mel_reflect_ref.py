"""tests/mel_reflect_ref.py, the reference of ZFLAC_PAD_REFLECT, against numpy.pad(mode="reflect")
and, for n > N / 2, against torch.stft(center=True, pad_mode="reflect") on the CPU; and what the
rule says where numpy has no answer (n <= N / 2). No GPU."""
import numpy as np
import pytest
import torch

from . import mel_ref
from . import mel_reflect_ref as rr


@pytest.mark.parametrize("N,n", [(16, 50), (16, 9), (2, 2), (2, 5), (400, 201), (400, 1000), (30, 16), (2048, 1025)])
def test_padded_is_numpy_reflect(N, n):
    x = np.random.default_rng(N + n).uniform(-1, 1, n + 7)
    x[n:] = 1e30  # past the length: never signal
    got = rr.padded(x, n, N, n + N)
    assert np.array_equal(got, np.pad(x[:n], N // 2, mode="reflect"))
    assert np.array_equal(rr.padded(x, n, N, n + N + 40)[n + N:], np.zeros(40))  # zero beyond the one reflection
    assert np.array_equal(rr.padded(x, n, N, n + N, reflect=False), np.pad(x[:n], N // 2))
    assert np.array_equal(rr.padded(x, n + 100, N, n + 7 + N), np.pad(x, N // 2, mode="reflect"))  # clamped to the row


def test_short_rows_follow_the_rule():
    N = 8
    x = np.arange(1.0, 6.0)
    assert np.array_equal(rr.padded(x, 0, N, 12), np.zeros(12))
    # n = 1: rho(s) = -s left of 0 and -s right of it: only s = 0 lands inside the row
    assert np.array_equal(rr.padded(x, 1, N, 12), [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0])
    # n = 3 <= N / 2: x[3] x[2] x[1] | x[0] x[1] x[2] | x[1] x[0] x[-1] ...: out-of-row indices are zero
    assert np.array_equal(rr.padded(x, 3, N, 12), [0, 0, 3, 2, 1, 2, 3, 2, 1, 0, 0, 0])
    # n = N / 2: one index short of a full reflection on the left
    assert np.array_equal(rr.padded(x, 4, N, 12), [0, 4, 3, 2, 1, 2, 3, 4, 3, 2, 1, 0])


@pytest.mark.parametrize("N,hop,n", [(16, 3, 50), (400, 160, 1000), (30, 7, 16)])
def test_features_against_torch_stft(N, hop, n):
    rng = np.random.default_rng(N)
    x = rng.uniform(-1, 1, (2, n)).astype(np.float32)
    w = mel_ref.hann(N)
    F = rng.uniform(0, 1, (5, N // 2 + 1)).astype(np.float32)
    frames = n // hop + 1
    v, e_v = rr.features(x, [n, n], w, F, hop, 0, frames)
    try:
        s = torch.stft(torch.from_numpy(x).double(), N, hop, window=torch.from_numpy(w).double(), center=True,
                       pad_mode="reflect", return_complex=True)
    except RuntimeError as e:  # a build without a CPU FFT
        pytest.skip(f"torch.stft does not run here: {e}")
    want = (torch.from_numpy(F).double() @ (s.abs() ** 2)).numpy()
    assert want.shape == v.shape
    assert np.allclose(v, want, rtol=1e-10, atol=1e-12)
    assert e_v.shape == v.shape and (e_v >= 0).all()
