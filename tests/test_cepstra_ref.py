"""The float64 reference of the cepstra plans (tests/cepstra_ref.py) and the host recipes users get
(zflac_amd.tensor.dct_matrix, delta_scales), without a GPU: the DCT against its closed form and
its orthonormality, Kaldi's lifter at hand-worked points, the delta taps against integer tables,
order-1 deltas against a convolution over a replicate-padded row, and the difference between
Kaldi's order-2 deltas and delta-of-delta, which lives within 2 W frames of a row's ends."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from zflac_amd import tensor

from . import cepstra_ref as R


@pytest.mark.parametrize("n_ceps,n_mels", [(1, 1), (2, 2), (3, 5), (13, 23), (13, 80), (40, 80), (256, 256)])
@pytest.mark.parametrize("norm", ["ortho", None])
@pytest.mark.parametrize("lifter", [0.0, 22.0])
def test_dct_matrix_is_the_closed_form_rounded_once(n_ceps, n_mels, norm, lifter):
    got = tensor.dct_matrix(n_ceps, n_mels, norm, lifter)
    want = R.dct_closed_form(n_ceps, n_mels, norm, lifter)
    assert got.dtype == np.float32 and got.shape == (n_ceps, n_mels)
    # two float64 evaluations differ by parts in 2^-50; then one f32 rounding
    assert np.all(np.abs(got.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 2.0 ** -45 + 2.0 ** -150)
    if norm == "ortho" and lifter == 0.0:
        assert np.all(got[0] == np.float32(np.sqrt(1.0 / n_mels)))


@pytest.mark.parametrize("n", [1, 2, 23, 80, 256])
def test_the_orthonormal_dct_is_orthonormal(n):
    D = R.dct_closed_form(n, n)
    assert np.abs(D @ D.T - np.eye(n)).max() <= 1e-12
    # and the f32 matrix is that one to rounding
    assert np.abs(tensor.dct_matrix(n, n).astype(np.float64) - D).max() <= 2.0 ** -24


def test_kaldi_lifter_values():
    """1 + (Q / 2) sin(pi k / Q), Q = 22. k = 0: 1. k = 11: sin(pi / 2) = 1, so 12. k = 1:
    sin(pi / 22) = x - x^3 / 6 + x^5 / 120 at x = 0.1427996661 = 0.1423148383, times 11 plus 1 =
    2.565463221. k = 12: sin(12 pi / 22) = cos(pi / 22) = 1 - x^2 / 2 + x^4 / 24 - x^6 / 720 =
    0.9898214419, times 11 plus 1 = 11.88803586."""
    want = {0: 1.0, 1: 2.565463221, 11: 12.0, 12: 11.88803586}
    plain, lifted = R.dct_closed_form(13, 23), R.dct_closed_form(13, 23, lifter=22.0)
    f32, f32_lifted = tensor.dct_matrix(13, 23), tensor.dct_matrix(13, 23, lifter=22.0)
    for k, v in want.items():
        assert np.allclose(lifted[k] / plain[k], v, rtol=1e-8, atol=0)
        assert np.allclose(f32_lifted[k].astype(np.float64) / f32[k].astype(np.float64), v, rtol=2.0 ** -22, atol=0)


def test_delta_scales_against_integer_tables():
    tables = {
        (1, 2): np.array([-2, -1, 0, 1, 2]) / 10.0,
        (2, 2): np.array([4, 4, 1, -4, -10, -4, 1, 4, 4]) / 100.0,
        # W = 1: s_1 = [-1, 0, 1] / 2; s_2 = s_1 * s_1 = [1, 0, -2, 0, 1] / 4; s_3 = s_2 * s_1 = [-1, 0, 3, 0, -3, 0, 1] / 8
        (3, 1): np.array([-1, 0, 3, 0, -3, 0, 1]) / 8.0,
        # W = 5: sum j^2 = 2 (1 + 4 + 9 + 16 + 25) = 110
        (1, 5): np.arange(-5, 6) / 110.0,
        (0, 3): np.array([1.0]),
    }
    for (order, window), want in tables.items():
        for got in (tensor.delta_scales(order, window), R.delta_scales(order, window)):
            assert got.dtype == np.float64 and got.shape == want.shape
            assert np.abs(got - want).max() <= 2.0 ** -52, (order, window)
    for order in (1, 2, 3):
        for window in (1, 2, 3, 4, 5):
            s = tensor.delta_scales(order, window)
            assert np.abs(s - R.delta_scales(order, window)).max() <= 2.0 ** -52
            assert np.allclose(s, (-1) ** order * s[::-1], rtol=0, atol=2.0 ** -52)  # odd orders antisymmetric
            assert abs(s.sum()) <= 2.0 ** -50  # a derivative of a constant is 0


def test_refusals_of_the_recipes():
    for bad in (dict(n_ceps=0, n_mels=5), dict(n_ceps=6, n_mels=5), dict(n_ceps=1, n_mels=257),
                dict(n_ceps=2, n_mels=5, norm="slaney"), dict(n_ceps=2, n_mels=5, lifter=-1.0),
                dict(n_ceps=2, n_mels=5, lifter=float("nan"))):
        with pytest.raises(ValueError):
            tensor.dct_matrix(**bad)
    for order, window in ((4, 2), (-1, 2), (1, 0), (1, 6)):
        with pytest.raises(ValueError):
            tensor.delta_scales(order, window)


def test_projection_reference():
    rng = np.random.default_rng(1)
    T, x = rng.standard_normal((3, 5)), rng.standard_normal((2, 5, 7))
    out, mag = R.project(T, x)
    for r in range(2):
        for f in range(7):
            assert np.allclose(out[r, :, f], T @ x[r, :, f], rtol=0, atol=1e-14)
            assert np.allclose(mag[r, :, f], np.abs(T) @ np.abs(x[r, :, f]), rtol=0, atol=1e-14)
    # an all-equal frame: only c0 is non-zero
    D = R.dct_closed_form(13, 23)
    out, _ = R.project(D, np.full((1, 23, 1), -7.25))
    assert abs(out[0, 0, 0] + 7.25 * np.sqrt(23.0)) <= 1e-12 and np.abs(out[0, 1:, 0]).max() <= 1e-13


@pytest.mark.parametrize("window", [1, 2, 5])
def test_order_1_deltas_are_a_convolution_over_a_replicate_padded_row(window):
    rng = np.random.default_rng(window)
    x = rng.standard_normal((2, 3, 40))
    got = R.deltas(x, 1, window)[0][:, 3:]
    xp = torch.nn.functional.pad(torch.from_numpy(x), (window, window), mode="replicate")
    kernel = torch.from_numpy(R.delta_scales(1, window)).view(1, 1, -1)  # conv1d correlates: tap j meets x[t + j]
    want = torch.nn.functional.conv1d(xp.reshape(6, 1, -1), kernel).reshape(2, 3, 40).numpy()
    assert np.abs(got - want).max() <= 1e-14
    # and with a valid length: the clamp is at F - 1 and nothing behind it is read
    y = x.copy()
    y[0, :, 17:] = 1e30
    cut = R.deltas(y, 1, window, valid=[17, 40], pad=-3.0)[0]
    assert np.abs(cut[0, 3:, :17] - R.deltas(x[:1, :, :17], 1, window)[0][0, 3:]).max() == 0
    assert np.all(cut[0, :, 17:] == -3.0) and np.array_equal(cut[1], R.deltas(x[1:], 1, window)[0][0])


@pytest.mark.parametrize("window", [1, 2, 5])
def test_order_2_deltas_are_not_delta_of_delta_at_the_ends(window):
    """Kaldi's ComputeDeltas is one clamped pass over the base features. Applying the order-1
    operator twice clamps the *deltas* at the ends instead: the two agree wherever neither clamp
    is reached, t in [2 W, frames - 2 W), and differ inside 2 W frames of either end."""
    rng = np.random.default_rng(10 + window)
    x = rng.standard_normal((1, 4, 50))
    kaldi = R.deltas(x, 2, window)[0][:, 8:]
    twice = R.delta_of_delta(x, window)
    inner = slice(2 * window, 50 - 2 * window)
    assert np.abs(kaldi[..., inner] - twice[..., inner]).max() <= 1e-14
    head, tail = np.abs(kaldi - twice)[..., :2 * window], np.abs(kaldi - twice)[..., 50 - 2 * window:]
    assert head.max() > 1e-3 and tail.max() > 1e-3
    # every feature row differs somewhere in each end zone
    assert np.all(head.max(axis=-1) > 1e-6) and np.all(tail.max(axis=-1) > 1e-6)


def test_delta_blocks_and_scales_argument():
    x = np.arange(2 * 3 * 9, dtype=np.float64).reshape(2, 3, 9) ** 1.5
    out, mag = R.deltas(x, 3, 1, valid=[9, 0], pad=5.0)
    assert out.shape == (2, 12, 9) and np.array_equal(out[0, :3], x[0]) and np.all(out[1] == 5.0)
    assert np.all(mag[0, :3] == 0) and np.all(mag[1] == 0)
    same, _ = R.deltas(x, 3, 1, valid=[9, 0], pad=5.0, scales={o: R.delta_scales(o, 1) for o in (1, 2, 3)})
    assert np.array_equal(out, same)
