"""GPU tests of zflac_hip_mel_cmvn (k_mel_cmvn): both modes, both ddof values, both layouts and the
three dtypes against a float64 reference taken from the stored values; valid lengths around the
workgroup's strides; frames past a row's valid length; misaligned destinations with guard elements;
runs repeat bit for bit and a row's bits depend neither on the batch nor on the alignment; and
MelSpectrogram(cmvn=...).

The tolerance per element, with l the stored input, mu and sigma the float64 statistics,
r = 1 / (sigma + eps) and ref = (l - mu) r:
  2^-22 |ref| + 2^-23 (|l| + |mu|) r  (+ the output dtype's own rounding, u_dt |ref|, for f16 / bf16)
mu32 and r are one f32 rounding each (2^-24 relative), the subtraction and the product one each:
|l - mu32 - (l - mu)| <= 2^-24 |mu| and the subtraction's rounding 2^-24 |l - mu32| <= 2^-24 (|l| + |mu|),
times r: 2^-23 (|l| + |mu|) r with a factor 2 in hand; the roundings of r and of the product are
2 * 2^-24 |ref|, again doubled. The device's f64 sums differ from numpy's by parts in 2^-45."""
import ctypes

import torch  # before zflac_amd loads its library: one HIP runtime per process (zflac_amd/tensor.py)

import numpy as np
import pytest

from zflac_amd import _lib, errors, tensor

from .test_mel_reflect import DEV, TORCH_DT, same_bits

pytestmark = pytest.mark.gpu

U_DT = {_lib.EXPORT_F32: 0.0, _lib.EXPORT_F16: 2.0 ** -11, _lib.EXPORT_BF16: 2.0 ** -8}
MEAN, MEAN_VAR = _lib.CMVN_MEAN, _lib.CMVN_MEAN_VAR
GUARD = 7  # elements before and behind a misaligned tensor


class Plan:
    """A plan only to carry the dtype, the layout and the bin count to zflac_hip_mel_cmvn."""

    def __init__(self, n_bins, layout, dtype):
        tensor.check_single_runtime()
        self.L = _lib.load()
        self.n_bins, self.layout, self.dtype = n_bins, layout, dtype
        w, f = np.ones(2, np.float32), np.ones((n_bins, 2), np.float32)
        d = _lib.zflac_mel_desc(ctypes.sizeof(_lib.zflac_mel_desc), dtype, layout, _lib.MEL_POWER, 0, 2, 1, n_bins, 0, 0.0,
                                w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), f.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        self.h = ctypes.c_void_p()
        errors.check(self.L.zflac_hip_mel_create(ctypes.byref(d), 0, ctypes.byref(self.h)), "mel_create")

    def cmvn(self, feat_ptr, rows, frames, mode, ddof, valid=None, eps=1e-5, pad=0.0, stats=True):
        """In place at feat_ptr -> (mean, std) [rows, n_bins] float32 (NaN-filled before the call), or None."""
        v = None if valid is None else torch.tensor([int(n) for n in valid], dtype=torch.int64, device=DEV)
        mean = torch.full((rows, self.n_bins), float("nan"), device=DEV) if stats else None
        std = torch.full((rows, self.n_bins), float("nan"), device=DEV) if stats else None
        c = _lib.zflac_mel_cmvn_desc(ctypes.sizeof(_lib.zflac_mel_cmvn_desc), mode, ddof, 0, feat_ptr, rows, frames,
                                     None if v is None else v.data_ptr(), mean.data_ptr() if stats else None,
                                     std.data_ptr() if stats else None, eps, pad)
        torch.cuda.synchronize()
        errors.check(self.L.zflac_hip_mel_cmvn(self.h, ctypes.byref(c), None), "mel_cmvn")
        return mean, std

    def close(self):
        if self.h:
            self.L.zflac_hip_mel_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def features(rows, n_bins, frames, layout, dtype, seed):
    """Log-mel-like values, stored in the dtype and layout: [rows, n_bins, frames] or [rows, frames, n_bins]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, n_bins, frames, generator=g) * 3.0 - 5.0 + torch.arange(n_bins).view(1, -1, 1) * 0.05
    x[:, 0] = 1.5  # a constant bin: sigma = 0
    x = x.to(TORCH_DT[dtype])
    return (x if layout == 0 else x.transpose(1, 2)).contiguous().to(DEV)


def reference(x, layout, valid, mode, ddof, eps, pad, dtype):
    """x: the stored input (torch, on the host or the device) -> (out, tol, mean, std) in float64, [rows, n_bins, frames]."""
    l = (x if layout == 0 else x.transpose(1, 2)).double().cpu().numpy()
    rows, n_bins, frames = l.shape
    out, tol = np.empty_like(l), np.zeros_like(l)
    mean, std = np.zeros((rows, n_bins)), np.zeros((rows, n_bins))
    padv = float(torch.tensor(pad, dtype=torch.float32).to(TORCH_DT[dtype]).double())
    for i in range(rows):
        F = frames if valid is None else min(int(valid[i]), frames)
        out[i, :, F:] = padv
        if F == 0:
            continue
        v = l[i, :, :F]
        mu = v.sum(axis=1) / F
        div = max(F - ddof, 0)
        sigma = np.sqrt(((v - mu[:, None]) ** 2).sum(axis=1) / div) if div and mode == MEAN_VAR else np.zeros(n_bins)
        den = sigma + float(np.float32(eps))
        r = np.where(den == 0, 0.0, 1.0 / np.where(den == 0, 1.0, den)) if mode == MEAN_VAR else np.ones(n_bins)
        o = (v - mu[:, None]) * r[:, None]
        out[i, :, :F] = o
        tol[i, :, :F] = 2.0 ** -22 * np.abs(o) + 2.0 ** -23 * (np.abs(v) + np.abs(mu)[:, None]) * r[:, None] + \
            U_DT[dtype] * np.abs(o) + (2.0 ** -25 if dtype == _lib.EXPORT_F16 else 0.0)
        mean[i], std[i] = mu, sigma
    return out, tol, mean, std


def view(t, layout):
    return t if layout == 0 else t.transpose(1, 2)


@pytest.mark.parametrize("dtype", [_lib.EXPORT_F32, _lib.EXPORT_F16, _lib.EXPORT_BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("layout", [0, 1], ids=["bins_first", "frames_first"])
@pytest.mark.parametrize("n_bins,frames", [(80, 130), (5, 133), (33, 1031)])
def test_against_float64(gpu_ready, n_bins, frames, layout, dtype):
    valid = [0, 1, 2, 127, 128, 129, frames]
    rows = len(valid)
    worst = 0.0
    with Plan(n_bins, layout, dtype) as p:
        for mode, ddof, eps, pad in ((MEAN_VAR, 0, 1e-5, 0.0), (MEAN_VAR, 1, 0.0, -2.5), (MEAN, 0, 1e-5, 1e30), (MEAN, 1, 0.0, 0.0)):
            if dtype == _lib.EXPORT_F16 and pad == 1e30:
                pad = 60000.0
            x = features(rows, n_bins, frames, layout, dtype, 100 * n_bins + frames)
            want, tol, mu, sigma = reference(x, layout, valid, mode, ddof, eps, pad, dtype)
            y = x.clone()
            mean, std = p.cmvn(y.data_ptr(), rows, frames, mode, ddof, valid, eps, pad)
            got = view(y, layout).double().cpu().numpy()
            assert np.isfinite(got).all()
            err = np.abs(got - want)
            exact = tol == 0  # the frames past F_i hold pad_value exactly, and r = 0 stores exact zeros
            assert (err[exact] == 0).all(), (mode, ddof)
            if (~exact).any():
                worst = max(worst, float((err[~exact] / tol[~exact]).max()))
            assert worst <= 1.0, (mode, ddof, worst)
            m, s = mean.double().cpu().numpy(), std.double().cpu().numpy()
            assert np.all(np.abs(m - mu) <= 2.0 ** -23 * np.abs(mu)) and not m[0].any() and not s[0].any()
            assert np.all(np.abs(s - sigma) <= 2.0 ** -23 * np.abs(sigma))
            # again: the same bits, and without the optional outputs and lengths too
            z = x.clone()
            p.cmvn(z.data_ptr(), rows, frames, mode, ddof, valid, eps, pad, stats=False)
            assert same_bits(y, z)
            full = x.clone()
            p.cmvn(full.data_ptr(), rows, frames, mode, ddof, None, eps, pad)
            assert same_bits(full[rows - 1], y[rows - 1])  # valid = frames is no lengths
    print(f"cmvn bins {n_bins} frames {frames} layout {layout} dtype {dtype}: worst error / bound = {worst:.4f}")


@pytest.mark.parametrize("dtype", [_lib.EXPORT_F32, _lib.EXPORT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", [0, 1], ids=["bins_first", "frames_first"])
def test_a_rows_bits_alone_in_a_batch_and_misaligned(gpu_ready, layout, dtype):
    n_bins, frames, rows = 80, 129, 5
    es = 4 if dtype == _lib.EXPORT_F32 else 2
    with Plan(n_bins, layout, dtype) as p:
        x = features(rows, n_bins, frames, layout, dtype, 9)
        valid = [129, 77, 128, 1, 129]
        batch = x.clone()
        p.cmvn(batch.data_ptr(), rows, frames, MEAN_VAR, 1, valid)
        for i in (0, 1, 4):  # a row alone, wherever it sat in the batch
            alone = x[i:i + 1].clone()
            p.cmvn(alone.data_ptr(), 1, frames, MEAN_VAR, 1, valid[i:i + 1])
            assert same_bits(alone, batch[i:i + 1]), i
        n = x.numel()
        for shift in (1, 2, 3, 5):  # elements off the allocation's 16-byte boundary
            buf = torch.full((n + 2 * GUARD,), 123.0, dtype=x.dtype, device=DEV)
            start = GUARD + shift - 4  # 4, 5, 6 and 8 elements into the buffer
            buf[start:start + n] = x.reshape(-1)
            p.cmvn(buf.data_ptr() + es * start, rows, frames, MEAN_VAR, 1, valid)
            assert same_bits(buf[start:start + n].view(x.shape), batch), shift
            assert bool((buf[:start] == 123.0).all()) and bool((buf[start + n:] == 123.0).all()), shift


def test_melspectrogram_cmvn(gpu_ready):
    """MelSpectrogram(cmvn=...) is the features, then zflac_hip_mel_cmvn over feature_lengths."""
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.uniform(-1, 1, (3, 16000 // 4)).astype(np.float32)).to(DEV)
    lengths = torch.tensor([4000, 1234, 0])
    with tensor.MelSpectrogram.kaldi_fbank(cmvn="mean_var", cmvn_ddof=1, cmvn_pad=-1.0) as m, \
            tensor.MelSpectrogram.kaldi_fbank() as plain:
        f, fl = m(x, lengths)
        g, gl = plain(x, lengths)
        torch.cuda.synchronize()
        assert torch.equal(fl, gl) and fl.tolist() == [23, 6, 0]
        want, tol, mu, sigma = reference(g, 1, fl.tolist(), MEAN_VAR, 1, 1e-5, -1.0, _lib.EXPORT_F32)
        err = np.abs(f.transpose(1, 2).double().cpu().numpy() - want)
        assert (err <= tol).all() and (err[tol == 0] == 0).all()
        assert bool((f[2] == -1.0).all()) and bool((f[1, 6:] == -1.0).all())
        assert m.last_mean.shape == (3, 80) and np.abs(m.last_mean.double().cpu().numpy() - mu).max() < 1e-5
        assert np.abs(m.last_std.double().cpu().numpy() - sigma).max() < 1e-5
