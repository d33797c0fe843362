"""End to end: zflac_hip_cepstra_cmvn is zflac_hip_mel_cmvn; MelSpectrogram.kaldi_mfcc() and
kaldi_fbank(deltas=(2, 2), cmvn="mean_var") through decode_to_features on golden streams against the
stepwise float64 pipeline (tests/fbank_ref.py, cepstra_ref, the CMVN reference of test_cmvn.py,
the deltas); a MelSpectrogram call against the explicit sequence of ABI calls, bit for bit; and
the Python surface (n_features, out=, both layouts, the unchanged plain plan).

How the stages' bounds compose. Stage k's device output y_k is within e_k of the float64 value of
the exact pipeline. A linear stage L with its own bound b(.) (a sum in f32 over its stored input)
gives e_{k+1} = |L| e_k + b(|y_k| + e_k) + the output rounding: the projection with |T|, the deltas
with |s_o| at the clamped frames. CMVN is not linear, so its step is bounded directly: with
d = l - mu, a = e + mean(e) bounds the change of d, b = rms(a) that of sigma (the triangle
inequality on ||d|| / sqrt(F), ddof = 0), r' = 1 / (sigma - b + eps) >= both r's, and
|out' - out| <= a r' + |d| r b r', to which test_cmvn.py's bound of the kernel itself is added."""
import os

import numpy as np
import pytest
import torch

from zflac_amd import _lib, tensor

from . import cepstra_ref as C
from . import fbank_ref as R
from . import mel_ref as ref
from .cepstra_gpu import BF16, DEV, F16, F32, TORCH_DT, Cepstra, same_bits
from .test_cmvn import MEAN, MEAN_VAR, Plan as MelCarrier, features as cmvn_features

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STREAMS = ["c3_ms16_lpc8.flac", "c2_mono16_fixed2_k4.flac", "mono8_lpc3.flac", "stereo12_ms_rice2.flac"]
U = 2.0 ** -24


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("layout", [0, 1], ids=["bins_first", "frames_first"])
@pytest.mark.parametrize("n_out", [13, 80, 256])
def test_cepstra_cmvn_is_mel_cmvn(gpu_ready, n_out, layout, dtype):
    """The same kernel launch on the same bytes: the same bits, statistics included."""
    rows, frames = 4, 131
    valid = [131, 64, 1, 0]
    x = cmvn_features(rows, n_out, frames, layout, dtype, 31)
    T = np.zeros((n_out, 7), np.float32)
    with MelCarrier(n_out, layout, dtype) as m, Cepstra(7, n_out, layout, F32, dtype, T) as c:
        for mode, ddof, eps, pad in ((MEAN_VAR, 0, 1e-5, 0.0), (MEAN_VAR, 1, 0.0, -2.5), (MEAN, 0, 1e-5, 3.0)):
            a, b = x.clone(), x.clone()
            mean_a, std_a = m.cmvn(a.data_ptr(), rows, frames, mode, ddof, valid, eps, pad)
            mean_b = torch.full((rows, n_out), float("nan"), device=DEV)
            std_b = torch.full((rows, n_out), float("nan"), device=DEV)
            assert c.cmvn_ptr(b.data_ptr(), rows, frames, mode, ddof, valid, eps, pad, mean_b, std_b) == 0
            assert same_bits(a, b) and same_bits(mean_a, mean_b) and same_bits(std_a, std_b), (mode, ddof)
        # the same refusals: the descriptor's rules do not know which plan carries the bin count
        assert c.cmvn_ptr(x.data_ptr(), rows, 0, MEAN, 0) == 14 and c.cmvn_ptr(0, rows, frames, MEAN, 0) == 14
        assert c.cmvn_ptr(x.data_ptr(), rows, frames, 2, 0) == 14 and c.cmvn_ptr(x.data_ptr(), 0, frames, MEAN, 0) == 0


@pytest.fixture(scope="module")
def golden(gpu_ready):
    """The golden streams at 16 kHz mono on the device, and the float64 log-mel references of
    Kaldi's 23-bin and 80-bin fbank over them: {bins: (want, tol) [rows, bins, frames]}."""
    datas = [open(os.path.join(GOLDEN, n), "rb").read() for n in STREAMS]
    x, lengths, infos = tensor.decode_to_tensor(datas, sample_rate=16000, mix="mono")
    assert all(i[0] == "OK" for i in infos)
    xs = x[:, 0].cpu().numpy()
    out = {}
    for bins in (23, 80):
        with tensor.MelSpectrogram.kaldi_fbank(num_mel_bins=bins) as mel:
            frames = max(mel.mel_frames(int(x.shape[-1])), 1)
            v, e_v = R.features(xs, lengths.tolist(), mel.window, mel.filters, 512, 160, 0, R.SNIP, R.PAD_ZEROS,
                                float(np.float32(0.97)), True, 32768.0, 0, frames)
            out[bins] = R.scaled(v, e_v, ref.LN, 2.0 ** -23)
    return datas, x, lengths, out


def project_step(T, want, tol, dtype):
    c, mag = C.project(T, want)
    e = np.einsum("km,rmf->rkf", np.abs(T).astype(np.float64), tol)
    n = T.shape[1]
    return c, e + 1.01 * (n + 1) * U * (mag + e) + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0) * (np.abs(c) + e)


def cmvn_step(want, tol, valid, eps, pad):
    """mean_var, ddof 0 -> (out, tol) as the module's head derives."""
    out, e_out = np.full_like(want, pad), np.zeros_like(tol)
    unbounded = []
    for i, F in enumerate(valid):
        if F == 0:
            continue
        l, e = want[i, :, :F], tol[i, :, :F]
        mu = l.mean(axis=1, keepdims=True)
        d = l - mu
        sigma = np.sqrt((d * d).mean(axis=1, keepdims=True))
        a = e + e.mean(axis=1, keepdims=True)
        b = np.sqrt((a * a).mean(axis=1, keepdims=True))
        # A bin whose spread is within the error bound of its own log-mels has no bound here: where a
        # stream has no energy (the bins above a low-rate stream's band) the power is at the floor,
        # fbank_ref's own tolerance of the logarithm is unbounded, and so is any normalisation of it.
        # Such a (row, bin) gets an unbounded tolerance (1e300: finite, so the taps' zeros stay zeros).
        den = sigma - b + eps
        free = den <= 0
        unbounded.append(int(free.sum()))
        r, r2 = 1.0 / (sigma + eps), 1.0 / np.where(free, 1.0, den)
        o = d * r
        out[i, :, :F] = o
        own = 2.0 ** -22 * np.abs(o) + 2.0 ** -23 * (np.abs(l) + e + np.abs(mu) + e.mean(axis=1, keepdims=True)) * r2
        e_out[i, :, :F] = np.where(free, 1e300, np.minimum(a * r2 + np.abs(d) * r * b * r2 + 1.01 * own, 1e300))
    # nearly every (row, bin) is held to a bound
    assert sum(unbounded) <= 0.1 * sum(1 for F in valid if F) * want.shape[1], unbounded
    return out, e_out


def delta_step(want, tol, order, W, valid, pad):
    out, mag = C.deltas(want, order, W, valid, pad)
    ones = {o: np.abs(C.delta_scales(o, W)) for o in range(1, order + 1)}
    e = C.deltas(tol, order, W, valid, 0.0, scales=ones)[0]  # |s_o| over the clamped frames; block 0: tol itself
    Cn = want.shape[1]
    for o in range(1, order + 1):
        blk = slice(o * Cn, (o + 1) * Cn)
        # the taps' own f32 rounding (2^-24 each) rides on the sum's bound
        e[:, blk] += 1.01 * (2 * o * W + 3) * U * (mag[:, blk] + e[:, blk])
    return out, e


def check(got, want, tol, what):
    got = got.double().cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    bad = err > tol
    worst = float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
    print(f"{what}: worst error / bound = {worst:.4f}")
    assert not bad.any(), (what, worst, int(bad.sum()))
    assert (err[tol == 0] == 0).all(), what


def test_kaldi_mfcc_through_decode_to_features(golden):
    datas, x, lengths, refs = golden
    want_l, tol_l = refs[23]
    with tensor.MelSpectrogram.kaldi_mfcc() as mel:
        assert (mel.n_bins, mel.n_base, mel.n_features, mel.layout) == (23, 13, 13, "frames_first")
        assert np.array_equal(mel.dct, tensor.dct_matrix(13, 23, lifter=22.0))
        f, fl, infos = tensor.decode_to_features(datas, mel)
        assert f.shape == (len(datas), 1, want_l.shape[2], 13) and f.dtype == torch.float32
        assert fl.tolist() == [(n - 400) // 160 + 1 if n >= 400 else 0 for n in lengths.tolist()] and int(fl.max()) > 9
        want, tol = project_step(mel.dct, want_l, tol_l, torch.float32)
        check(f[:, 0].transpose(1, 2), want, tol, "kaldi_mfcc() end to end")


def test_kaldi_fbank_with_cmvn_and_deltas_through_decode_to_features(golden):
    datas, x, lengths, refs = golden
    want_l, tol_l = refs[80]
    with tensor.MelSpectrogram.kaldi_fbank(deltas=(2, 2), cmvn="mean_var", cmvn_pad=-1.0) as mel:
        assert (mel.n_bins, mel.n_base, mel.n_features) == (80, 80, 240) and mel.dct is None
        f, fl, infos = tensor.decode_to_features(datas, mel)
        assert f.shape == (len(datas), 1, want_l.shape[2], 240)
        valid = fl.tolist()
        base, e_base = cmvn_step(want_l, tol_l, valid, float(np.float32(1e-5)), -1.0)
        want, tol = delta_step(base, e_base, 2, 2, valid, -1.0)
        check(f[:, 0].transpose(1, 2), want, tol, "kaldi_fbank(deltas, cmvn) end to end")
        for i, F in enumerate(valid):
            assert bool((f[i, 0, F:] == -1.0).all())
        assert mel.last_mean.shape == (len(datas), 1, 80)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", ["bins_first", "frames_first"])
def test_a_call_is_the_explicit_sequence_of_abi_calls(golden, layout, dtype):
    datas, x, lengths, refs = golden
    kw = dict(sample_rate=16000, n_fft=512, hop=160, window="povey", scale="ln", floor=2.0 ** -23, center=False, layout=layout,
              win_length=400, framing="snip", remove_dc=True, preemphasis=0.97, sample_scale=32768.0,
              filters=tensor.kaldi_mel_filters(16000, 512, 23))
    lay = 0 if layout == "bins_first" else 1
    dt = tensor._DTYPES[dtype]
    with tensor.MelSpectrogram(dtype=dtype, mfcc=13, lifter=22.0, cmvn="mean_var", cmvn_ddof=1, cmvn_pad=0.5, deltas=(2, 2), **kw) as mel, \
            tensor.MelSpectrogram(dtype=torch.float32, **kw) as plain, \
            Cepstra(23, 13, lay, F32, dt, tensor.dct_matrix(13, 23, lifter=22.0), 2, 2) as c:
        got, fl = mel(x, lengths)
        bins, fl2 = plain(x, lengths)
        torch.cuda.synchronize()
        assert torch.equal(fl, fl2) and mel.n_features == 39
        rows = bins.shape[0] * bins.shape[1]
        frames = bins.shape[-1] if lay == 0 else bins.shape[-2]
        assert got.shape == bins.shape[:2] + ((39, frames) if lay == 0 else (frames, 39)) and got.dtype == dtype
        ceps = c.project(bins.view((rows,) + bins.shape[2:]))
        mean = torch.empty(rows, 13, device=DEV)
        std = torch.empty(rows, 13, device=DEV)
        assert c.cmvn_ptr(ceps.data_ptr(), rows, frames, MEAN_VAR, 1, fl.tolist(), 1e-5, 0.5, mean, std) == 0
        want = c.deltas(ceps, fl.tolist(), 0.5)
        assert same_bits(got.view(want.shape), want)
        assert same_bits(mel.last_mean.view(mean.shape), mean) and same_bits(mel.last_std.view(std.shape), std)
        # out=: the right tensor is filled, a wrong one refused
        out = torch.empty_like(got)
        again, _ = mel(x, lengths, out=out)
        torch.cuda.synchronize()
        assert again is out and same_bits(out, got)
        with pytest.raises(ValueError):
            mel(x, lengths, out=torch.empty_like(bins.to(dtype)))


def test_a_plan_without_the_new_arguments_is_unchanged(golden):
    """mfcc=None, deltas=None: no cepstra plan, and the bits of the mel run followed by zflac_hip_mel_cmvn."""
    datas, x, lengths, refs = golden
    with tensor.MelSpectrogram.kaldi_fbank(cmvn="mean", dtype=torch.float16) as mel, \
            tensor.MelSpectrogram.kaldi_fbank(dtype=torch.float16) as plain, MelCarrier(80, 1, F16) as carrier:
        assert mel._c is None and plain._c is None and mel.n_features == mel.n_bins == 80 and mel.deltas is None
        got, fl = mel(x, lengths)
        want, _ = plain(x, lengths)
        torch.cuda.synchronize()
        rows, frames = want.shape[0] * want.shape[1], want.shape[2]
        carrier.cmvn(want.data_ptr(), rows, frames, MEAN, 0, fl.tolist(), 1e-5, 0.0)
        torch.cuda.synchronize()
        assert same_bits(got, want)


def test_deltas_alone_keep_the_dtype_of_the_mel_plan(golden):
    """Without a projection the mel plan writes `dtype` itself and the deltas extend that tensor."""
    datas, x, lengths, refs = golden
    with tensor.MelSpectrogram.kaldi_fbank(num_mel_bins=23, dtype=torch.bfloat16, deltas=(1, 2), cmvn_pad=7.0) as mel, \
            tensor.MelSpectrogram.kaldi_fbank(num_mel_bins=23, dtype=torch.bfloat16) as plain, \
            Cepstra(23, 23, 1, BF16, BF16, None, 1, 2) as c:
        got, fl = mel(x, lengths)
        bins, _ = plain(x, lengths)
        torch.cuda.synchronize()
        want = c.deltas(bins.view((-1,) + bins.shape[2:]), fl.tolist(), 7.0)
        assert mel.n_features == 46 and got.dtype == torch.bfloat16 and same_bits(got.view(want.shape), want)
