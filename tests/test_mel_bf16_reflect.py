"""GPU tests of the split-bf16 feature plans through zflac_hip_mel_run_ex (k_mel_split with lengths,
reflect padding and the row maximum; k_mel_norm behind it): parity of reflect padding and per-row
lengths with the kept-term reference within tests/test_mel_bf16.py's bound; bit for bit against a
zeros run of an uncentred plan of the same math over host-reflected rows, and interior frames
across the pad modes; the row maximum; the normalising pass; the Whisper preset against the
torch.stft composition; decode_to_features with a split plan."""
import functools

import torch  # before zflac_amd loads its library: one HIP runtime per process (zflac_amd/tensor.py)

import numpy as np
import pytest

import synth
from zflac_amd import _lib, tensor

from . import malformed
from . import mel_bf16_ref as bref
from . import mel_ref as ref
from . import mel_reflect_ref as rr
from .test_mel_bf16 import MATHS, TERMS, SplitPlan
from .test_mel_reflect import (DEV, FLOOR, LAYOUTS, REFLECT, TORCH_DT, ZEROS, check, filters_of, max_rows, normalised, plus_zero,
                               same_bits, strided, window_of)

pytestmark = pytest.mark.gpu


def reflected_features(x, lengths, w, F, hop, first, frames, terms):
    """tests/mel_reflect_ref.py's features for a split plan: the uncentred frames of the reflected rows."""
    N = np.asarray(w).size
    X = ref.frames_of(rr.padded_rows(x, lengths, N, hop, first, frames), N, hop, 0, first, frames)
    return bref.features_of_frames(X, w, F, terms)


@functools.lru_cache(maxsize=None)
def parity_case(N, hop, n_bins, terms):
    """Noise rows of the length batch, 1e30 behind every length, and their reference, once for both layouts."""
    rng = np.random.default_rng(N * 11 + hop)
    T = 40 * hop + 77
    w, F = window_of(N), filters_of(rng, n_bins, N // 2 + 1)
    frames = ref.mel_frames(T, N, hop, 1) + 2  # two past the longest row's count: computed from the reflected row
    assert frames % 32 != 0
    x = rng.uniform(-1.0, 1.0, (7, T)).astype(np.float32)
    lengths = [T, T + 5, N // 2 + 1, N // 2, 1, 0, 17 * hop + 3]
    v, e_v = reflected_features(x, lengths, w, F, hop, 0, frames, terms)
    return dict(T=T, w=w, F=F, frames=frames, x=x, lengths=lengths, v=v, e_v=e_v)


@pytest.mark.parametrize("math", list(MATHS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("N,hop,n_bins", [(400, 160, 80), (16, 3, 5)])
def test_parity(gpu_ready, N, hop, n_bins, layout, math):
    c = parity_case(N, hop, n_bins, TERMS[math])
    T, stride, lengths = c["T"], c["T"] + 3, c["lengths"]
    buf = strided(c["x"], stride, lengths)
    with SplitPlan(MATHS[math], c["w"], c["F"], hop, 1, ref.POWER, LAYOUTS[layout]) as p:
        got = p.run_ex(buf, len(lengths), T, stride, 0, c["frames"], REFLECT, lengths)
    check(got, c["v"], c["e_v"], f"{math} reflect {N, hop, n_bins} {layout} lengths {lengths}")
    assert plus_zero(got[lengths.index(0)])  # +0, every bit
    want, tol = ref.scaled(c["v"], c["e_v"], ref.LOG10, FLOOR)
    with SplitPlan(MATHS[math], c["w"], c["F"], hop, 1, ref.LOG10, LAYOUTS[layout]) as p:
        got = p.run_ex(buf, len(lengths), T, stride, 0, c["frames"], REFLECT, lengths)
    check(got, want, tol, f"{math} reflect log10 {N, hop, n_bins} {layout}")


@pytest.mark.parametrize("math", list(MATHS))
@pytest.mark.parametrize("N,hop,n_bins", [(400, 160, 80), (16, 3, 5)])
def test_bits_of_the_zeros_run_over_reflected_rows(gpu_ready, N, hop, n_bins, math):
    """The reflect run of the length batch == zflac_hip_mel_run of an uncentred plan of the same math over each
    row reflected on the host, every frame; and its interior frames == the centred zeros run."""
    rng = np.random.default_rng(N + hop)
    T = 40 * hop + 77
    lengths = [T, T + 5, N // 2 + 1, N // 2, 1, 0, 17 * hop + 3, 128 * hop // 4 + 1]
    x = rng.uniform(-1.0, 1.0, (len(lengths), T)).astype(np.float32)
    w, F = window_of(N), filters_of(rng, n_bins, N // 2 + 1)
    frames = ref.mel_frames(T, N, hop, 1) + 2
    width = (frames - 1) * hop + N
    with SplitPlan(MATHS[math], w, F, hop, 1) as pc, SplitPlan(MATHS[math], w, F, hop, 0) as pu:
        got = pc.run_ex(strided(x, T + 3, lengths), len(lengths), T, T + 3, 0, frames, REFLECT, lengths)
        for i, n in enumerate(lengths):
            host = rr.padded(x[i], n, N, width).astype(np.float32)[None, :]
            want = pu.run(strided(host, width), 1, width, width, 0, frames)
            assert same_bits(got[i:i + 1], want), (N, hop, i, n)
        cut = x.copy()
        for i, n in enumerate(lengths):
            cut[i, n:] = 0.0
        zeros = pc.run(strided(cut, T), len(lengths), T, T, 0, frames)
        zeros_ex = pc.run_ex(strided(x, T + 3, lengths), len(lengths), T, T + 3, 0, frames, ZEROS, lengths)
        assert same_bits(zeros, zeros_ex)  # the lengths with zero padding: nothing behind a length is signal
        seen = 0
        for i, n in enumerate(lengths):
            ts = [t for t in range(frames) if t * hop - N // 2 >= 0 and t * hop - N // 2 + N <= min(n, T)]  # n_i is clamped
            if ts:
                assert same_bits(got[i][:, ts[0]:ts[-1] + 1], zeros[i][:, ts[0]:ts[-1] + 1]), (N, hop, i, n)
                assert not same_bits(got[i][:, :ts[0]], zeros[i][:, :ts[0]])  # the padding is there
                seen += 1
        assert seen


@pytest.mark.parametrize("math", list(MATHS))
@pytest.mark.parametrize("frames", [1, 128, 129])
def test_row_maximum(gpu_ready, frames, math):
    for N, hop, n_bins in ((400, 160, 80), (16, 3, 5)):
        rng = np.random.default_rng(N + n_bins + frames)
        T = 129 * hop + 77
        x, lengths = max_rows(rng, T)
        w = ref.hann(N)
        F = tensor.mel_filters(16000, N, 80) if n_bins == 80 else filters_of(rng, n_bins, N // 2 + 1)
        buf = strided(x, T, lengths)
        for scale in (ref.LOG10, ref.POWER):
            with SplitPlan(MATHS[math], w, F, hop, 1, scale) as p:
                out, rm = p.run_ex(buf, 4, T, T, 0, frames, REFLECT, lengths, row_max=True)
                plain = p.run_ex(buf, 4, T, T, 0, frames, REFLECT, lengths)
            assert same_bits(out, plain)  # asking for the maxima changes nothing else
            assert same_bits(rm, out.amax(dim=(1, 2))), (scale, rm, out.amax(dim=(1, 2)))
            if scale == ref.LOG10:
                assert torch.unique(out[2].contiguous().view(torch.int32)).numel() == 1
                assert abs(float(rm[2]) - np.log10(FLOOR)) < 1e-5
            else:
                assert plus_zero(rm[2:3]) and float(rm[1]) > 0
            with SplitPlan(MATHS[math], w, F, hop, 1, scale, 1, _lib.EXPORT_BF16) as ph:  # the maximum is taken before the rounding
                oh, rh = ph.run_ex(buf, 4, T, T, 0, frames, REFLECT, lengths, row_max=True)
            assert same_bits(rh, rm) and same_bits(oh, out.to(torch.bfloat16))


@pytest.mark.parametrize("math", list(MATHS))
@pytest.mark.parametrize("dtype", list(TORCH_DT))
def test_normalisation_against_separate_f32_operations(gpu_ready, dtype, math):
    norm = (8.0, 4.0, 0.25)
    for N, hop, n_bins, frames, layout in ((16, 3, 5, 1001, 0), (400, 160, 80, 129, 1)):
        rng = np.random.default_rng(N + frames)
        T = frames * hop + 11
        x, lengths = max_rows(rng, T)
        x[1] *= np.float32(0.01)
        w = ref.hann(N)
        F = tensor.mel_filters(16000, N, 80) if n_bins == 80 else filters_of(rng, n_bins, N // 2 + 1)
        buf = strided(x, T, lengths)
        with SplitPlan(MATHS[math], w, F, hop, 1, ref.LOG10, layout, dtype) as p:
            none, rm = p.run_ex(buf, 4, T, T, 0, frames, REFLECT, lengths, row_max=True)
            got, rm2 = p.run_ex(buf, 4, T, T, 0, frames, REFLECT, lengths, norm=norm)
        assert same_bits(rm, rm2)
        assert same_bits(got, normalised(none, rm, norm)), (N, frames)
        clamped = (none.float() < (rm - norm[0])[:, None, None])
        assert clamped[3].any() and not clamped.all()


def test_whisper_preset(gpu_ready):
    """MelSpectrogram.whisper(math="bf16x6") against the torch.stft composition in float64, within the log bound
    of the kept-term reference times mul plus an f32 ulp of the result."""
    rng = np.random.default_rng(5)
    B, T = 3, 40 * 160 + 77
    xn = rng.uniform(-1.0, 1.0, (B, T)).astype(np.float32)
    xn[1, 3000:] = 0.0  # a shorter utterance, zero-filled as Whisper's rows are
    x = torch.from_numpy(xn).to(DEV)
    frames = T // 160  # Whisper drops the STFT's last frame
    with tensor.MelSpectrogram.whisper(math="bf16x6") as mel:
        assert mel.math == "bf16x6" and (mel.pad, mel.normalize, mel.reflect_at) == ("reflect", (8.0, 4.0, 0.25), "end")
        got, fl = mel(x, torch.tensor([T, 3000, T]), frames=frames)
        torch.cuda.synchronize()
        assert got.shape == (B, 80, frames) and got.dtype == torch.float32
        row_max = mel.last_row_max
        w, F = mel.window, mel.filters
    with tensor.MelSpectrogram.whisper() as f32:
        assert f32.math == "f32"
        other, _ = f32(x, torch.tensor([T, 3000, T]), frames=frames)
        torch.cuda.synchronize()
        assert not same_bits(other, got)
    s = torch.stft(torch.from_numpy(xn).double(), 400, 160, window=torch.from_numpy(w).double(), center=True,
                   pad_mode="reflect", return_complex=True)
    logs = torch.clamp(torch.from_numpy(F).double() @ (s.abs() ** 2)[:, :, :frames], min=1e-10).log10()
    comp = ((torch.maximum(logs, logs.amax(dim=(1, 2), keepdim=True) - 8.0) + 4.0) / 4.0).numpy()
    # the kept-term reference's log tolerance around the full product: the truncation on top of the summation bound
    factor = bref.summation_factor(400, 6) + bref.truncation_factor(6)
    X = ref.frames_of(rr.padded_rows(xn, [T] * B, 400, 160, 0, frames), 400, 160, 0, 0, frames)
    v, e_v = bref.features_of_frames(X, w, F, 6, factor)
    out, tol = ref.scaled(v, e_v, ref.LOG10, 1e-10)
    bound = tol * 0.25 + np.spacing(np.abs(comp).astype(np.float32)).astype(np.float64)
    check(got, comp, bound, "whisper preset, bf16x6, against the torch.stft composition")
    assert np.abs(row_max.cpu().numpy() - out.max(axis=(1, 2))).max() < 1e-4


def test_decode_to_features_with_a_split_plan(gpu_ready):
    """A mixed-rate batch with an error stream: decode_to_features is mel(export(..., sample_rate, mix="mono"))."""
    cfgs = [dict(channels=1, bps=8, order=3, precision=7, block_size=576, n_samples=3 * 576 + 77, sample_rate=8000),
            dict(channels=1, bps=16, order=6, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=22050),
            dict(channels=2, bps=16, stereo_mode=10, order=8, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=44100),
            dict(channels=2, bps=16, stereo_mode=1, order=8, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=48000)]
    datas = [synth.generate(**dict(c, seed=7200 + i)).flac for i, c in enumerate(cfgs)]
    datas.insert(2, malformed.cases()["bad_sync_frame2"][0])
    with tensor.MelSpectrogram(16000, pad="reflect", normalize=(8.0, 4.0, 0.25), math="bf16x3") as mel, \
            tensor.MelSpectrogram(16000, pad="reflect", normalize=(8.0, 4.0, 0.25)) as f32:
        assert mel.math == "bf16x3"
        f, fl, infos = tensor.decode_to_features(datas, mel)
        rmax = mel.last_row_max
        x, lengths, infos2 = tensor.decode_to_tensor(datas, sample_rate=16000, mix="mono")
        assert infos == infos2 and [i[0] for i in infos].count("OK") == 4 and infos[2][0] != "OK"
        assert x.shape[1] == 1 and f.shape[:3] == (5, 1, 80) and rmax.shape == (5, 1)
        g, gl = mel(x, lengths)
        torch.cuda.synchronize()
        assert same_bits(f, g) and torch.equal(fl, gl)
        assert fl.tolist() == [int(n) // 160 + 1 if n else 0 for n in lengths.tolist()]
        assert fl[2] == 0 and torch.unique(f[2].contiguous().view(torch.int32)).numel() == 1
        assert abs(float(rmax[2, 0]) - np.log10(1e-10)) < 1e-5 and abs(float(f[2].flatten()[0]) - (np.log10(1e-10) + 4) / 4) < 1e-5
        assert torch.unique(f[0].contiguous().view(torch.int32)).numel() > 100
        h, _ = f32(x, lengths)
        torch.cuda.synchronize()
        assert not same_bits(h, g)  # another arithmetic
