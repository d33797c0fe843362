"""GPU tests of framed plans (zflac_hip_mel_create_framed; k_mel, k_mel_ex and k_mel_split over a
frame shorter than the DFT, the three framings, the folded frame operator, ZFLAC_PAD_MIRROR):
parity of every element with the float64 reference of tests/fbank_ref.py within its derived bound;
bit for bit against the plans that existed before (the identity plan, a mirror run against a zeros
run over the host-mirrored row, interior frames across pad modes, slices, row counts,
misalignments); per-row lengths with junk behind them; a short window against torch.stft; and
MelSpectrogram.kaldi_fbank() through decode_to_features."""
import ctypes
import functools

import torch  # before zflac_amd loads its library: one HIP runtime per process (zflac_amd/tensor.py)

import numpy as np
import pytest

import synth
from zflac_amd import _lib, errors, tensor

from . import fbank_ref as R
from . import malformed
from . import mel_ref as ref
from .test_mel_reflect import DEV, JUNK, TORCH_DT, check, filters_of, plus_zero, same_bits, strided

pytestmark = pytest.mark.gpu

F32, X6, X3 = _lib.MEL_MATH_F32, _lib.MEL_MATH_BF16X6, _lib.MEL_MATH_BF16X3
TERMS = {F32: None, X6: 6, X3: 3}
STFT, SNIP, KALDI = R.STFT, R.SNIP, R.KALDI_CENTER
ZEROS, REFLECT, MIRROR = R.PAD_ZEROS, R.PAD_REFLECT, R.PAD_MIRROR
FLOOR = 2.0 ** -23
# N, Nw, hop, bins (the issue's table); the largest shape runs one row
SHAPES = [(2, 1, 1, 2), (16, 11, 3, 5), (32, 30, 7, 33), (512, 400, 160, 80), (2048, 1201, 1201, 256)]


class Plan:
    """zflac_hip_mel_create_framed (or _create_ex with framed=False) / _run / _run_ex through ctypes, on torch tensors."""

    def __init__(self, window, filters, N, hop, center=0, framing=SNIP, dc=0, a=0.0, g=1.0, math=F32, scale=ref.POWER, layout=0,
                 dtype=_lib.EXPORT_F32, floor=None, framed=True):
        tensor.check_single_runtime()
        self.L = _lib.load()
        self.w = np.ascontiguousarray(window, dtype=np.float32)
        self.f = np.ascontiguousarray(filters, dtype=np.float32)
        self.N, self.Nw, self.hop, self.center, self.framing = N, self.w.size, hop, center, framing
        self.dc, self.a, self.g, self.math, self.scale, self.layout, self.dtype = dc, a, g, math, scale, layout, dtype
        self.n_bins = self.f.shape[0]
        self.floor = (0.0 if scale == ref.POWER else FLOOR) if floor is None else floor
        d = _lib.zflac_mel_desc(ctypes.sizeof(_lib.zflac_mel_desc), dtype, layout, scale, center, N, hop, self.n_bins, 0,
                                self.floor, self.w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                self.f.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        self.h = ctypes.c_void_p()
        if framed:
            fd = _lib.zflac_mel_frame_desc(ctypes.sizeof(_lib.zflac_mel_frame_desc), self.Nw, framing, dc, a, g, 0)
            errors.check(self.L.zflac_hip_mel_create_framed(ctypes.byref(d), ctypes.byref(fd), math, 0, ctypes.byref(self.h)),
                         "mel_create_framed")
        else:
            errors.check(self.L.zflac_hip_mel_create_ex(ctypes.byref(d), math, 0, ctypes.byref(self.h)), "mel_create_ex")

    def frames(self, n):
        got = int(self.L.zflac_hip_mel_plan_frames(self.h, int(n)))
        assert got == R.plan_frames(self.framing, int(n), self.N, self.Nw, self.hop, self.center)
        return got

    def shape(self, rows, frames):
        return (rows, self.n_bins, frames) if self.layout == 0 else (rows, frames, self.n_bins)

    def view(self, out):
        return out if self.layout == 0 else out.transpose(1, 2)

    def run(self, buf, rows, wave_frames, row_stride, first, frames, offset=0):
        out = torch.empty(self.shape(rows, frames), dtype=TORCH_DT[self.dtype], device=DEV)
        torch.cuda.synchronize()
        rc = self.L.zflac_hip_mel_run(self.h, buf.data_ptr() + 4 * offset, rows, wave_frames, row_stride, first, frames,
                                      out.data_ptr(), out.numel() * out.element_size(), None)
        errors.check(rc, "mel_run")
        return self.view(out)

    def run_ex(self, buf, rows, wave_frames, row_stride, first, frames, pad=ZEROS, lengths=None, offset=0):
        out = torch.empty(self.shape(rows, frames), dtype=TORCH_DT[self.dtype], device=DEV)
        ln = None if lengths is None else torch.tensor([int(n) for n in lengths], dtype=torch.int64, device=DEV)
        d = _lib.zflac_mel_run_desc(ctypes.sizeof(_lib.zflac_mel_run_desc), pad, _lib.NORM_NONE, 0,
                                    buf.data_ptr() + 4 * offset, rows, wave_frames, row_stride,
                                    None if ln is None else ln.data_ptr(), first, frames, out.data_ptr(),
                                    out.numel() * out.element_size(), None, 0.0, 0.0, 0.0, 0)
        torch.cuda.synchronize()
        errors.check(self.L.zflac_hip_mel_run_ex(self.h, ctypes.byref(d), None), "mel_run_ex")
        return self.view(out)

    def reference(self, x, lengths, pad, first, frames):
        """-> (out, tol) float64 [rows, n_bins, frames] of tests/fbank_ref.py for this plan."""
        v, e_v = R.features(x, lengths, self.w, self.f, self.N, self.hop, self.center, self.framing, pad,
                            float(np.float32(self.a)), bool(self.dc), float(np.float32(self.g)), first, frames, TERMS[self.math])
        return R.scaled(v, e_v, self.scale, self.floor)

    def close(self):
        if self.h:
            self.L.zflac_hip_mel_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def window_of(Nw):
    return tensor.kaldi_window("povey", Nw) if Nw > 2 else np.array([0.75, 1.0], np.float32)[:Nw]


@functools.lru_cache(maxsize=None)
def signals(N, Nw, hop):
    """float32 [rows, T]: noise, a 0.9 DC with a 2^-10 ripple, impulses, a zero row; T long enough for 129+ frames
    (two workgroup tiles) under every framing. The largest shape has the noise row alone."""
    rng = np.random.default_rng(1000 * N + Nw)
    T = 130 * hop + Nw + 3
    t = np.arange(T)
    x = np.zeros((4, T), dtype=np.float32)
    x[0] = rng.uniform(-1.0, 1.0, T)
    x[1] = 0.9 + 2.0 ** -10 * np.sin(0.7 * t)
    x[2, ::max(Nw - 1, 1) * 3 + 1] = 0.75
    x[2, 5::97] = -0.5
    if N == 2048:
        x = x[:1]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def filters(N, bins):
    return filters_of(np.random.default_rng(N + bins), bins, N // 2 + 1)


# framing, center, pad, dc, a, g, layout, scale
COMBOS = [(SNIP, 0, ZEROS, 1, 0.97, 32768.0, 1, ref.LN),
          (KALDI, 0, MIRROR, 1, 0.97, 32768.0, 0, ref.LN),
          (STFT, 1, REFLECT, 0, 0.0, 1.0, 0, ref.LOG10),
          (STFT, 0, ZEROS, 0, 0.97, 1.0, 1, ref.POWER),
          (KALDI, 0, ZEROS, 1, 0.0, 1.0, 0, ref.POWER)]


@pytest.mark.parametrize("math", [F32, X6, X3], ids=["f32", "bf16x6", "bf16x3"])
@pytest.mark.parametrize("N,Nw,hop,bins", SHAPES)
def test_parity_with_the_float64_reference(gpu_ready, N, Nw, hop, bins, math):
    """Every element within the derived bound; a zero row gives exactly log(floor) (or +0); frames
    at and past the plan's count included (one more is asked for)."""
    x = signals(N, Nw, hop)
    rows, T = x.shape
    buf = strided(x, T + 5)
    for framing, center, pad, dc, a, g, layout, scale in COMBOS:
        with Plan(window_of(Nw), filters(N, bins), N, hop, center, framing, dc, a, g, math, scale, layout) as p:
            frames = p.frames(T) + 1
            assert frames > 129
            got = p.run_ex(buf, rows, T, T + 5, 0, frames, pad)
            want, tol = p.reference(x, None, pad, 0, frames)
            check(got, want, tol, f"N {N} Nw {Nw} math {math} framing {framing} pad {pad} dc {dc} a {a} g {g}")
            if pad == ZEROS:  # zflac_hip_mel_run is the same run
                assert same_bits(p.run(buf, rows, T, T + 5, 0, frames), got)
            if rows == 4:
                z = got[3].contiguous()
                if scale == ref.POWER:
                    assert plus_zero(z)
                else:
                    assert torch.unique(z.view(torch.int32)).numel() == 1
                    lg = np.log10 if scale == ref.LOG10 else np.log
                    assert abs(float(z.flatten()[0]) - lg(FLOOR)) <= 2.0 ** -21 * abs(lg(FLOOR))


@pytest.mark.parametrize("math", [F32, X6, X3], ids=["f32", "bf16x6", "bf16x3"])
@pytest.mark.parametrize("dtype,layout", [(_lib.EXPORT_F32, 0), (_lib.EXPORT_F16, 1), (_lib.EXPORT_BF16, 0)])
def test_identity_plan_is_create_ex_bit_for_bit(gpu_ready, math, dtype, layout):
    for N, hop, bins, center in ((32, 7, 33, 1), (400, 160, 80, 1), (512, 160, 80, 0)):
        x = signals(N, N, hop)
        rows, T = x.shape
        buf = strided(x, T)
        kw = dict(center=center, framing=STFT, math=math, scale=ref.LN, layout=layout, dtype=dtype)
        with Plan(ref.hann(N), filters(N, bins), N, hop, framed=True, **kw) as a, \
                Plan(ref.hann(N), filters(N, bins), N, hop, framed=False, **kw) as b:
            frames = a.frames(T)
            assert same_bits(a.run(buf, rows, T, T, 0, frames), b.run(buf, rows, T, T, 0, frames))
            if center:
                assert same_bits(a.run_ex(buf, rows, T, T, 0, frames, REFLECT), b.run_ex(buf, rows, T, T, 0, frames, REFLECT))


@pytest.mark.parametrize("math", [F32, X6, X3], ids=["f32", "bf16x6", "bf16x3"])
@pytest.mark.parametrize("N,Nw,hop,bins", SHAPES[1:4])
def test_mirror_is_zeros_over_the_host_mirrored_row(gpu_ready, N, Nw, hop, bins, math):
    """A _KALDI_CENTER plan under ZFLAC_PAD_MIRROR equals a _SNIP plan of the same tables under
    zeros over the row mirrored on the host and shifted by Nw / 2 - hop / 2: a wrong rho, an
    off-by-one at either end or a changed order of summation cannot pass."""
    x = signals(N, Nw, hop)[:3]
    rows = x.shape[0]
    off = Nw // 2 - hop // 2
    for n in (Nw + 1, 20 * hop + 1, x.shape[1]):
        kw = dict(dc=1, a=0.97, g=32768.0, math=math, scale=ref.LN)
        with Plan(window_of(Nw), filters(N, bins), N, hop, 0, KALDI, **kw) as k, \
                Plan(window_of(Nw), filters(N, bins), N, hop, 0, SNIP, **kw) as s:
            frames = k.frames(n) + 2
            span = (frames - 1) * hop + Nw
            y = np.stack([R.padded(x[i], n, np.arange(span) - off, MIRROR, N) for i in range(rows)]).astype(np.float32)
            got = k.run_ex(strided(x[:, :n], n + 3), rows, n, n + 3, 0, frames, MIRROR)
            assert same_bits(got, s.run(strided(y, span), rows, span, span, 0, frames)), n


@pytest.mark.parametrize("math", [F32, X6, X3], ids=["f32", "bf16x6", "bf16x3"])
def test_interior_frames_have_the_same_bits_in_every_pad_mode(gpu_ready, math):
    N, Nw, hop, bins = 512, 400, 160, 80
    x = signals(N, Nw, hop)
    rows, T = x.shape
    buf = strided(x, T)
    for framing, center, pad in ((KALDI, 0, MIRROR), (STFT, 1, REFLECT)):
        with Plan(window_of(Nw), filters(N, bins), N, hop, center, framing, 1, 0.97, 32768.0, math, ref.LN) as p:
            frames = p.frames(T)
            a, b = p.run_ex(buf, rows, T, T, 0, frames, ZEROS), p.run_ex(buf, rows, T, T, 0, frames, pad)
            s0 = R.frame_start(framing, np.arange(frames), N, Nw, hop, center)
            inside = torch.from_numpy((s0 >= 0) & (s0 + Nw <= T)).to(DEV)
            assert int(inside.sum()) > 120 and not bool(inside[0]) and not bool(inside[-1])
            assert same_bits(a[:, :, inside], b[:, :, inside])
            assert not same_bits(a[:3, :, ~inside], b[:3, :, ~inside])


@pytest.mark.parametrize("math", [F32, X6, X3], ids=["f32", "bf16x6", "bf16x3"])
@pytest.mark.parametrize("N,Nw,hop,bins", SHAPES[1:4])
def test_slices_rows_and_misalignment_do_not_change_a_frame(gpu_ready, N, Nw, hop, bins, math):
    x = signals(N, Nw, hop)
    rows, T = x.shape
    with Plan(window_of(Nw), filters(N, bins), N, hop, 0, KALDI, 1, 0.97, 32768.0, math, ref.LN, layout=1) as p:
        frames = p.frames(T)
        buf = strided(x, T + 8)
        full = p.run_ex(buf, rows, T, T + 8, 0, frames, MIRROR)
        for first in (1, 31, 32, 33):  # a frame moves through the lanes, waves and tiles
            part = p.run_ex(buf, rows, T, T + 8, first, frames - first, MIRROR)
            assert same_bits(part, full[:, :, first:]), first
        five = np.concatenate([x[:1]] * 5)  # one row against five
        alone = p.run_ex(strided(x[:1], T), 1, T, T, 0, frames, MIRROR)
        many = p.run_ex(strided(five, T + 1), 5, T, T + 1, 0, frames, MIRROR)
        assert same_bits(alone, full[:1]) and all(same_bits(many[i:i + 1], alone) for i in range(5))
        flat = torch.from_numpy(np.array(x).reshape(-1)).to(DEV)
        for shift in (1, 2, 3):  # wave_device 4, 8 and 12 bytes off a 16-byte boundary
            moved = torch.full((flat.numel() + 4,), JUNK, device=DEV)
            moved[shift:shift + flat.numel()] = flat
            assert same_bits(p.run_ex(moved, rows, T, T, 0, frames, MIRROR, offset=shift), full), shift


@pytest.mark.parametrize("math", [F32, X6, X3], ids=["f32", "bf16x6", "bf16x3"])
@pytest.mark.parametrize("N,Nw,hop,bins", SHAPES[:4])
def test_lengths_with_junk_behind_them(gpu_ready, N, Nw, hop, bins, math):
    """Rows of every length at which a framing or a reflection changes, 1e30 behind each: nothing
    past n_i may show, under every framing and pad mode."""
    lengths = sorted({0, 1, 2, max(Nw // 2 - 1, 0), Nw // 2, Nw - 1, Nw, Nw + 1, 20 * hop - 1, 20 * hop + 1})
    rng = np.random.default_rng(N)
    T = 20 * hop + 1
    x = rng.uniform(-1.0, 1.0, (len(lengths), T)).astype(np.float32)
    buf = strided(x, T + 3, lengths)
    for framing, center, pad in ((SNIP, 0, ZEROS), (KALDI, 0, MIRROR), (KALDI, 0, ZEROS), (STFT, 1, REFLECT), (STFT, 0, ZEROS)):
        with Plan(window_of(Nw), filters(N, bins), N, hop, center, framing, 1, 0.97, 32768.0, math, ref.LN) as p:
            frames = max(p.frames(T), 1) + 1
            got = p.run_ex(buf, len(lengths), T + 3, T + 3, 0, frames, pad, lengths)
            want, tol = p.reference(x, lengths, pad, 0, frames)
            check(got, want, tol, f"lengths: N {N} Nw {Nw} math {math} framing {framing} pad {pad}")
            assert torch.unique(got[0].contiguous().view(torch.int32)).numel() == 1  # n_i = 0: log(floor) everywhere


@pytest.mark.parametrize("math", [F32, X6], ids=["f32", "bf16x6"])
def test_short_window_against_torch_stft(gpu_ready, math):
    """An _STFT plan with Nw < N, center = 1 and reflect padding is torch.stft(n_fft=N,
    win_length=Nw) in float64: the reference here is composed from torch.stft, not fbank_ref."""
    N, Nw, hop, bins = 512, 400, 160, 80
    x = signals(N, Nw, hop)[:3]
    rows, T = x.shape
    w, F = window_of(Nw), filters(N, bins)
    with Plan(w, F, N, hop, 1, STFT, math=math, scale=ref.LOG10, floor=1e-10) as p:
        frames = p.frames(T)
        got = p.run_ex(strided(x, T), rows, T, T, 0, frames, REFLECT)
        S = torch.stft(torch.from_numpy(np.array(x)).double(), N, hop_length=hop, win_length=Nw,
                       window=torch.from_numpy(w).double(), center=True, pad_mode="reflect", return_complex=True)
        assert S.shape == (rows, N // 2 + 1, frames)
        comp = np.log10(np.maximum(np.einsum("mk,rkt->rmt", F.astype(np.float64), (S.abs() ** 2).numpy()), 1e-10))
        want, tol = p.reference(x, None, REFLECT, 0, frames)
        assert np.abs(comp - want).max() < 1e-9  # the two float64 references agree
        check(got, comp, tol, f"short window against torch.stft, math {math}")


def test_kaldi_fbank_through_decode_to_features(gpu_ready):
    """A mixed-rate batch with an error stream through MelSpectrogram.kaldi_fbank(): the features are
    mel(export(..., 16000, mix="mono")), Kaldi's frame count, and the float64 pipeline's values."""
    cfgs = [dict(channels=1, bps=8, order=3, precision=7, block_size=576, n_samples=3 * 576 + 77, sample_rate=8000),
            dict(channels=1, bps=16, order=6, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=22050),
            dict(channels=2, bps=16, stereo_mode=10, order=8, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=44100),
            dict(channels=2, bps=16, stereo_mode=1, order=8, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=48000)]
    datas = [synth.generate(**dict(c, seed=7300 + i)).flac for i, c in enumerate(cfgs)]
    datas.insert(2, malformed.cases()["bad_sync_frame2"][0])
    for snip in (True, False):
        with tensor.MelSpectrogram.kaldi_fbank(snip_edges=snip) as mel:
            assert (mel.n_fft, mel.win_length, mel.hop, mel.n_bins, mel.math) == (512, 400, 160, 80, "f32")
            f, fl, infos = tensor.decode_to_features(datas, mel)
            x, lengths, infos2 = tensor.decode_to_tensor(datas, sample_rate=16000, mix="mono")
            assert infos == infos2 and [i[0] for i in infos].count("OK") == 4 and infos[2][0] != "OK"
            assert f.shape[:2] == (5, 1) and f.shape[3] == 80 and f.dtype == torch.float32
            g, gl = mel(x, lengths)
            torch.cuda.synchronize()
            assert same_bits(f, g) and torch.equal(fl, gl)
            want_fl = [((n - 400) // 160 + 1 if n >= 400 else 0) if snip else (n + 80) // 160 for n in lengths.tolist()]
            assert fl.tolist() == want_fl and fl[2] == 0
            assert torch.unique(f[2].contiguous().view(torch.int32)).numel() == 1
            assert abs(float(f[2].flatten()[0]) - np.log(2.0 ** -23)) < 1e-5
            xs = x[:, 0].cpu().numpy()
            v, e_v = R.features(xs, lengths.tolist(), mel.window, mel.filters, 512, 160, 0, SNIP if snip else KALDI,
                                ZEROS if snip else MIRROR, float(np.float32(0.97)), True, 32768.0, 0, f.shape[2])
            want, tol = R.scaled(v, e_v, ref.LN, 2.0 ** -23)
            check(f[:, 0].transpose(1, 2), want, tol, f"kaldi_fbank(snip_edges={snip}) end to end")
