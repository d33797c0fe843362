"""GPU tests of the log-mel features (zflac_hip_mel_*, k_mel; zflac_amd.tensor.MelSpectrogram):
parity with the float64 reference of tests/mel_ref.py within its elementwise bound, the DFT alone,
independence of a frame's bits from everything but its samples, the half dtypes, coverage and
bounds of the destination, streams and plan lifetime, and the Python layer."""
import ctypes

import torch  # before zflac_amd loads its library: one HIP runtime per process (zflac_amd/tensor.py)

import numpy as np
import pytest

import synth
from zflac_amd import _lib, errors, tensor

from . import malformed
from . import mel_ref as ref

pytestmark = pytest.mark.gpu

CONFIGS = [(400, 160, 80, 1), (16, 3, 5, 0), (30, 7, 33, 1), (1024, 256, 128, 1), (2048, 2048, 256, 0), (2, 1, 2, 1)]
LAYOUTS = {"bins_first": _lib.MEL_BINS_FIRST, "frames_first": _lib.MEL_FRAMES_FIRST}
TORCH_DT = {_lib.EXPORT_F32: torch.float32, _lib.EXPORT_F16: torch.float16, _lib.EXPORT_BF16: torch.bfloat16}
FLOOR = 1e-10
ROWS = 5
DEV = torch.device("cuda", 0)


class Plan:
    """zflac_hip_mel_create / _run / _destroy through ctypes, on torch tensors."""

    def __init__(self, window, filters, hop, center, scale=ref.POWER, layout=0, dtype=_lib.EXPORT_F32, floor=None):
        tensor.check_single_runtime()
        self.L = _lib.load()
        self.w = np.ascontiguousarray(window, dtype=np.float32)
        self.f = np.ascontiguousarray(filters, dtype=np.float32)
        self.N, self.hop, self.center, self.scale, self.layout, self.dtype = self.w.size, hop, center, scale, layout, dtype
        self.n_bins = self.f.shape[0]
        self.floor = (0.0 if scale == ref.POWER else FLOOR) if floor is None else floor
        d = _lib.zflac_mel_desc(ctypes.sizeof(_lib.zflac_mel_desc), dtype, layout, scale, center, self.N, hop, self.n_bins,
                                0, self.floor, self.w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                self.f.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        self.h = ctypes.c_void_p()
        errors.check(self.L.zflac_hip_mel_create(ctypes.byref(d), 0, ctypes.byref(self.h)), "mel_create")

    def shape(self, rows, frames):
        return (rows, self.n_bins, frames) if self.layout == 0 else (rows, frames, self.n_bins)

    def run_raw(self, wave_ptr, rows, wave_frames, row_stride, first, frames, dst_ptr, dst_bytes, stream=None):
        return self.L.zflac_hip_mel_run(self.h, wave_ptr, rows, wave_frames, row_stride, first, frames, dst_ptr, dst_bytes,
                                        stream)

    def run(self, buf, rows, wave_frames, row_stride, first, frames, offset=0, stream=None):
        """buf: a flat float32 cuda tensor holding the rows from element `offset` on -> [rows, bins, frames]."""
        out = torch.empty(self.shape(rows, frames), dtype=TORCH_DT[self.dtype], device=DEV)
        torch.cuda.synchronize()
        rc = self.run_raw(buf.data_ptr() + 4 * offset, rows, wave_frames, row_stride, first, frames, out.data_ptr(),
                          out.numel() * out.element_size(), stream)
        errors.check(rc, "mel_run")
        return out if self.layout == 0 else out.transpose(1, 2)

    def close(self):
        if self.h:
            self.L.zflac_hip_mel_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def filters_of(rng, n_bins, K):
    """Non-negative, sparse-ish rows like a mel bank's, with some zeros."""
    f = rng.uniform(0.0, 1.0, (n_bins, K)).astype(np.float32)
    f[rng.uniform(size=f.shape) < 0.5] = 0.0
    return f


def signals(rng, N, hop, T):
    """name -> float32 [T]"""
    t = np.arange(T, dtype=np.float64)
    imp = lambda at: np.where(t == at, 1.0, 0.0)  # noqa: E731
    return {
        "noise": rng.uniform(-1.0, 1.0, T),
        "tone16": np.round(0.8 * np.sin(2.0 * np.pi * 0.0731 * t) * 32767.0) / 32768.0,
        "dc": np.ones(T),
        "alternation": np.where(t % 2 == 0, 1.0, -1.0),
        "impulse_first": imp(0),
        "impulse_last": imp(T - 1),
        "impulse_tile_edge": imp(32 * hop - 1),
        "zero": np.zeros(T),
        "noise2": rng.uniform(-1.0, 1.0, T),
        "tone16b": np.round(0.5 * np.cos(2.0 * np.pi * 0.25 * t) * 32767.0) / 32768.0,
    }


def strided(x, stride):
    """x: float32 [rows, T] -> a flat cuda tensor with rows `stride` apart, junk between them."""
    rows, T = x.shape
    h = np.full((rows, stride), 1e30, dtype=np.float32)  # what lies past wave_frames must never be read as signal
    h[:, :T] = x
    return torch.from_numpy(h.reshape(-1)).to(DEV)


def check(got, want, tol, what):
    """|got - want| <= tol everywhere; prints the worst error-to-bound ratio."""
    got = got.detach().cpu().double().numpy()
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    exact = tol == 0
    assert (err[exact] == 0).all(), what
    ratio = float((err[~exact] / tol[~exact]).max()) if (~exact).any() else 0.0
    print(f"{what}: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0, what


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("N,hop,n_bins,center", CONFIGS)
def test_parity(gpu_ready, N, hop, n_bins, center, layout):
    rng = np.random.default_rng(N * 7 + hop)
    T = 40 * hop + 77
    stride = T + 3
    w = ref.hann(N) if N > 2 else np.array([0.75, 1.0], np.float32)
    F = filters_of(rng, n_bins, N // 2 + 1)
    sig = signals(rng, N, hop, T)
    frames = ref.mel_frames(T, N, hop, center) + 2  # two past the count: computed from the zero-extended row
    assert frames % 32 != 0
    groups = [["noise", "tone16", "dc", "alternation", "impulse_first"],
              ["impulse_last", "impulse_tile_edge", "zero", "noise2", "tone16b"]]
    with Plan(w, F, hop, center, ref.POWER, LAYOUTS[layout]) as p:
        for names in groups:
            x = np.stack([sig[n] for n in names]).astype(np.float32)
            v, e_v = ref.features(x, w, F, hop, center, 0, frames)
            got = p.run(strided(x, stride), ROWS, T, stride, 0, frames)
            check(got, v, e_v, f"power {N, hop, n_bins, center} {layout} {names}")
            zero = names.index("zero") if "zero" in names else None
            if zero is not None:
                assert not got[zero].view(torch.int32).any()  # +0, every bit
    x = rng.uniform(-1.0, 1.0, (ROWS, T)).astype(np.float32)
    v, e_v = ref.features(x, w, F, hop, center, 0, frames)
    for scale in (ref.LOG10, ref.LN):
        want, tol = ref.scaled(v, e_v, scale, FLOOR)
        assert (tol <= 0.01).all()  # noise: no bin cancels, every element is compared
        with Plan(w, F, hop, center, scale, LAYOUTS[layout]) as p:
            got = p.run(strided(x, stride), ROWS, T, stride, 0, frames)
        check(got, want, tol, f"log scale {scale} {N, hop, n_bins, center} {layout}")


@pytest.mark.parametrize("N", [16, 400])
def test_dft_alone(gpu_ready, N):
    """Identity filters, a rectangular window and a cosine on bin k0: P[k0] = (N / 2)^2, its neighbours 0."""
    K, hop, k0 = N // 2 + 1, N // 4, 3
    T = 12 * hop + N
    x = np.cos(2.0 * np.pi * k0 * np.arange(T) / N).astype(np.float32)[None, :]
    w, F = np.ones(N, np.float32), np.eye(K, dtype=np.float32)
    frames = ref.mel_frames(T, N, hop, 0)
    v, e_v = ref.features(x, w, F, hop, 0, 0, frames)
    with Plan(w, F, hop, 0) as p:
        got = p.run(strided(x, T), 1, T, T, 0, frames)
    check(got, v, e_v, f"dft alone N={N}")
    g = got.cpu().numpy()[0]
    assert np.allclose(g[k0], (N / 2.0) ** 2, rtol=1e-4)
    assert (np.abs(g[[k0 - 1, k0 + 1]]) <= e_v[0][[k0 - 1, k0 + 1]]).all() and (e_v[0][[k0 - 1, k0 + 1]] < 1e-3 * N).all()
    assert (g.argmax(axis=0) == k0).all()  # an asymmetric answer: bins on the rows, frames on the columns


@pytest.fixture(scope="module")
def whisper(gpu_ready):
    rng = np.random.default_rng(99)
    N, hop, T = 400, 160, 40 * 160 + 77
    x = rng.uniform(-1.0, 1.0, (ROWS, T)).astype(np.float32)
    x[3] = 0.0
    w, F = ref.hann(N), tensor.mel_filters(16000, N, 80)
    frames = ref.mel_frames(T, N, hop, 1) + 2
    p = Plan(w, F, hop, 1, ref.LOG10)
    full = p.run(strided(x, T + 3), ROWS, T, T + 3, 0, frames)
    yield dict(p=p, x=x, T=T, frames=frames, full=full, w=w, F=F)
    p.close()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("first", [1, 31, 32, 33])
def test_independence_of_first_frame(whisper, first):
    m = whisper
    n = 7
    got = m["p"].run(strided(m["x"], m["T"] + 3), ROWS, m["T"], m["T"] + 3, first, n)
    assert same_bits(got, m["full"][:, :, first:first + n])


def test_independence_of_rows_and_alignment(whisper):
    m = whisper
    T = m["T"]
    one = m["p"].run(strided(m["x"][1:2], T), 1, T, T, 0, m["frames"])
    assert same_bits(one[0], m["full"][1])
    for shift in (1, 2, 3):  # wave_device 4, 8, 12 bytes past a 16-byte boundary
        buf = torch.cat([torch.full((shift,), 1e30, device=DEV), strided(m["x"], T + 3)])
        assert buf.data_ptr() % 16 == 0
        got = m["p"].run(buf, ROWS, T, T + 3, 0, m["frames"], offset=shift)
        assert same_bits(got, m["full"]), shift
    # a row that starts one sample later is the same signal one sample earlier: hop = 1 moves it by a frame
    with Plan(m["w"], m["F"], 1, 0, ref.LOG10) as p1:
        a = p1.run(strided(m["x"][:1], T), 1, T, T, 0, 300)
        b = p1.run(strided(m["x"][:1], T), 1, T - 1, T - 1, 0, 299, offset=1)
        assert same_bits(a[:, :, 1:300], b)


def test_zero_rows_hold_one_bit_pattern(whisper):
    z = whisper["full"][3]
    bits = torch.unique(z.contiguous().view(torch.int32))
    assert bits.numel() == 1
    assert abs(float(z.flatten()[0]) - np.log10(FLOOR)) < 1e-5
    with Plan(whisper["w"], whisper["F"], 160, 1, ref.LN) as p:
        z = p.run(torch.zeros(1000, device=DEV), 1, 1000, 1000, 0, 9)
        assert torch.unique(z.contiguous().view(torch.int32)).numel() == 1
        assert abs(float(z.flatten()[0]) - np.log(FLOOR)) < 1e-5


@pytest.mark.parametrize("dtype", [_lib.EXPORT_F16, _lib.EXPORT_BF16])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_half_dtypes_round_the_f32_result(whisper, dtype, layout):
    m = whisper
    x = m["x"] * np.float32(128.0)  # powers on both sides of 65504, f16's largest
    x[2] *= np.float32(1e-3)
    buf = strided(x, m["T"])
    for scale in (ref.POWER, ref.LOG10):
        with Plan(m["w"], m["F"], 160, 1, scale, LAYOUTS[layout]) as p32, \
                Plan(m["w"], m["F"], 160, 1, scale, LAYOUTS[layout], dtype) as p16:
            a = p32.run(buf, ROWS, m["T"], m["T"], 0, m["frames"])
            b = p16.run(buf, ROWS, m["T"], m["T"], 0, m["frames"])
        if scale == ref.POWER:
            assert float(a.max()) > 65504.0 and float(a[2].max()) < 60000.0
            if dtype == _lib.EXPORT_F16:
                assert torch.isinf(b).any() and not torch.isinf(b[2]).any()
        want = a.to(TORCH_DT[dtype])
        assert b.dtype == want.dtype
        assert torch.equal(b.contiguous().view(torch.int16), want.contiguous().view(torch.int16))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("frames", [129, 128, 1])
def test_coverage_and_bounds(whisper, layout, frames):
    m = whisper
    guard, n = 257, ROWS * 80 * frames
    big = torch.full((n + 2 * guard,), float("nan"), device=DEV)
    buf = strided(m["x"], m["T"])
    with Plan(m["w"], m["F"], 160, 1, ref.POWER, LAYOUTS[layout]) as p:
        torch.cuda.synchronize()
        assert p.run_raw(buf.data_ptr(), ROWS, m["T"], m["T"], 0, frames, big.data_ptr() + 4 * guard, 4 * n) == 0
        assert p.run_raw(buf.data_ptr(), ROWS, m["T"], m["T"], 0, frames, big.data_ptr() + 4 * guard, 4 * n - 1) == 14
    assert torch.isnan(big[:guard]).all() and torch.isnan(big[guard + n:]).all()
    assert not torch.isnan(big[guard:guard + n]).any()


def test_state_and_stream(whisper):
    m = whisper
    buf = strided(m["x"], m["T"] + 3)
    args = (ROWS, m["T"], m["T"] + 3, 0, m["frames"])
    side = torch.cuda.Stream(DEV)
    out = torch.empty(m["p"].shape(ROWS, m["frames"]), device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert m["p"].run_raw(buf.data_ptr(), *args, out.data_ptr(), out.numel() * 4, side.cuda_stream) == 0
        doubled = out * 2  # on the same stream: ordered after the run
    side.synchronize()
    assert same_bits(out, m["full"]) and torch.equal(doubled, m["full"] * 2)
    # two plans at once, each on a stream of its own, and a plan destroyed with its run enqueued
    s2 = torch.cuda.Stream(DEV)
    p2 = Plan(m["w"], m["F"], 160, 1, ref.LN)
    with Plan(m["w"], m["F"], 160, 1, ref.LN) as ln_sync:
        want2 = ln_sync.run(buf, *args)
    o1, o2 = torch.empty_like(out), torch.empty_like(out)
    torch.cuda.synchronize()
    assert m["p"].run_raw(buf.data_ptr(), *args, o1.data_ptr(), o1.numel() * 4, side.cuda_stream) == 0
    assert p2.run_raw(buf.data_ptr(), *args, o2.data_ptr(), o2.numel() * 4, s2.cuda_stream) == 0
    p2.close()  # waits for the device
    assert same_bits(o2, want2)
    side.synchronize()
    assert same_bits(o1, m["full"])
    # arguments a run refuses, with the device there
    assert m["p"].run_raw(buf.data_ptr() + 2, *args, out.data_ptr(), out.numel() * 4) == 14
    assert m["p"].run_raw(buf.data_ptr(), ROWS, m["T"] + 4, m["T"] + 3, 0, m["frames"], out.data_ptr(), out.numel() * 4) == 14
    assert m["p"].run_raw(buf.data_ptr(), 0, m["T"], m["T"] + 3, 0, m["frames"], out.data_ptr(), 0) == 0


def test_python_layer(whisper):
    m = whisper
    T = m["T"]
    x = torch.from_numpy(m["x"]).to(DEV)
    with tensor.MelSpectrogram(16000) as mel:
        assert (mel.n_fft, mel.hop, mel.n_bins) == (400, 160, 80)
        assert np.array_equal(mel.window.view(np.uint32), m["w"].view(np.uint32))
        f, fl = mel(x)
        torch.cuda.synchronize()
        assert f.shape == (ROWS, 80, T // 160 + 1) and fl.tolist() == [T // 160 + 1] * ROWS
        assert same_bits(f, m["full"][:, :, :T // 160 + 1])
        lengths = torch.tensor([T, 0, 1, 159, 160 * 20])
        f2, fl2 = mel(x, lengths, frames=30, first_frame=5)
        assert fl2.tolist() == [30, 0, 0, 0, 16] and fl2.dtype == torch.int64 and fl2.device == DEV
        torch.cuda.synchronize()
        assert same_bits(f2, m["full"][:, :, 5:35])
        x3 = x[:4].reshape(2, 2, T).contiguous()
        f3, fl3 = mel(x3)
        torch.cuda.synchronize()
        assert f3.shape == (2, 2, 80, T // 160 + 1) and fl3.shape == (2,)
        assert same_bits(f3.reshape(4, 80, -1), m["full"][:4, :, :T // 160 + 1])
        out = torch.empty_like(f)
        assert mel(x, out=out)[0] is out
        for bad, exc in ((torch.empty(ROWS, 80, 3, device=DEV), ValueError), (out.half(), TypeError), (out.cpu(), ValueError),
                         (torch.empty(ROWS, T // 160 + 1, 80, device=DEV).transpose(1, 2), ValueError)):
            with pytest.raises(exc):
                mel(x, out=bad)
        with pytest.raises(TypeError):
            mel(x.double())
        with pytest.raises(ValueError):
            mel(x[:, ::2])
    with pytest.raises(ValueError):
        mel(x)  # closed
    with tensor.MelSpectrogram(16000, layout="frames_first", dtype=torch.bfloat16, scale="power") as mel:
        f, _ = mel(x)
        assert f.shape == (ROWS, T // 160 + 1, 80) and f.dtype == torch.bfloat16


def test_decode_to_features(gpu_ready):
    """A mixed-rate batch with an error stream: decode_to_features is mel(export(..., sample_rate, mix="mono"))."""
    cfgs = [dict(channels=1, bps=8, order=3, precision=7, block_size=576, n_samples=3 * 576 + 77, sample_rate=8000),
            dict(channels=1, bps=16, order=6, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=22050),
            dict(channels=2, bps=16, stereo_mode=10, order=8, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=44100),
            dict(channels=2, bps=16, stereo_mode=1, order=8, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=48000)]
    datas = [synth.generate(**dict(c, seed=7000 + i)).flac for i, c in enumerate(cfgs)]
    datas.insert(2, malformed.cases()["bad_sync_frame2"][0])
    with tensor.MelSpectrogram(16000) as mel:
        f, fl, infos = tensor.decode_to_features(datas, mel)
        x, lengths, infos2 = tensor.decode_to_tensor(datas, sample_rate=16000, mix="mono")
        assert infos == infos2 and [i[0] for i in infos].count("OK") == 4 and infos[2][0] != "OK"
        assert x.shape[1] == 1 and f.shape[:3] == (5, 1, 80)
        g, gl = mel(x, lengths)
        torch.cuda.synchronize()
        assert same_bits(f, g) and torch.equal(fl, gl)
        assert fl.tolist() == [int(n) // 160 + 1 if n else 0 for n in lengths.tolist()]
        assert fl[2] == 0 and torch.unique(f[2].contiguous().view(torch.int32)).numel() == 1
        assert abs(float(f[2].flatten()[0]) - np.log10(1e-10)) < 1e-5
        assert torch.unique(f[0].contiguous().view(torch.int32)).numel() > 100
