"""GPU tests of zflac_hip_mel_run_ex (k_mel_ex, k_mel_norm; MelSpectrogram's pad=, normalize=,
whisper()): parity of reflect padding and per-row lengths with the float64 reference of
tests/mel_reflect_ref.py within tests/mel_ref.py's bound; bit for bit against zflac_hip_mel_run
(an uncentred plan over host-reflected rows: the test a wrong rho, an off-by-one at n - 1 or a
changed order of summation cannot pass); tile and wave edges; independence of the window; lengths
with zero padding; the row maximum; the normalising pass bit for bit; streams; the Python layer."""
import ctypes
import functools

import torch  # before zflac_amd loads its library: one HIP runtime per process (zflac_amd/tensor.py)

import numpy as np
import pytest

import synth
from zflac_amd import _lib, errors, tensor

from . import malformed
from . import mel_ref as ref
from . import mel_reflect_ref as rr

pytestmark = pytest.mark.gpu

LAYOUTS = {"bins_first": _lib.MEL_BINS_FIRST, "frames_first": _lib.MEL_FRAMES_FIRST}
TORCH_DT = {_lib.EXPORT_F32: torch.float32, _lib.EXPORT_F16: torch.float16, _lib.EXPORT_BF16: torch.bfloat16}
ZEROS, REFLECT = _lib.PAD_ZEROS, _lib.PAD_REFLECT
FLOOR = 1e-10
DEV = torch.device("cuda", 0)
JUNK = 1e30  # what lies past a row's length and between rows: must never be read as signal


class Plan:
    """zflac_hip_mel_create / _run / _run_ex / _destroy through ctypes, on torch tensors."""

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

    def view(self, out):
        return out if self.layout == 0 else out.transpose(1, 2)

    def run(self, buf, rows, wave_frames, row_stride, first, frames, offset=0):
        """zflac_hip_mel_run: buf a flat float32 cuda tensor holding the rows from element `offset` on."""
        out = torch.empty(self.shape(rows, frames), dtype=TORCH_DT[self.dtype], device=DEV)
        torch.cuda.synchronize()
        rc = self.L.zflac_hip_mel_run(self.h, buf.data_ptr() + 4 * offset, rows, wave_frames, row_stride, first, frames,
                                      out.data_ptr(), out.numel() * out.element_size(), None)
        errors.check(rc, "mel_run")
        return self.view(out)

    def desc(self, wave_ptr, rows, wave_frames, row_stride, first, frames, dst_ptr, dst_bytes, pad=REFLECT, lengths=None,
             row_max=None, norm=None):
        rng, add, mul = norm or (0.0, 0.0, 0.0)
        return _lib.zflac_mel_run_desc(ctypes.sizeof(_lib.zflac_mel_run_desc), pad,
                                       _lib.NORM_NONE if norm is None else _lib.NORM_ROW_MAX, 0, wave_ptr, rows, wave_frames,
                                       row_stride, None if lengths is None else lengths.data_ptr(), first, frames, dst_ptr,
                                       dst_bytes, None if row_max is None else row_max.data_ptr(), rng, add, mul, 0)

    def run_ex(self, buf, rows, wave_frames, row_stride, first, frames, pad=REFLECT, lengths=None, norm=None, row_max=False,
               offset=0):
        """zflac_hip_mel_run_ex on the plan's own stream -> the tensor, or (tensor, row maxima)."""
        out = torch.empty(self.shape(rows, frames), dtype=TORCH_DT[self.dtype], device=DEV)
        ln = None if lengths is None else torch.tensor([int(n) for n in lengths], dtype=torch.int64, device=DEV)
        rm = torch.full((rows,), float("nan"), device=DEV) if row_max or norm else None
        d = self.desc(buf.data_ptr() + 4 * offset, rows, wave_frames, row_stride, first, frames, out.data_ptr(),
                      out.numel() * out.element_size(), pad, ln, rm, norm)
        torch.cuda.synchronize()
        errors.check(self.L.zflac_hip_mel_run_ex(self.h, ctypes.byref(d), None), "mel_run_ex")
        return (self.view(out), rm) if row_max or norm else self.view(out)

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


def window_of(N):
    return ref.hann(N) if N > 2 else np.array([0.75, 1.0], np.float32)


def strided(x, stride, lengths=None):
    """x: float32 [rows, T] -> a flat cuda tensor with rows `stride` apart; JUNK past each row's length and between rows."""
    rows, T = x.shape
    h = np.full((rows, stride), JUNK, dtype=np.float32)
    for i in range(rows):
        n = T if lengths is None else min(int(lengths[i]), T)
        h[i, :n] = x[i, :n]
    return torch.from_numpy(h.reshape(-1)).to(DEV)


def check(got, want, tol, what):
    """|got - want| <= tol everywhere (exactly equal where tol is 0); prints the worst error-to-bound ratio."""
    got = got.detach().cpu().double().numpy()
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    exact = tol == 0
    assert (err[exact] == 0).all(), what
    ratio = float((err[~exact] / tol[~exact]).max()) if (~exact).any() else 0.0
    print(f"{what}: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0, what


def same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    v = torch.int32 if a.element_size() == 4 else torch.int16
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def plus_zero(t):
    return not t.contiguous().view(torch.int32).any()


# ---- 1. parity with the float64 reference ---------------------------------------------------

PARITY = [(400, 160, 80), (16, 3, 5), (30, 7, 33), (2048, 2048, 256), (2, 1, 2)]


@functools.lru_cache(maxsize=None)
def parity_case(N, hop, n_bins):
    """The two batches of a configuration and their reference, computed once for both layouts."""
    rng = np.random.default_rng(N * 11 + hop)
    T = 40 * hop + 77
    t = np.arange(T, dtype=np.float64)
    imp = lambda at: np.where(t == at, 1.0, 0.0)  # noqa: E731
    sig = [rng.uniform(-1.0, 1.0, T), np.round(0.8 * np.sin(2.0 * np.pi * 0.0731 * t) * 32767.0) / 32768.0, np.ones(T),
           np.where(t % 2 == 0, 1.0, -1.0), imp(0), imp(1), imp(T - 2), imp(T - 1), np.zeros(T)]
    w, F = window_of(N), filters_of(rng, n_bins, N // 2 + 1)
    frames = ref.mel_frames(T, N, hop, 1) + 2  # two past the longest row's count: computed from the reflected row
    assert frames % 32 != 0
    a = np.stack(sig).astype(np.float32)
    la = [T] * len(sig)
    b = rng.uniform(-1.0, 1.0, (7, T)).astype(np.float32)
    lb = [T, T + 5, N // 2 + 1, N // 2, 1, 0, 17 * hop + 3]
    batches = []
    for x, lengths in ((a, la), (b, lb)):
        v, e_v = rr.features(x, lengths, w, F, hop, 0, frames)
        batches.append((x, lengths, v, e_v))
    return dict(T=T, w=w, F=F, frames=frames, batches=batches)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("N,hop,n_bins", PARITY)
def test_parity(gpu_ready, N, hop, n_bins, layout):
    c = parity_case(N, hop, n_bins)
    T, stride = c["T"], c["T"] + 3
    with Plan(c["w"], c["F"], hop, 1, ref.POWER, LAYOUTS[layout]) as p:
        for x, lengths, v, e_v in c["batches"]:
            got = p.run_ex(strided(x, stride, lengths), len(lengths), T, stride, 0, c["frames"], REFLECT, lengths)
            check(got, v, e_v, f"reflect {N, hop, n_bins} {layout} lengths {lengths}")
            for i, n in enumerate(lengths):
                if n == 0 or not x[i, :min(n, T)].any():
                    assert plus_zero(got[i]), (i, n)  # +0, every bit


# ---- 2, 3. bit for bit against zflac_hip_mel_run -------------------------------------------


def against_the_old_kernel(N, hop, n_bins, lengths, seed, interior=True):
    """The reflect run of noise rows of `lengths` in one batch == zflac_hip_mel_run of an uncentred plan with the same
    tables over each row reflected on the host, every frame; and its interior frames == the centred zeros run."""
    rng = np.random.default_rng(seed)
    T = max(lengths)
    x = rng.uniform(-1.0, 1.0, (len(lengths), T)).astype(np.float32)
    w, F = window_of(N), filters_of(rng, n_bins, N // 2 + 1)
    frames = max(ref.mel_frames(n, N, hop, 1) for n in lengths) + 2
    width = (frames - 1) * hop + N
    with Plan(w, F, hop, 1) as pc, Plan(w, F, hop, 0) as pu:
        got = pc.run_ex(strided(x, T + 3, lengths), len(lengths), T, T + 3, 0, frames, REFLECT, lengths)
        for i, n in enumerate(lengths):
            host = rr.padded(x[i], n, N, width).astype(np.float32)[None, :]
            want = pu.run(strided(host, width), 1, width, width, 0, frames)
            assert same_bits(got[i:i + 1], want), (N, hop, i, n)
        if interior:
            cut = x.copy()
            for i, n in enumerate(lengths):
                cut[i, n:] = 0.0
            zeros = pc.run(strided(cut, T), len(lengths), T, T, 0, frames)
            seen = 0
            for i, n in enumerate(lengths):
                ts = [t for t in range(frames) if t * hop - N // 2 >= 0 and t * hop - N // 2 + N <= n]
                if ts:
                    assert same_bits(got[i][:, ts[0]:ts[-1] + 1], zeros[i][:, ts[0]:ts[-1] + 1]), (N, hop, i, n)
                    assert not same_bits(got[i][:, :ts[0]], zeros[i][:, :ts[0]])  # the padding is there
                    seen += 1
            assert seen


@pytest.mark.parametrize("N,hop,n_bins", [(400, 160, 80), (16, 3, 5), (2048, 2048, 256)])
def test_bits_of_the_old_kernel(gpu_ready, N, hop, n_bins):
    T = 40 * hop + 77
    against_the_old_kernel(N, hop, n_bins, [T, T - 1, 20 * hop + 5, N // 2 + 1, N + 3, N // 2, 2, 1], N + hop)


@pytest.mark.parametrize("N,hop,n_bins", [(400, 160, 80), (16, 3, 5)])
@pytest.mark.parametrize("edge", [128, 32])
def test_tile_and_wave_edges(gpu_ready, N, hop, n_bins, edge):
    """Rows whose end reflection straddles frames edge - 1 / edge: the last tile (or wave) boundary inside the padding."""
    lengths = [edge * hop + r for r in (-1, 0, 1, N // 2 - 1, N // 2, N // 2 + 1)]
    against_the_old_kernel(N, hop, n_bins, lengths, N + edge)


@pytest.mark.parametrize("n", [128 * 2048 + 1, 32 * 2048 + 1023, 32 * 2048 - 1])
def test_tile_and_wave_edges_at_the_largest_hop(gpu_ready, n):
    against_the_old_kernel(2048, 2048, 256, [n], n, interior=False)


# ---- 4, 5. the window, the rows, the alignment; lengths with zero padding ------------------


@pytest.fixture(scope="module")
def whisper(gpu_ready):
    rng = np.random.default_rng(98)
    N, hop, T = 400, 160, 40 * 160 + 77
    rows = 5
    x = rng.uniform(-1.0, 1.0, (rows, T)).astype(np.float32)
    x[3] = 0.0
    lengths = [T, 20 * 160 + 5, 33 * 160 - 7, T, 201]
    w, F = ref.hann(N), tensor.mel_filters(16000, N, 80)
    frames = ref.mel_frames(T, N, hop, 1) + 2
    p = Plan(w, F, hop, 1, ref.LOG10)
    buf = strided(x, T + 3, lengths)
    full, row_max = p.run_ex(buf, rows, T, T + 3, 0, frames, REFLECT, lengths, row_max=True)
    yield dict(p=p, x=x, T=T, rows=rows, lengths=lengths, frames=frames, full=full, row_max=row_max, w=w, F=F, buf=buf)
    p.close()


@pytest.mark.parametrize("first,n", [(1, 7), (31, 7), (32, 7), (33, 7), (21, 5), (39, 4)])
def test_independence_of_the_window(whisper, first, n):
    """(21, 5) lies wholly in the end region of row 1, (39, 4) in that of the full rows and past the count."""
    m = whisper
    got = m["p"].run_ex(m["buf"], m["rows"], m["T"], m["T"] + 3, first, n, REFLECT, m["lengths"])
    assert same_bits(got, m["full"][:, :, first:first + n])


def test_independence_of_rows_and_alignment(whisper):
    m = whisper
    T = m["T"]
    one = m["p"].run_ex(strided(m["x"][1:2], T, m["lengths"][1:2]), 1, T, T, 0, m["frames"], REFLECT, m["lengths"][1:2])
    assert same_bits(one[0], m["full"][1])
    for shift in (1, 2, 3):  # wave_device 4, 8, 12 bytes past a 16-byte boundary
        buf = torch.cat([torch.full((shift,), JUNK, device=DEV), m["buf"]])
        assert buf.data_ptr() % 16 == 0
        got = m["p"].run_ex(buf, m["rows"], T, T + 3, 0, m["frames"], REFLECT, m["lengths"], offset=shift)
        assert same_bits(got, m["full"]), shift
    # lengths_device == NULL: every row ends at wave_frames
    got = m["p"].run_ex(strided(m["x"], T + 3), m["rows"], T, T + 3, 0, m["frames"], REFLECT, None)
    assert same_bits(got[0], m["full"][0]) and same_bits(got[3], m["full"][3])
    assert not same_bits(got[1], m["full"][1])


def test_lengths_with_zero_padding_and_the_default_descriptor(whisper):
    m = whisper
    T, p = m["T"], m["p"]
    cut = m["x"].copy()
    for i, n in enumerate(m["lengths"]):
        cut[i, n:] = 0.0
    old = p.run(strided(cut, T + 3), m["rows"], T, T + 3, 0, m["frames"])
    got = p.run_ex(m["buf"], m["rows"], T, T + 3, 0, m["frames"], ZEROS, m["lengths"])  # JUNK past every length
    assert same_bits(got, old)
    over = [n + T for n in m["lengths"]]  # clamped to wave_frames
    assert same_bits(p.run_ex(strided(cut, T + 3), m["rows"], T, T + 3, 0, m["frames"], ZEROS, over),
                     p.run(strided(cut, T + 3), m["rows"], T, T + 3, 0, m["frames"]))
    plain = p.run_ex(strided(m["x"], T + 3), m["rows"], T, T + 3, 0, m["frames"], ZEROS, None)
    assert same_bits(plain, p.run(strided(m["x"], T + 3), m["rows"], T, T + 3, 0, m["frames"]))
    # what the old call refuses with the device there, the new one refuses
    out = torch.empty(p.shape(m["rows"], m["frames"]), device=DEV)
    args = (m["rows"], T, T + 3, 0, m["frames"], out.data_ptr(), out.numel() * 4)
    run = lambda d: p.L.zflac_hip_mel_run_ex(p.h, ctypes.byref(d), None)  # noqa: E731
    assert run(p.desc(m["buf"].data_ptr() + 2, *args)) == 14
    assert run(p.desc(m["buf"].data_ptr(), m["rows"], T + 4, T + 3, 0, m["frames"], out.data_ptr(), out.numel() * 4)) == 14
    assert run(p.desc(m["buf"].data_ptr(), m["rows"], T, T + 3, 0, m["frames"], out.data_ptr(), out.numel() * 4 - 1)) == 14
    assert run(p.desc(m["buf"].data_ptr(), 0, T, T + 3, 0, m["frames"], out.data_ptr(), 0)) == 0
    with Plan(m["w"], m["F"], 160, 0, ref.LOG10) as uncentred:
        assert uncentred.L.zflac_hip_mel_run_ex(uncentred.h, ctypes.byref(uncentred.desc(m["buf"].data_ptr(), *args)), None) == 14
        clean = strided(m["x"], T + 3)
        assert same_bits(uncentred.run_ex(clean, m["rows"], T, T + 3, 0, 30, ZEROS, None),
                         uncentred.run(clean, m["rows"], T, T + 3, 0, 30))


# ---- 6. the row maximum --------------------------------------------------------------------


def max_rows(rng, T):
    """all-negative logs, positive logs, a zero row, a short row -> (x, lengths)"""
    x = rng.uniform(-1.0, 1.0, (4, T)).astype(np.float32)
    x[0] *= np.float32(1e-3)
    x[1] *= np.float32(100.0)
    x[2] = 0.0
    return x, [T, T, T, T // 3]


@pytest.mark.parametrize("frames", [1, 128, 129])
@pytest.mark.parametrize("N,hop,n_bins", [(400, 160, 80), (16, 3, 5), (400, 160, 256)])
def test_row_maximum(gpu_ready, N, hop, n_bins, frames):
    rng = np.random.default_rng(N + n_bins + frames)
    T = 129 * hop + 77
    x, lengths = max_rows(rng, T)
    w = ref.hann(N)
    F = tensor.mel_filters(16000, N, 80) if n_bins == 80 else filters_of(rng, n_bins, N // 2 + 1)
    buf = strided(x, T, lengths)
    for scale in (ref.LOG10, ref.POWER):
        for pad in (REFLECT, ZEROS):
            with Plan(w, F, hop, 1, scale) as p:
                out, rm = p.run_ex(buf, 4, T, T, 0, frames, pad, lengths, row_max=True)
                plain = p.run_ex(buf, 4, T, T, 0, frames, pad, lengths)
            assert same_bits(out, plain)  # asking for the maxima changes nothing else
            assert same_bits(rm, out.amax(dim=(1, 2))), (scale, pad, rm, out.amax(dim=(1, 2)))
            if scale == ref.LOG10:
                if frames > 1:
                    assert (out[0] < 0).all() and float(rm[0]) < 0 and float(rm[1]) > 0
                assert torch.unique(out[2].contiguous().view(torch.int32)).numel() == 1  # log10f(floor), the device's bits
                assert abs(float(rm[2]) - np.log10(FLOOR)) < 1e-5
            else:
                assert plus_zero(rm[2:3]) and float(rm[1]) > 0
            for dtype in (_lib.EXPORT_F16, _lib.EXPORT_BF16) if pad == REFLECT else ():  # the maximum is taken before the rounding
                for layout in (0, 1):
                    with Plan(w, F, hop, 1, scale, layout, dtype) as ph:
                        oh, rh = ph.run_ex(buf, 4, T, T, 0, frames, pad, lengths, row_max=True)
                    assert same_bits(rh, rm), (scale, pad, dtype, layout)
                    assert same_bits(oh, out.to(TORCH_DT[dtype]))


# ---- 7. the normalising pass ----------------------------------------------------------------


def normalised(none, row_max, norm):
    """The header's formula with separate f32 torch operations on the stored NORM_NONE values."""
    rng, add, mul = norm
    thr = row_max - rng                                   # one f32 rounding
    c = torch.maximum(none.float(), thr[:, None, None])
    s = c + add
    return (s * mul).to(none.dtype)


@pytest.mark.parametrize("norm", [(8.0, 4.0, 0.25), (3.5, -1.3, -0.7)])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dtype", list(TORCH_DT))
def test_normalisation_bit_for_bit(gpu_ready, dtype, layout, norm):
    # (N, hop, n_bins, frames): one pass per row and odd; two passes per row, odd; Whisper's bins, three passes
    for N, hop, n_bins, frames in ((16, 3, 5, 129), (16, 3, 5, 1001), (400, 160, 80, 129)):
        rng = np.random.default_rng(N + frames)
        T = frames * hop + 11
        x, lengths = max_rows(rng, T)
        x[1] *= np.float32(0.01)
        w = ref.hann(N)
        F = tensor.mel_filters(16000, N, 80) if n_bins == 80 else filters_of(rng, n_bins, N // 2 + 1)
        buf = strided(x, T, lengths)
        with Plan(w, F, hop, 1, ref.LOG10, LAYOUTS[layout], dtype) as p:
            none, rm = p.run_ex(buf, 4, T, T, 0, frames, REFLECT, lengths, row_max=True)
            got, rm2 = p.run_ex(buf, 4, T, T, 0, frames, REFLECT, lengths, norm=norm)
            assert same_bits(rm, rm2)
            want = normalised(none, rm, norm)
            assert same_bits(got, want), (N, frames)
            clamped = (none.float() < (rm - norm[0])[:, None, None])
            assert clamped[3].any() and not clamped.all()  # the clamp acts (the zero frames behind the short row) and not everywhere
            # a destination one element past a 16-byte boundary, guards on both sides
            n, guard = 4 * n_bins * frames, 64
            big = torch.full((n + 2 * guard + 1,), float("nan"), dtype=TORCH_DT[dtype], device=DEV)
            dst = big[guard + 1:guard + 1 + n]
            assert (dst.data_ptr() - big.element_size()) % 16 == 0
            ln = torch.tensor(lengths, dtype=torch.int64, device=DEV)
            rm3 = torch.empty(4, device=DEV)
            torch.cuda.synchronize()
            d = p.desc(buf.data_ptr(), 4, T, T, 0, frames, dst.data_ptr(), n * big.element_size(), REFLECT, ln, rm3, norm)
            assert p.L.zflac_hip_mel_run_ex(p.h, ctypes.byref(d), None) == 0
            assert same_bits(p.view(dst.view(p.shape(4, frames))), want) and same_bits(rm3, rm)
            assert torch.isnan(big[:guard + 1]).all() and torch.isnan(big[guard + 1 + n:]).all()


# ---- 8. streams ------------------------------------------------------------------------------


def test_streams_and_plan_lifetime(whisper):
    m = whisper
    p, T, rows, frames = m["p"], m["T"], m["rows"], m["frames"]
    norm = (8.0, 4.0, 0.25)
    want, want_max = p.run_ex(m["buf"], rows, T, T + 3, 0, frames, REFLECT, m["lengths"], norm=norm)
    assert same_bits(want_max, m["row_max"])
    ln = torch.tensor(m["lengths"], dtype=torch.int64, device=DEV)
    outs = [torch.empty(p.shape(rows, frames), device=DEV) for _ in range(3)]
    maxs = [torch.empty(rows, device=DEV) for _ in range(3)]
    desc = lambda i, plan: plan.desc(m["buf"].data_ptr(), rows, T, T + 3, 0, frames, outs[i].data_ptr(),  # noqa: E731
                                     outs[i].numel() * 4, REFLECT, ln, maxs[i], norm)
    side, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert p.L.zflac_hip_mel_run_ex(p.h, ctypes.byref(desc(0, p)), side.cuda_stream) == 0
        doubled = outs[0] * 2  # on the same stream: ordered after the fill, k_mel_ex and k_mel_norm
        max_copy = maxs[0].clone()
    side.synchronize()
    assert same_bits(outs[0], want) and torch.equal(doubled, want * 2) and same_bits(max_copy, want_max)
    # two runs of one plan on two streams, each with its own row_max; then a plan destroyed behind an enqueued run
    assert p.L.zflac_hip_mel_run_ex(p.h, ctypes.byref(desc(1, p)), side.cuda_stream) == 0
    assert p.L.zflac_hip_mel_run_ex(p.h, ctypes.byref(desc(2, p)), s2.cuda_stream) == 0
    side.synchronize()
    s2.synchronize()
    for i in (1, 2):
        assert same_bits(outs[i], want) and same_bits(maxs[i], want_max), i
    p2 = Plan(m["w"], m["F"], 160, 1, ref.LOG10)
    outs[1].zero_()
    torch.cuda.synchronize()
    assert p2.L.zflac_hip_mel_run_ex(p2.h, ctypes.byref(desc(1, p2)), s2.cuda_stream) == 0
    p2.close()  # waits for the device
    assert same_bits(outs[1], want) and same_bits(maxs[1], want_max)


# ---- 9. the Python layer ----------------------------------------------------------------------


def stft_power(x, N, hop, window):
    """|STFT|^2 of float64 rows with torch.stft's reflect padding -> [B, K, frames]."""
    s = torch.stft(x, N, hop, window=window, center=True, pad_mode="reflect", return_complex=True)
    return s.abs() ** 2


def test_whisper_preset(gpu_ready):
    rng = np.random.default_rng(5)
    B, T = 3, 40 * 160 + 77
    xn = rng.uniform(-1.0, 1.0, (B, T)).astype(np.float32)
    xn[1, 3000:] = 0.0  # a shorter utterance, zero-filled as Whisper's rows are
    x = torch.from_numpy(xn).to(DEV)
    frames = T // 160  # Whisper drops the STFT's last frame
    with tensor.MelSpectrogram.whisper() as mel:
        assert (mel.n_fft, mel.hop, mel.n_bins, mel.pad, mel.normalize, mel.reflect_at) == (400, 160, 80, "reflect", (8.0, 4.0, 0.25), "end")
        got, fl = mel(x, torch.tensor([T, 3000, T]), frames=frames)
        torch.cuda.synchronize()
        assert got.shape == (B, 80, frames) and got.dtype == torch.float32
        assert fl.tolist() == [frames, 3000 // 160 + 1, frames]
        row_max = mel.last_row_max
        assert row_max.shape == (B,)
        w, F = mel.window, mel.filters
    # the composition, in float64 on the host
    P = stft_power(torch.from_numpy(xn).double(), 400, 160, torch.from_numpy(w).double())[:, :, :frames]
    logs = torch.clamp(torch.from_numpy(F).double() @ P, min=1e-10).log10()
    peak = logs.amax(dim=(1, 2), keepdim=True)
    comp = ((torch.maximum(logs, peak - 8.0) + 4.0) / 4.0).numpy()
    # the bound: mel_ref's log tolerance times mul, from the float64 reference, plus an f32 ulp of the result
    v, e_v = rr.features(xn, [T] * B, w, F, 160, 0, frames)
    out, tol = ref.scaled(v, e_v, ref.LOG10, 1e-10)
    want = (np.maximum(out, out.max(axis=(1, 2), keepdims=True) - 8.0) + 4.0) / 4.0
    assert np.abs(comp - want).max() < 1e-9  # the two float64 compositions agree: torch.stft's padding is the rule's
    bound = tol * 0.25 + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    check(got, comp, bound, "whisper preset against the torch.stft composition")
    assert np.abs(row_max.cpu().numpy() - out.max(axis=(1, 2))).max() < 1e-4
    assert (got.amin(dim=(1, 2)) >= got.amax(dim=(1, 2)) - 2.0 - 1e-6).all()  # a row spans (M - 4) / 4 .. (M + 4) / 4


def test_python_layer(whisper):
    m = whisper
    T, rows = m["T"], m["rows"]
    cut = m["x"].copy()
    for i, n in enumerate(m["lengths"]):
        cut[i, n:] = 0.0
    x = torch.from_numpy(cut).to(DEV)
    lengths = torch.tensor(m["lengths"])
    count = T // 160 + 1
    with tensor.MelSpectrogram(16000, pad="reflect") as mel:
        f, fl, rmax = mel(x, lengths, return_row_max=True)
        torch.cuda.synchronize()
        assert f.shape == (rows, 80, count) and fl.tolist() == [n // 160 + 1 for n in m["lengths"]]
        assert same_bits(f, m["full"][:, :, :count])
        assert rmax is mel.last_row_max and same_bits(rmax, f.amax(dim=(1, 2)))
        f2, _ = mel(x, lengths, frames=9, first_frame=17)
        torch.cuda.synchronize()
        assert same_bits(f2, m["full"][:, :, 17:26])
        # [B, C, T]: the lengths are per batch row, every channel of it has that length
        x3 = torch.stack([x[0], x[3], x[1], x[1]]).reshape(2, 2, T).contiguous()
        f3, fl3, r3 = mel(x3, torch.tensor([T, m["lengths"][1]]), return_row_max=True)
        torch.cuda.synchronize()
        assert f3.shape == (2, 2, 80, count) and fl3.shape == (2,) and r3.shape == (2, 2)
        for (b, c), i in {(0, 0): 0, (0, 1): 3, (1, 0): 1, (1, 1): 1}.items():
            assert same_bits(f3[b, c], m["full"][i][:, :count]), (b, c)
        assert same_bits(r3.reshape(4), f3.reshape(4, 80, count).amax(dim=(1, 2)))
    with tensor.MelSpectrogram(16000, pad="reflect", reflect_at="end") as mel:
        f, fl = mel(x, lengths)
        torch.cuda.synchronize()
        assert fl.tolist() == [n // 160 + 1 for n in m["lengths"]]
        assert same_bits(f[0], m["full"][0][:, :count]) and not same_bits(f[1], m["full"][1][:, :count])
    with tensor.MelSpectrogram(16000) as mel:  # the defaults: the old call, no maxima
        f, _ = mel(x, lengths)
        assert mel.last_row_max is None and (mel.pad, mel.normalize) == ("zeros", None)
    with tensor.MelSpectrogram(16000, normalize=(8, 4, 0.25), dtype=torch.bfloat16, layout="frames_first") as mel:
        g, _ = mel(x, lengths)  # zero padding, normalised
        torch.cuda.synchronize()
        assert g.shape == (rows, count, 80) and g.dtype == torch.bfloat16 and mel.last_row_max.shape == (rows,)
    for kw in (dict(pad="reflect", center=False), dict(pad="replicate"), dict(normalize=(8, 4, 0)), dict(normalize=(-1, 4, 1)),
               dict(normalize=(8, 4, 0.25), scale="power"), dict(reflect_at="start"), dict(normalize=(8, 4))):
        with pytest.raises(ValueError):
            tensor.MelSpectrogram(16000, **kw)


def test_decode_to_features_with_a_reflect_plan(gpu_ready):
    """A mixed-rate batch with an error stream: each row is reflected at its own length, the error row has length 0."""
    cfgs = [dict(channels=1, bps=8, order=3, precision=7, block_size=576, n_samples=3 * 576 + 77, sample_rate=8000),
            dict(channels=1, bps=16, order=6, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=22050),
            dict(channels=2, bps=16, stereo_mode=10, order=8, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=44100),
            dict(channels=2, bps=16, stereo_mode=1, order=8, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=48000)]
    datas = [synth.generate(**dict(c, seed=7100 + i)).flac for i, c in enumerate(cfgs)]
    datas.insert(2, malformed.cases()["bad_sync_frame2"][0])
    with tensor.MelSpectrogram(16000, pad="reflect", normalize=(8.0, 4.0, 0.25)) as mel, tensor.MelSpectrogram(16000) as zeros:
        f, fl, infos = tensor.decode_to_features(datas, mel)
        rmax = mel.last_row_max
        x, lengths, infos2 = tensor.decode_to_tensor(datas, sample_rate=16000, mix="mono")
        assert infos == infos2 and [i[0] for i in infos].count("OK") == 4 and infos[2][0] != "OK"
        assert x.shape[1] == 1 and f.shape[:3] == (5, 1, 80) and rmax.shape == (5, 1)
        g, gl = mel(x, lengths)
        torch.cuda.synchronize()
        assert same_bits(f, g) and torch.equal(fl, gl)
        assert fl.tolist() == [int(n) // 160 + 1 if n else 0 for n in lengths.tolist()]
        # the error stream: length 0, the constant an all-zero row gives: ((log10f(floor) clamped to itself) + 4) / 4
        assert fl[2] == 0 and torch.unique(f[2].contiguous().view(torch.int32)).numel() == 1
        assert abs(float(rmax[2, 0]) - np.log10(1e-10)) < 1e-5 and abs(float(f[2].flatten()[0]) - (np.log10(1e-10) + 4) / 4) < 1e-5
        assert torch.unique(f[0].contiguous().view(torch.int32)).numel() > 100
        # interior frames are the zeros plan's, normalised; the first frame is not
        z, _ = zeros(x, lengths)
        torch.cuda.synchronize()
        zn = (torch.maximum(z, rmax[:, :, None, None] - 8.0) + 4.0) * 0.25
        n0 = int(lengths[0])
        inside = [t for t in range(f.shape[3]) if t * 160 - 200 >= 0 and t * 160 + 200 <= n0]
        assert same_bits(f[0, 0][:, inside[0]:inside[-1] + 1], zn[0, 0][:, inside[0]:inside[-1] + 1])
        assert not same_bits(f[0, 0][:, :1], zn[0, 0][:, :1])
