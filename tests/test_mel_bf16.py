"""GPU tests of the split-bf16 feature plans (zflac_hip_mel_create_ex, ZFLAC_MEL_MATH_BF16X6 /
_BF16X3, k_mel_split) through zflac_hip_mel_run: parity with the kept-term float64 reference of
tests/mel_bf16_ref.py within the summation bound of the kernel's f32 accumulation, that the mode
ran, the f32 plan through the new entry, and what the f32 plan guarantees, of the split kernel
against itself: a frame's bits depend on the values under it alone, a zero row is one bit
pattern, the half dtypes round the f32 result, every element is written and nothing else, streams
and plan lifetime.

The bound: e_re = A = (t N16 + 2) 2^-23 S (1 + 2^-7), t = 6 or 3 terms, N16 = N padded to 16,
S = sum_n |c| |x|: t N16 products summed in any order with a faithfully rounded add each
(2 * 2^-24; the documents at hand do not say how the bf16 MFMA rounds its internal adds, nearest
would be 2^-24), two table roundings, over kept products whose magnitudes sum to at most
S (1 + 2^-7); propagated through P, v and the log as tests/mel_ref.py propagates its e_re."""
import ctypes
import functools

import torch  # before zflac_amd loads its library: one HIP runtime per process (zflac_amd/tensor.py)

import numpy as np
import pytest

from zflac_amd import _lib, errors, tensor

from . import mel_bf16_ref as bref
from . import mel_ref as ref
from . import test_mel_reflect as tr
from .test_mel import CONFIGS, FLOOR, ROWS, filters_of, signals
from .test_mel_reflect import DEV, LAYOUTS, TORCH_DT, check, same_bits

pytestmark = pytest.mark.gpu

MATHS = {"bf16x6": _lib.MEL_MATH_BF16X6, "bf16x3": _lib.MEL_MATH_BF16X3}
TERMS = {"bf16x6": 6, "bf16x3": 3, _lib.MEL_MATH_BF16X6: 6, _lib.MEL_MATH_BF16X3: 3}


class SplitPlan(tr.Plan):
    """tests/test_mel_reflect.py's Plan made by zflac_hip_mel_create_ex with a math."""

    def __init__(self, math, window, filters, hop, center, scale=ref.POWER, layout=0, dtype=_lib.EXPORT_F32, floor=None):
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
        errors.check(self.L.zflac_hip_mel_create_ex(ctypes.byref(d), math, 0, ctypes.byref(self.h)), "mel_create_ex")
        assert self.L.zflac_hip_mel_math(self.h) == math

    def run_raw(self, wave_ptr, rows, wave_frames, row_stride, first, frames, dst_ptr, dst_bytes, stream=None):
        return self.L.zflac_hip_mel_run(self.h, wave_ptr, rows, wave_frames, row_stride, first, frames, dst_ptr, dst_bytes,
                                        stream)


def strided(x, stride):
    return tr.strided(x, stride)  # 1e30 between the rows: what lies past wave_frames must never be read as signal


@functools.lru_cache(maxsize=None)
def parity_case(N, hop, n_bins, center, terms):
    """test_mel.py's batches of a configuration and their kept-term reference, computed once for both layouts."""
    rng = np.random.default_rng(N * 7 + hop)
    T = 40 * hop + 77
    w = ref.hann(N) if N > 2 else np.array([0.75, 1.0], np.float32)
    F = filters_of(rng, n_bins, N // 2 + 1)
    sig = signals(rng, N, hop, T)
    frames = ref.mel_frames(T, N, hop, center) + 2  # two past the count: computed from the zero-extended row
    assert frames % 32 != 0
    groups = [["noise", "tone16", "dc", "alternation", "impulse_first"],
              ["impulse_last", "impulse_tile_edge", "zero", "noise2", "tone16b"]]
    batches = []
    for names in groups:
        x = np.stack([sig[n] for n in names]).astype(np.float32)
        batches.append((names, x) + bref.features(x, w, F, hop, center, 0, frames, terms))
    x = rng.uniform(-1.0, 1.0, (ROWS, T)).astype(np.float32)
    return dict(T=T, w=w, F=F, frames=frames, batches=batches, noise=(x,) + bref.features(x, w, F, hop, center, 0, frames, terms))


@pytest.mark.parametrize("math", list(MATHS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("N,hop,n_bins,center", CONFIGS)
def test_parity(gpu_ready, N, hop, n_bins, center, layout, math):
    c = parity_case(N, hop, n_bins, center, TERMS[math])
    T, stride, frames = c["T"], c["T"] + 3, c["frames"]
    with SplitPlan(MATHS[math], c["w"], c["F"], hop, center, ref.POWER, LAYOUTS[layout]) as p:
        for names, x, v, e_v in c["batches"]:
            got = p.run(strided(x, stride), ROWS, T, stride, 0, frames)
            check(got, v, e_v, f"{math} power {N, hop, n_bins, center} {layout} {names}")
            if "zero" in names:
                assert not got[names.index("zero")].view(torch.int32).any()  # +0, every bit
    x, v, e_v = c["noise"]
    for scale in (ref.LOG10, ref.LN):
        want, tol = ref.scaled(v, e_v, scale, FLOOR)
        assert (tol <= 0.1).all()  # noise: no bin cancels, every element is compared (t N16 2^-22 at most, not N 2^-24)
        with SplitPlan(MATHS[math], c["w"], c["F"], hop, center, scale, LAYOUTS[layout]) as p:
            got = p.run(strided(x, stride), ROWS, T, stride, 0, frames)
        check(got, want, tol, f"{math} log scale {scale} {N, hop, n_bins, center} {layout}")


def test_the_mode_ran(gpu_ready):
    """The three maths give three different tensors on noise, and the six-term one is the closer to float64."""
    rng = np.random.default_rng(4)
    N, hop, T = 400, 160, 40 * 160 + 77
    x = rng.uniform(-1.0, 1.0, (1, T)).astype(np.float32)
    w, F = ref.hann(N), tensor.mel_filters(16000, N, 80)
    frames = ref.mel_frames(T, N, hop, 1)
    v, _ = ref.features(x, w, F, hop, 1, 0, frames)
    out = {}
    for name, math in dict(MATHS, f32=_lib.MEL_MATH_F32).items():
        with SplitPlan(math, w, F, hop, 1) as p:
            out[name] = p.run(strided(x, T), 1, T, T, 0, frames)
    assert not same_bits(out["bf16x6"], out["bf16x3"]) and not same_bits(out["bf16x6"], out["f32"])
    assert not same_bits(out["bf16x3"], out["f32"])
    err = {k: float(np.abs(o.cpu().double().numpy() - v).max()) for k, o in out.items()}
    print(f"worst |out - float64| on noise: {err}")
    assert err["bf16x6"] < err["bf16x3"]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dtype", list(TORCH_DT))
def test_f32_through_the_new_entry(gpu_ready, dtype, layout):
    rng = np.random.default_rng(8)
    for N, hop, n_bins, center in ((400, 160, 80, 1), (30, 7, 33, 1)):
        T = 40 * hop + 77
        x = rng.uniform(-1.0, 1.0, (ROWS, T)).astype(np.float32)
        w, F = ref.hann(N), filters_of(rng, n_bins, N // 2 + 1)
        frames = ref.mel_frames(T, N, hop, center) + 2
        lengths = [T, T // 2, 1, 0, T - 1]
        buf = tr.strided(x, T + 3, lengths)
        with tr.Plan(w, F, hop, center, ref.LOG10, LAYOUTS[layout], dtype) as old, \
                SplitPlan(_lib.MEL_MATH_F32, w, F, hop, center, ref.LOG10, LAYOUTS[layout], dtype) as new:
            assert same_bits(new.run(buf, ROWS, T, T + 3, 0, frames), old.run(buf, ROWS, T, T + 3, 0, frames))
            a, am = new.run_ex(buf, ROWS, T, T + 3, 0, frames, tr.REFLECT, lengths, norm=(8.0, 4.0, 0.25))
            b, bm = old.run_ex(buf, ROWS, T, T + 3, 0, frames, tr.REFLECT, lengths, norm=(8.0, 4.0, 0.25))
            assert same_bits(a, b) and same_bits(am, bm)


# ---- the split kernel against itself -------------------------------------------------------


@pytest.fixture(scope="module", params=list(MATHS))
def whisper(gpu_ready, request):
    math = MATHS[request.param]
    rng = np.random.default_rng(99)
    N, hop, T = 400, 160, 40 * 160 + 77
    x = rng.uniform(-1.0, 1.0, (ROWS, T)).astype(np.float32)
    x[3] = 0.0
    w, F = ref.hann(N), tensor.mel_filters(16000, N, 80)
    frames = ref.mel_frames(T, N, hop, 1) + 2
    p = SplitPlan(math, w, F, hop, 1, ref.LOG10)
    full = p.run(strided(x, T + 3), ROWS, T, T + 3, 0, frames)
    yield dict(p=p, math=math, x=x, T=T, frames=frames, full=full, w=w, F=F)
    p.close()


@pytest.mark.parametrize("first", [1, 31, 32, 33])
def test_independence_of_first_frame(whisper, first):
    m = whisper
    got = m["p"].run(strided(m["x"], m["T"] + 3), ROWS, m["T"], m["T"] + 3, first, 7)
    assert same_bits(got, m["full"][:, :, first:first + 7])


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
    # a row that starts one sample later is the same signal one sample earlier: hop = 1 moves it by a frame,
    # and a frame by a lane, a wave and (frame 128 -> 127) a workgroup
    with SplitPlan(m["math"], m["w"], m["F"], 1, 0, ref.LOG10) as p1:
        a = p1.run(strided(m["x"][:1], T), 1, T, T, 0, 300)
        b = p1.run(strided(m["x"][:1], T), 1, T - 1, T - 1, 0, 299, offset=1)
        assert same_bits(a[:, :, 1:300], b)


def test_zero_rows_hold_one_bit_pattern(whisper):
    z = whisper["full"][3]
    assert torch.unique(z.contiguous().view(torch.int32)).numel() == 1
    assert abs(float(z.flatten()[0]) - np.log10(FLOOR)) < 1e-5
    for scale, want in ((ref.LN, np.log(FLOOR)), (ref.POWER, 0.0)):
        with SplitPlan(whisper["math"], whisper["w"], whisper["F"], 160, 1, scale) as p:
            z = p.run(torch.zeros(1000, device=DEV), 1, 1000, 1000, 0, 9)
            assert torch.unique(z.contiguous().view(torch.int32)).numel() == 1
            assert abs(float(z.flatten()[0]) - want) < 1e-5
            if scale == ref.POWER:
                assert not z.view(torch.int32).any()  # +0


@pytest.mark.parametrize("dtype", [_lib.EXPORT_F16, _lib.EXPORT_BF16])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_half_dtypes_round_the_f32_result(whisper, dtype, layout):
    m = whisper
    x = m["x"] * np.float32(128.0)  # powers on both sides of 65504, f16's largest
    x[2] *= np.float32(1e-3)
    buf = strided(x, m["T"])
    for scale in (ref.POWER, ref.LOG10):
        with SplitPlan(m["math"], m["w"], m["F"], 160, 1, scale, LAYOUTS[layout]) as p32, \
                SplitPlan(m["math"], m["w"], m["F"], 160, 1, scale, LAYOUTS[layout], dtype) as p16:
            a = p32.run(buf, ROWS, m["T"], m["T"], 0, m["frames"])
            b = p16.run(buf, ROWS, m["T"], m["T"], 0, m["frames"])
        if scale == ref.POWER:
            assert float(a.max()) > 65504.0 and float(a[2].max()) < 60000.0
        want = a.to(TORCH_DT[dtype])
        assert b.dtype == want.dtype and same_bits(b, want)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("frames", [129, 128, 1])
def test_coverage_and_bounds(whisper, layout, frames):
    m = whisper
    guard, n = 257, ROWS * 80 * frames
    big = torch.full((n + 2 * guard,), float("nan"), device=DEV)
    buf = strided(m["x"], m["T"])
    with SplitPlan(m["math"], m["w"], m["F"], 160, 1, ref.POWER, LAYOUTS[layout]) as p:
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
    # two plans of different math alive at once, each on a stream of its own, and a plan destroyed with its run enqueued
    other = next(v for v in MATHS.values() if v != m["math"])
    s2 = torch.cuda.Stream(DEV)
    p2 = SplitPlan(other, m["w"], m["F"], 160, 1, ref.LOG10)
    with SplitPlan(other, m["w"], m["F"], 160, 1, ref.LOG10) as sync:
        want2 = sync.run(buf, *args)
    assert not same_bits(want2, m["full"])
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
