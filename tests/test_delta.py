"""GPU tests of zflac_hip_cepstra_deltas (k_mel_delta): C x (order, window) x layout x dtype with
frames = 133 and valid lengths at every edge of the clamp, against the float64 reference
(tests/cepstra_ref.py) of the stored inputs and the plan's f32 taps. Every frame at or past a row's
valid length holds 1e30 in src (60000 in f16), so a read past the clamp shows; block 0 is the input
bit for bit; conv(pad_value) sits exactly at t >= F_i in every block.

The tolerance per element of block o, n = 2 o W + 1 taps:
  1.01 (n + 1) 2^-24 sum_j |s_o[j]| |x[clamp(t + j)]|  +  u_dt |ref|  (+ 2^-25 for f16)
the bound of an f32 sum of n products in any order (tests/test_cepstra.py), then the output
dtype's rounding. The taps themselves are checked against the float64 recipe within one f32 rounding.

The ramp. With W = 1 every tap is a dyadic rational (s_1 = [-1, 0, 1] / 2, s_2 = [1, 0, -2, 0, 1] / 4,
s_3 = [-1, 0, 3, 0, -3, 0, 1] / 8), so on x[t] = (t - 6) / 2, whose values and partial sums are small
multiples of 2^-4, every product and sum is exact in f32 and in all three dtypes: the order-1
delta is exactly 1/2 and the order-2 and order-3 deltas exactly 0 at every interior frame. With
W = 2 or 5 the taps j / 10, j / 110 are not representable: the rounded order-2 taps do not sum
to 0 (W = 2: 2 fl(.04) + 2 fl(.01) - fl(.1) = -3.7e-9), so "exactly" is not a property of the
definition there and the ramp is held to the bound above, which still pins signs and order
(the bound, the bf16 rounding of the result included, is below 1 % of the slope)."""
import numpy as np
import pytest
import torch

from zflac_amd import tensor

from . import cepstra_ref as R
from .cepstra_gpu import BF16, DEV, F16, F32, NAMES, TORCH_DT, Cepstra, from_layout, guard_room, guarded, guards_intact, \
    out_rounding, same_bits, to_layout

pytestmark = pytest.mark.gpu

FRAMES = 133
CASES = [(1, 1), (1, 2), (2, 2), (3, 1), (2, 5), (3, 5)]
_CACHE = {}


def lengths(order, W):
    return sorted({0, 1, 2, W, 2 * W, 2 * W + 1, 2 * order * W, 2 * order * W + 1, 63, 64, 65, FRAMES})


def junk(dtype):
    return 60000.0 if dtype == F16 else 1e30


def features(rows, C, dtype, valid):
    """[rows, C, FRAMES] in the stored dtype on the host, junk at every frame >= valid[i]."""
    key = (rows, C, dtype, tuple(valid))
    if key not in _CACHE:
        g = torch.Generator().manual_seed(C * 131 + rows)
        x = torch.randn(rows, C, FRAMES, generator=g) * 3.0 - 5.0 + torch.arange(C).view(1, -1, 1) * 0.05
        for i, F in enumerate(valid):
            x[i, :, F:] = junk(dtype)
        _CACHE[key] = x.to(TORCH_DT[dtype])
    return _CACHE[key]


def plan_scales(p):
    """The plan's taps per order, each within one f32 rounding of the float64 recipe."""
    s = {o: p.scales(o) for o in range(1, p.order + 1)}
    for o, v in s.items():
        want = tensor.delta_scales(o, p.window)
        # (a tap that is 0 but for the float64 sums' cancellation, order 2 at W = 5, is 1e-19 either way)
        assert v.shape == want.shape and np.all(np.abs(v.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 2.0 ** -60)
    assert p.scales(0).tolist() == [1.0]
    return s


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("layout", [0, 1], ids=["bins_first", "frames_first"])
@pytest.mark.parametrize("order,W", CASES)
@pytest.mark.parametrize("C", [1, 5, 13, 80, 256])
def test_against_float64(gpu_ready, C, order, W, layout, dtype):
    valid = lengths(order, W)
    rows = len(valid)
    pad = -2.5
    x = features(rows, C, dtype, valid)
    xl = to_layout(x, layout).to(DEV)
    worst = 0.0
    with Cepstra(C, C, layout, dtype, dtype, None, order, W) as p:
        s = plan_scales(p)
        ref, mag = R.deltas(x.double().numpy(), order, W, valid, pad, scales=s)
        got_t = p.deltas(xl, valid, pad)
        got = from_layout(got_t, layout)
        g64 = got.double().cpu().numpy()
        assert np.isfinite(g64).all()
        for i, F in enumerate(valid):
            assert same_bits(got[i, :C, :F].cpu(), x[i, :, :F]), i          # block 0: the input's bits
            assert bool((got[i, :, F:] == pad).all()), i                     # conv(pad) in every block (-2.5 is exact)
        for o in range(1, order + 1):
            blk = slice(o * C, (o + 1) * C)
            tol = 1.01 * (2 * o * W + 2) * 2.0 ** -24 * mag[:, blk] + out_rounding(ref[:, blk], dtype)
            live = mag[:, blk] > 0
            err = np.abs(g64[:, blk] - ref[:, blk])
            assert (err[live] <= tol[live]).all(), (o, float((err[live] / tol[live]).max()))
            if live.any():
                worst = max(worst, float((err[live] / tol[live]).max()))
        assert same_bits(p.deltas(xl, valid, pad), got_t)  # a run repeats
        # no lengths is every length = frames (the junk is then signal: any finite value will do)
        full = p.deltas(xl[-1:].contiguous(), None, pad)
        assert same_bits(full, got_t[-1:]) and valid[-1] == FRAMES
    print(f"delta C {C} order {order} W {W} layout {layout} {NAMES[dtype]}: worst error / bound = {worst:.4f}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", [0, 1], ids=["bins_first", "frames_first"])
@pytest.mark.parametrize("C,order,W", [(13, 2, 2), (80, 3, 5), (5, 1, 1)])
def test_a_rows_bits_alone_in_a_batch_and_misaligned(gpu_ready, C, order, W, layout, dtype):
    valid = [FRAMES, 77, 64, 1, FRAMES]
    rows = len(valid)
    x = features(rows, C, dtype, valid)
    xl = to_layout(x, layout).to(DEV)
    es = xl.element_size()
    with Cepstra(C, C, layout, dtype, dtype, None, order, W) as p:
        batch = p.deltas(xl, valid, 0.25)
        for i in (0, 1, 4):
            assert same_bits(p.deltas(xl[i:i + 1].contiguous(), valid[i:i + 1], 0.25), batch[i:i + 1]), i
        for shift in (1, 2, 3, 5):
            src, s0 = guarded(xl, shift)
            dst, d0 = guard_room(batch.numel(), batch.dtype, {1: 5, 2: 3, 3: 2, 5: 1}[shift])
            rc = p.deltas_ptr(src.data_ptr() + es * s0, dst.data_ptr() + es * d0, rows, FRAMES, valid, 0.25)
            torch.cuda.synchronize()
            assert rc == 0
            assert same_bits(dst[d0:d0 + batch.numel()].view(batch.shape), batch), shift
            assert guards_intact(dst, d0, batch.numel()) and guards_intact(src, s0, xl.numel()), shift


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("layout", [0, 1], ids=["bins_first", "frames_first"])
@pytest.mark.parametrize("order,W", CASES)
def test_ramp(gpu_ready, order, W, layout, dtype):
    """See the module's head: exact for W = 1, within the derived bound otherwise."""
    a, C = 0.5, 3
    t = torch.arange(FRAMES, dtype=torch.float32)
    x = ((t - 6.0) * a).view(1, 1, -1).expand(1, C, FRAMES).contiguous().to(TORCH_DT[dtype])
    assert torch.equal(x.float()[0, 0], (t - 6.0) * a)  # exactly representable in the dtype
    with Cepstra(C, C, layout, dtype, dtype, None, order, W) as p:
        got = from_layout(p.deltas(to_layout(x, layout).to(DEV)), layout).double().cpu().numpy()[0]
        s = plan_scales(p)
    ref, mag = R.deltas(x.double().numpy(), order, W, scales=s)
    for o in range(1, order + 1):
        inner = slice(o * W, FRAMES - o * W)
        d = got[o * C:(o + 1) * C, inner]
        want = a if o == 1 else 0.0
        if W == 1:
            assert np.all(d == want), (o, np.abs(d - want).max())
        else:
            tol = 1.01 * (2 * o * W + 2) * 2.0 ** -24 * mag[0, o * C:(o + 1) * C, inner] + out_rounding(want, dtype)
            assert np.all(np.abs(d - want) <= tol + np.abs(ref[0, o * C:(o + 1) * C, inner] - want)), (o, np.abs(d - want).max())
            assert tol.max() < 1e-2 * a  # far below the slope: a wrong sign or order cannot hide
