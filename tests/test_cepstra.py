"""GPU tests of zflac_hip_cepstra_project (k_mel_dct): every element of the shapes below in both
layouts and five dtype pairs against the float64 reference of the stored inputs and the f32 matrix,
and the bit-for-bit families: a run repeats; a row's bits do not depend on the batch; a frame's bits
do not depend on where the call's window starts, on the alignment of the tensors or on the layout;
a non-finite value stays in its frame.

The tolerance per element, with ref = sum_m T[k][m] l[m] in float64:
  1.01 (n_in + 1) 2^-24 sum_m |T[k][m]| |l[m]|  +  u_dt |ref|  (+ 2^-25 for f16: its subnormals)
A sum of n products in f32, in any order, fused or not, is within gamma_n sum |T| |l| of the exact
one with gamma_n = n u / (1 - n u), u = 2^-24 (one rounding per product and per addition; a fused
step has fewer); (n_in + 1) u with the 1 % in hand covers gamma_{n_in} up to n_in = 256. The
output dtype's rounding comes on top. Derived, not measured."""
import numpy as np
import pytest
import torch

from zflac_amd import tensor

from . import cepstra_ref as R
from .cepstra_gpu import BF16, DEV, F16, F32, NAMES, TORCH_DT, Cepstra, from_layout, guard_room, guarded, guards_intact, \
    out_rounding, same_bits, to_layout

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 2), (5, 3), (23, 13), (80, 13), (80, 80), (255, 256), (256, 256)]
FRAMES = [1, 2, 63, 64, 65, 130]
PAIRS = [(F32, F32), (F32, F16), (F32, BF16), (F16, F32), (BF16, F32)]
_CACHE = {}


def matrix(n_in, n_out):
    """The liftered DCT where there is one (n_out <= n_in), noise otherwise."""
    if n_out <= n_in:
        return tensor.dct_matrix(n_out, n_in, lifter=22.0)
    return np.random.default_rng(n_in * 1000 + n_out).standard_normal((n_out, n_in)).astype(np.float32)


def inputs(n_in, frames, dtype):
    """[3, n_in, frames] in the stored dtype, on the host: log-mel-like noise, a row whose frames are
    each one value in every bin (only c0 is non-zero, to rounding), a zero row."""
    key = (n_in, frames, dtype)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(n_in * 977 + frames)
        x = torch.randn(3, n_in, frames, generator=g) * 3.0 - 5.0
        x[1] = (torch.randn(1, frames, generator=g) * 3.0 - 5.0).expand(n_in, frames)
        x[2] = 0.0
        _CACHE[key] = x.to(TORCH_DT[dtype])
    return _CACHE[key]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{NAMES[p[0]]}-{NAMES[p[1]]}")
@pytest.mark.parametrize("layout", [0, 1], ids=["bins_first", "frames_first"])
@pytest.mark.parametrize("n_in,n_out", SHAPES)
def test_against_float64(gpu_ready, n_in, n_out, layout, pair):
    di, do = pair
    T = matrix(n_in, n_out)
    worst = 0.0
    with Cepstra(n_in, n_out, layout, di, do, T) as p:
        for frames in FRAMES:
            x = inputs(n_in, frames, di)
            ref, mag = R.project(T, x.double().numpy())
            tol = 1.01 * (n_in + 1) * 2.0 ** -24 * mag + out_rounding(ref, do)
            got = from_layout(p.project(to_layout(x, layout).to(DEV)), layout).double().cpu().numpy()
            assert np.isfinite(got).all()
            err = np.abs(got - ref)
            assert (got[2] == 0).all()  # the zero row: exact zeros
            nz = tol > 0
            if nz.any():
                worst = max(worst, float((err[nz] / tol[nz]).max()))
            assert (err <= tol).all(), (frames, worst)
    print(f"dct {n_in}->{n_out} layout {layout} {NAMES[di]}->{NAMES[do]}: worst error / bound = {worst:.4f}")


@pytest.mark.parametrize("pair", [(F32, F32), (BF16, F32), (F32, F16)], ids=lambda p: f"{NAMES[p[0]]}-{NAMES[p[1]]}")
@pytest.mark.parametrize("layout", [0, 1], ids=["bins_first", "frames_first"])
@pytest.mark.parametrize("n_in,n_out", [(5, 3), (80, 13), (255, 256)])
def test_bits(gpu_ready, n_in, n_out, layout, pair):
    di, do = pair
    frames, rows = 130, 5
    T = matrix(n_in, n_out)
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(rows, n_in, frames, generator=g) * 3.0 - 5.0).to(TORCH_DT[di])
    xl = to_layout(x, layout).to(DEV)
    with Cepstra(n_in, n_out, layout, di, do, T) as p:
        whole = p.project(xl)
        assert same_bits(p.project(xl), whole)  # a run repeats
        for i in (0, 2, 4):  # a row alone, wherever it sat in the batch
            assert same_bits(p.project(xl[i:i + 1].contiguous()), whole[i:i + 1]), i
        w = from_layout(whole, layout)
        for first in (1, 63, 64, 65):  # a window of the frames: the same frames of the whole run
            part = p.project(to_layout(x[:, :, first:], layout).to(DEV))
            assert same_bits(from_layout(part, layout), w[:, :, first:]), first
        es_in, es_out = xl.element_size(), whole.element_size()
        for shift in (1, 2, 3, 5):  # src and dst off the allocation's boundary, guard elements around both
            src, s0 = guarded(xl, shift)
            dst, d0 = guard_room(whole.numel(), whole.dtype, {1: 5, 2: 3, 3: 2, 5: 1}[shift])
            rc = p.project_ptr(src.data_ptr() + es_in * s0, dst.data_ptr() + es_out * d0, rows, frames)
            torch.cuda.synchronize()
            assert rc == 0
            assert same_bits(dst[d0:d0 + whole.numel()].view(whole.shape), whole), shift
            assert guards_intact(dst, d0, whole.numel()) and guards_intact(src, s0, xl.numel()), shift
        # a non-finite value stays in its frame
        y = x.clone()
        y[1, n_in // 2, 64] = float("nan")
        y[1, 0, 3] = 1e30 if di != F16 else 60000.0
        bad = from_layout(p.project(to_layout(y, layout).to(DEV)), layout)
        keep = torch.ones(frames, dtype=torch.bool)
        keep[[3, 64]] = False
        assert same_bits(bad[:, :, keep], w[:, :, keep])
        assert bool(torch.isnan(bad[1, :, 64]).all())  # fma(0, NaN, acc) is NaN too: the whole frame
    # the other layout: the same bits, transposed
    with Cepstra(n_in, n_out, 1 - layout, di, do, T) as q:
        other = q.project(to_layout(x, 1 - layout).to(DEV))
        assert same_bits(from_layout(other, 1 - layout).contiguous(), w.contiguous())


def test_refusals_with_a_device(gpu_ready):
    """What cannot be shown without a plan: the run calls' refusals enqueue nothing and say so."""
    T = matrix(5, 3)
    with Cepstra(5, 3, 0, F32, F32, T) as p, Cepstra(5, 5, 0, F32, F32, None, 1, 2) as d:
        x = torch.zeros(1, 5, 4, device=DEV)
        out = torch.full((1, 3, 4), 9.0, device=DEV)
        assert p.project_ptr(x.data_ptr(), x.data_ptr(), 1, 4) == 14       # src == dst
        assert p.project_ptr(x.data_ptr(), out.data_ptr(), 1, 0) == 14     # frames == 0
        assert p.project_ptr(x.data_ptr() + 2, out.data_ptr(), 1, 4) == 14  # src's alignment
        assert p.project_ptr(x.data_ptr(), out.data_ptr(), 0, 4) == 0      # rows == 0: nothing done
        assert d.project_ptr(x.data_ptr(), out.data_ptr(), 1, 4) == 14     # a plan without a matrix
        assert p.deltas_ptr(x.data_ptr(), out.data_ptr(), 1, 4) == 14      # a plan without deltas
        torch.cuda.synchronize()
        assert bool((out == 9.0).all())
        assert p.L.zflac_hip_cepstra_features(p.h) == 3 and d.L.zflac_hip_cepstra_features(d.h) == 10
