"""The resampler's host planning (zflac_amd/csrc/resample_plan.cpp: ratio, tap tables, lengths,
limits, tile rule) against the numpy reference (tests/resample_ref.py), without a GPU, and the
reference itself pinned by properties of the filter. The planner is built here with plain g++:
that it compiles is the check that it is free of HIP."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from zflac_amd import _lib

from . import resample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zflac_amd", "csrc")

PAIRS = [(44100, 16000), (48000, 16000), (8000, 16000), (37800, 16000), (96000, 16000), (768000, 16000),
         (22050, 48000), (44100, 48000), (11025, 16000)]


class Ratio(ctypes.Structure):
    _fields_ = [("L", ctypes.c_uint), ("M", ctypes.c_uint), ("W", ctypes.c_uint), ("K", ctypes.c_ulonglong),
                ("table_floats", ctypes.c_ulonglong), ("params_ok", ctypes.c_int), ("rates_ok", ctypes.c_int),
                ("k_over_limit", ctypes.c_int), ("table_over_budget", ctypes.c_int)]


@pytest.fixture(scope="module")
def probe():
    srcs = [os.path.join(ROOT, "tests", "c", "resample_probe.cpp"), os.path.join(CSRC, "resample_plan.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("resample_plan.h", "common.h")]
    lib = os.path.join(ROOT, "tests", "c", "_build", "libresample_probe.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Werror", "-O2", "-shared", "-fPIC", "-I", CSRC,
                               *srcs, "-o", lib])
    dll = ctypes.CDLL(lib)
    dll.resample_probe_ratio_of.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_double,
                                            ctypes.c_double, ctypes.POINTER(Ratio)]
    dll.resample_probe_ratio_of.restype = None
    dll.resample_probe_taps.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_double, ctypes.c_double,
                                        ctypes.POINTER(ctypes.c_float), ctypes.c_ulonglong]
    dll.resample_probe_taps.restype = ctypes.c_ulonglong
    dll.resample_probe_frames.argtypes = [ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_uint]
    dll.resample_probe_frames.restype = ctypes.c_ulonglong
    dll.resample_probe_tile.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_double, ctypes.c_uint] + [
        ctypes.POINTER(ctypes.c_uint)] * 4
    dll.resample_probe_tile.restype = None
    return dll


def _ratio(probe, fin, fout, Z=ref.ZEROS, rolloff=ref.ROLLOFF, beta=ref.BETA) -> Ratio:
    r = Ratio()
    probe.resample_probe_ratio_of(fin, fout, Z, rolloff, beta, ctypes.byref(r))
    return r


def _taps(probe, fin, fout, n, Z=ref.ZEROS, rolloff=ref.ROLLOFF, beta=ref.BETA) -> np.ndarray:
    out = np.zeros(n, dtype=np.float32)
    got = probe.resample_probe_taps(fin, fout, Z, rolloff, beta, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n)
    assert got == n
    return out


@pytest.mark.parametrize("fin,fout", PAIRS)
def test_plan_and_taps_match_the_reference(probe, fin, fout):
    L, M, W, K, h64 = ref.taps(fin, fout)
    r = _ratio(probe, fin, fout)
    assert (r.params_ok, r.rates_ok, r.k_over_limit, r.table_over_budget) == (1, 1, 0, 0)
    assert (r.L, r.M, r.W, r.K, r.table_floats) == (L, M, W, K, L * K)
    h = _taps(probe, fin, fout, L * K).reshape(L, K)
    want = h64.astype(np.float32)
    # within one unit in the last place of the larger of the two
    ulp = np.spacing(np.maximum(np.abs(h), np.abs(want)))
    worst = np.abs(h.astype(np.float64) - want.astype(np.float64)) / ulp
    assert worst.max() <= 1.0, (fin, fout, worst.max())
    assert np.array_equal(h == 0, want == 0)  # the window's support is the same set of taps
    sums = h.astype(np.float64).sum(axis=1)
    assert np.abs(sums - 1.0).max() <= K * 2.0 ** -24, (fin, fout, np.abs(sums - 1.0).max())


def test_the_issues_shapes():
    """The figures the kernel's design was argued from."""
    assert ref.ratio(44100, 16000)[:4] == (160, 441, 52, 105)
    assert ref.ratio(48000, 16000)[:4] == (1, 3, 57, 115)
    assert ref.ratio(768000, 16000)[:4] == (1, 48, 904, 1809)
    L, M, W, K, _ = ref.ratio(11025, 16000)
    assert (L, M, W, K) == (640, 441, 19, 39) and L * K == 24960


def test_limits_are_reported(probe):
    r = _ratio(probe, 768000, 16000, Z=64)  # W = ceil(64 * 48 / 0.85) = 3615
    assert (r.rates_ok, r.K, r.k_over_limit) == (1, 7231, 1)
    r = _ratio(probe, 768000, 16000, Z=36)  # W = 2033, K = 4067: the last that passes at this ratio
    assert (r.K, r.k_over_limit) == (4067, 0)
    r = _ratio(probe, 44101, 1048575)  # coprime: L = 1,048,575 phases of 39 taps
    assert (r.L, r.K, r.k_over_limit, r.table_over_budget) == (1048575, 39, 0, 1)
    assert _ratio(probe, 44100, 48000).table_over_budget == 0
    for fin, fout in ((0, 16000), (16000, 0), (1048576, 16000), (16000, 1048576)):
        assert _ratio(probe, fin, fout).rates_ok == 0
    for Z, rolloff, beta in ((0, 0.85, 8.0), (16, 0.0, 8.0), (16, 1.0000001, 8.0), (16, -0.5, 8.0), (16, 0.85, -1e-9),
                             (16, float("nan"), 8.0), (16, 0.85, float("nan")), (16, 0.85, float("inf"))):
        assert _ratio(probe, 44100, 16000, Z, rolloff, beta).params_ok == 0, (Z, rolloff, beta)
    assert _ratio(probe, 44100, 16000, 1, 1.0, 0.0).params_ok == 1


@pytest.mark.parametrize("fin,fout", PAIRS + [(768000, 8000), (1048575, 1)])
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
def test_tile_rule_fits_the_lds(probe, fin, fout, channels):
    """tile output frames span at most ceil((tile - 1) M / L) + K input frames, and cg channels of
    that fit the LDS beside the table when the table is kept there."""
    for Z in (16, 36):
        r = _ratio(probe, fin, fout, Z)
        if not r.rates_ok or r.k_over_limit:
            continue
        tile, cg, tab, lds = (ctypes.c_uint() for _ in range(4))
        probe.resample_probe_tile(fin, fout, Z, ref.ROLLOFF, channels, tile, cg, tab, lds)
        # a frame's staged channels are one LDS read of 1, 2 or 4 floats
        assert 1 <= tile.value <= 2048 and cg.value in (1, 2, 4) and cg.value <= {1: 1, 2: 2}.get(channels, 4)
        span = -((-(tile.value - 1) * r.M) // r.L) + r.K
        room = lds.value - ((r.L * r.K + 3) // 4 * 4 if tab.value else 0)  # the span is 16-byte aligned
        assert span * cg.value <= room, (fin, fout, Z, channels)
        assert tile.value % 512 == 0 or (tile.value < 512 and tile.value % 64 == 0) or tile.value < 64


def test_table_placement(probe):
    tile, cg, tab, lds = (ctypes.c_uint() for _ in range(4))
    probe.resample_probe_tile(48000, 16000, 16, ref.ROLLOFF, 2, tile, cg, tab, lds)
    assert tab.value == 1  # 115 floats
    probe.resample_probe_tile(44100, 16000, 16, ref.ROLLOFF, 2, tile, cg, tab, lds)
    # 16,800 floats: the flagship ratio keeps its table in LDS; 3,680 floats are left for two planes of
    # 1,840 frames, so ceil((tile - 1) 441 / 160) <= 1,735: 630 output frames, 512 as a multiple of the
    # workgroup's 512 lanes
    assert tab.value == 1 and tile.value == 512
    probe.resample_probe_tile(11025, 16000, 16, ref.ROLLOFF, 2, tile, cg, tab, lds)
    assert tab.value == 0  # 24,960 floats: read from global memory


# ---- the reference, pinned ---------------------------------------------------------------

@pytest.mark.parametrize("fin,fout", [(44100, 16000), (8000, 16000), (11025, 16000), (96000, 16000)])
def test_reference_keeps_a_constant(fin, fout):
    """Unit DC gain in every phase: a constant stream resamples to that constant wherever the
    filter's support lies inside the stream (float64 taps: the property of the formulas)."""
    L, M, W, K, h64 = ref.taps(fin, fout)
    n = 6 * W + 50
    x = np.full((n, 1), 0.375)
    y = ref.resample(x, 1, fin, fout, table=(L, M, W, K, h64), f32_taps=False)[:, 0]
    m = np.arange(y.size)
    q = (m * M) // L
    inside = (q - W >= 0) & (q + W <= n - 1)
    assert inside.sum() > 20 and not inside.all()
    assert np.abs(y[inside] - 0.375).max() <= 1e-12
    assert np.abs(y[~inside] - 0.375).max() > 1e-3  # no renormalisation at the edges
    assert y.size == ref.out_frames(n, fin, fout)


@pytest.mark.parametrize("fin,fout", [(44100, 16000), (22050, 48000)])
def test_reference_impulse_response(fin, fout):
    """A unit impulse at frame j yields h[r][j - q + W] at every m (0 outside the taps)."""
    L, M, W, K, h64 = ref.taps(fin, fout)
    h32 = h64.astype(np.float32).astype(np.float64)
    n, j = 4 * W + 31, 2 * W + 7
    x = np.zeros((n, 1))
    x[j] = 1.0
    y = ref.resample(x, 1, fin, fout)[:, 0]
    for m in range(y.size):
        q, r = (m * M) // L, (m * M) % L
        k = j - q + W
        assert y[m] == (h32[r][k] if 0 <= k < K else 0.0), m


def test_resampled_frames():
    L = _lib.load()
    for fin, fout in PAIRS:
        for n in (0, 1, 2, 440, 441, 442, 2 ** 40):
            want = ref.out_frames(n, fin, fout)
            assert L.zflac_hip_resampled_frames(n, fin, fout) == want, (n, fin, fout)
    assert ref.out_frames(441, 44100, 16000) == 160 and ref.out_frames(442, 44100, 16000) == 161
    assert L.zflac_hip_resampled_frames(1000, 0, 16000) == 0
    assert L.zflac_hip_resampled_frames(1000, 44100, 0) == 0
    assert L.zflac_hip_resampled_frames(1000, 16000, 16000) == 1000
