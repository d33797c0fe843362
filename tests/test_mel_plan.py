"""The feature plan's host half (zflac_amd/csrc/mel_plan.cpp) without a GPU: which arguments
zflac_hip_mel_create and zflac_hip_mel_run refuse, the tables against numpy doubles and their
padding, the frame count and the grid rule. tests/c/mel_probe.cpp is a program of its own linked
with mel_plan.cpp by plain g++ (that it links is the check that the planner is free of HIP); the
same cases run once more through a build of it with -fsanitize=address,undefined. Expected values
are arithmetic written here."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zflac_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "c", "_build")
E_OK, E_INVALID = 0, 14
F32, F16, BF16, I32 = 0, 1, 2, 3
TILE, FRAMES = 32, 128  # an MFMA tile's edge; feature frames per workgroup (common.h)
GRID_MAX = 0x7FFFFFFF
WAVE, DST = 0x7F4200000000, 0x7F5200000000  # made-up device addresses


def _build(name, extra):
    srcs = [os.path.join(ROOT, "tests", "c", "mel_probe.cpp"), os.path.join(CSRC, "mel_plan.cpp")]
    deps = srcs + [os.path.join(CSRC, "mel_plan.h"), os.path.join(CSRC, "common.h"),
                   os.path.join(ROOT, "include", "zflac_hip.h")]
    exe = os.path.join(BUILD, name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Werror", "-O1", "-g", *extra, "-I", CSRC, "-I",
                               os.path.join(ROOT, "include"), *srcs, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def probe():
    exe = _build("mel_probe", [])
    ran = []

    def run(*args):
        args = [str(a) for a in args]
        out = subprocess.run([exe, *args], capture_output=True, text=True, check=True).stdout
        ran.append((args, out))
        return out

    run.ran = ran
    return run


def create(probe, size=-1, dtype=F32, layout=0, scale=0, center=1, n=400, hop=160, bins=80, reserved=0, floor=None, flags=0):
    if floor is None:
        floor = 0 if scale == 0 else 1e-10
    return [int(v) for v in probe("create", size, dtype, layout, scale, center, n, hop, bins, reserved, floor, flags).split()]


def run_rc(probe, plan=1, wave=WAVE, rows=5, wave_frames=1000, row_stride=1000, first=0, frames=7, dst=DST,
           dst_bytes=None, n=400, hop=160, bins=80, dtype=F32):
    if dst_bytes is None:
        dst_bytes = rows * bins * frames * (4 if dtype == F32 else 2)
    return [int(v) for v in probe("run", plan, wave, rows, wave_frames, row_stride, first, frames, dst, dst_bytes, n, hop,
                                  bins, dtype).split()]


def m_tiles(bins):
    return next(q for q in (1, 2, 4, 8) if q * TILE >= bins)


def test_create_accepts_and_plans(probe):
    for n, hop, bins in ((400, 160, 80), (2, 1, 1), (2, 2, 256), (2048, 2048, 256), (2048, 1, 1), (16, 3, 5), (30, 7, 33)):
        K = n // 2 + 1
        bt = -(-K // TILE)
        assert create(probe, n=n, hop=hop, bins=bins) == [E_OK, K, bt, m_tiles(bins), bt * n * 64, bt * 16 * m_tiles(bins) * 64]
    for dtype in (F32, F16, BF16):
        for layout in (0, 1):
            for scale in (0, 1, 2):
                for center in (0, 1):
                    assert create(probe, dtype=dtype, layout=layout, scale=scale, center=center)[0] == E_OK


def test_create_refusals(probe):
    bad = [dict(flags=1), dict(flags=2), dict(flags=4), dict(flags=8), dict(flags=16), dict(flags=32),
           dict(size=0), dict(size=39), dict(size=41), dict(size=48),
           dict(dtype=I32), dict(dtype=4), dict(dtype=255), dict(layout=2), dict(scale=3), dict(center=2),
           dict(n=0), dict(n=1), dict(n=401), dict(n=2047), dict(n=2049), dict(n=2050, hop=1), dict(n=4096, hop=1),
           dict(hop=0), dict(hop=401), dict(n=2, hop=3), dict(n=2048, hop=2049),
           dict(bins=0), dict(bins=257), dict(reserved=1), dict(reserved=0x8000),
           dict(scale=0, floor=1e-10), dict(scale=0, floor="-1"), dict(scale=1, floor=0), dict(scale=2, floor=0),
           dict(scale=1, floor="-1e-10"), dict(scale=1, floor="inf"), dict(scale=2, floor="nan"), dict(scale=0, floor="nan")]
    for kw in bad:
        assert create(probe, **kw)[0] == E_INVALID, kw
    # the exact edges that pass
    for kw in (dict(n=2, hop=1), dict(n=2, hop=2), dict(n=2048), dict(n=2048, hop=2048), dict(hop=400), dict(hop=1),
               dict(bins=1), dict(bins=256), dict(scale=1, floor=1e-38), dict(scale=0, floor="-0.0")):
        assert create(probe, **kw)[0] == E_OK, kw


def test_run_refusals_and_the_grid(probe):
    assert run_rc(probe) == [E_OK, 1, 5]
    for kw in (dict(plan=0), dict(wave=0), dict(dst=0), dict(wave=WAVE + 1), dict(wave=WAVE + 2), dict(wave=WAVE + 3),
               dict(wave_frames=1001), dict(frames=0), dict(dst_bytes=5 * 80 * 7 * 4 - 1), dict(dtype=F16, dst_bytes=5 * 80 * 7 * 2 - 1),
               dict(rows=1 << 40, frames=1 << 40, dst_bytes=(1 << 64) - 1),      # the product overflows 64 bits
               dict(first=(1 << 63) // 160, dst_bytes=1 << 40),                    # (first + frames) * hop >= 2^63
               dict(first=(1 << 64) - 1, dst_bytes=1 << 40),
               dict(rows=GRID_MAX + 1, frames=1, bins=1, dst_bytes=1 << 40),       # the grid
               dict(rows=(GRID_MAX // 2) + 1, frames=129, bins=1, dst_bytes=1 << 50)):
        assert run_rc(probe, **kw)[0] == E_INVALID, kw
    assert run_rc(probe, wave=WAVE + 4)[0] == E_OK              # 4-byte alignment is all it asks
    assert run_rc(probe, dst=DST + 1)[0] == E_OK
    assert run_rc(probe, wave_frames=1000, row_stride=1000)[0] == E_OK
    assert run_rc(probe, wave_frames=0, row_stride=0)[0] == E_OK
    assert run_rc(probe, rows=0) == [E_OK, 1, 0]                # no workgroups: nothing to do ...
    assert run_rc(probe, rows=0, frames=0)[0] == E_INVALID      # ... but the other checks still apply
    assert run_rc(probe, first=(1 << 63) // 160 - 7, dst_bytes=1 << 40)[0] == E_OK
    for rows, frames in ((1, 1), (1, 127), (1, 128), (1, 129), (3, 256), (3, 257), (7, 100000)):
        tiles = -(-frames // FRAMES)
        assert run_rc(probe, rows=rows, frames=frames) == [E_OK, tiles, rows * tiles]
    assert run_rc(probe, rows=GRID_MAX, frames=128, bins=1, dst_bytes=1 << 50) == [E_OK, 1, GRID_MAX]
    assert run_rc(probe, rows=GRID_MAX // 2, frames=129, bins=1, dst_bytes=1 << 50) == [E_OK, 2, (GRID_MAX // 2) * 2]


def test_frames(probe):
    for n_fft, hop in ((400, 160), (16, 3), (2, 1), (2048, 2048)):
        for n in (0, 1, n_fft - 1, n_fft, n_fft + 1, 10 * hop - 1, 10 * hop, 10 * hop + 1, n_fft + 10 * hop - 1,
                  n_fft + 10 * hop, n_fft + 10 * hop + 1):
            assert int(probe("frames", n, n_fft, hop, 1)) == (n // hop + 1 if n else 0), (n_fft, hop, n)
            assert int(probe("frames", n, n_fft, hop, 0)) == ((n - n_fft) // hop + 1 if n >= n_fft else 0), (n_fft, hop, n)
    assert int(probe("frames", 100, 16, 0, 1)) == 0


def test_layout_of_the_descriptor(probe):
    from zflac_amd import _lib

    import ctypes
    D = _lib.zflac_mel_desc
    names = ["size", "dtype", "layout", "scale", "center", "n_fft", "hop", "n_bins", "reserved", "floor", "window", "filters"]
    assert [n for n, _ in D._fields_] == names
    want = [40, 0, 4, 5, 6, 7, 8, 10, 12, 14, 16, 24, 32]
    assert [int(v) for v in probe("layout").split()] == want
    assert [ctypes.sizeof(D)] + [getattr(D, n).offset for n in names] == want


def acc_row(r):
    """Row of a 32 x 32 f32 MFMA accumulator that register r holds in lanes 0..31 (lanes 32..63: + 4)."""
    return (r & 3) + 8 * (r >> 2)


def basis_index(N, n, k, im):
    """[bin tile][sample pair][re, im][sample of the pair][bin of the tile]"""
    return ((((k // TILE) * (N // 2) + n // 2) * 2 + im) * 2 + n % 2) * TILE + k % TILE


def filter_index(bins, m, k):
    """[bin tile][register][filter tile][lane]: lane = 32 h + filter of the tile, bin row = acc_row(r) + 4 h"""
    row = k % TILE
    r, h = next((r, h) for r in range(16) for h in (0, 1) if acc_row(r) + 4 * h == row)
    return (((k // TILE) * 16 + r) * m_tiles(bins) + m // TILE) * 64 + 32 * h + m % TILE


def test_index_rule(probe):
    N, bins = 30, 33
    K = N // 2 + 1
    got = [int(v) for v in probe("index", N, bins).split()]
    want = [basis_index(N, n, k, im) for im in (0, 1) for n in range(N) for k in range(K)]
    want += [filter_index(bins, m, k) for m in range(bins) for k in range(K)]
    assert got == want
    assert len(set(want[:2 * N * K])) == 2 * N * K and len(set(want[2 * N * K:])) == bins * K  # no two share a place


@pytest.mark.parametrize("N,hop,bins", [(2, 1, 2), (16, 3, 5), (30, 7, 33), (400, 160, 80), (2048, 2048, 256)])
def test_tables(probe, tmp_path, N, hop, bins):
    K = N // 2 + 1
    bt, q = -(-K // TILE), m_tiles(bins)
    path = tmp_path / "tables.f32"
    assert [int(v) for v in probe("tables", N, hop, bins, path).split()] == [E_OK, bt * N * 64, bt * 16 * q * 64]
    t = np.fromfile(path, dtype=np.float32)
    basis, filt = t[:bt * N * 64], t[bt * N * 64:]
    assert filt.size == bt * 16 * q * 64
    n, k = np.arange(N, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    w = (np.float32(0.25) + ((np.arange(N) * 37) % 101).astype(np.float32) / np.float32(128.0)).astype(np.float64)
    ang = 2.0 * np.pi * ((n * k) % N).astype(np.float64) / N
    want = {0: w[:, None] * np.cos(ang), 1: -w[:, None] * np.sin(ang)}
    used = np.zeros(basis.size, dtype=bool)
    for im in (0, 1):
        at = (((((k // TILE) * (N // 2) + n // 2) * 2 + im) * 2 + n % 2) * TILE + k % TILE)
        used[at.ravel()] = True
        got = basis[at].astype(np.float64)
        # one f32 rounding of the double; where the double is a rounding residue of 0 (1e-16), that much
        assert np.all(np.abs(got - want[im]) <= 2.0 ** -24 * np.abs(want[im]) + 1e-15), (N, im)
    assert not basis[~used].any()                       # bins K .. 32 bt - 1: zero
    assert used.sum() == 2 * N * K
    s = basis[(((((k // TILE) * (N // 2) + n // 2) * 2 + 1) * 2 + n % 2) * TILE + k % TILE)]
    assert not s[:, 0].any() and not s[:, N // 2].any()  # exactly 0, not sin(pi) of a double
    m = np.arange(bins, dtype=np.int64)[:, None]
    fwant = (((m * 131 + k * 7) % 97).astype(np.float32) / np.float32(64.0) - np.float32(0.5))
    row = k % TILE
    r, h = (row & 3) + 4 * (row >> 3), (row >> 2) & 1
    assert np.array_equal((r & 3) + 8 * (r >> 2) + 4 * h, row)
    at = (((k // TILE) * 16 + r) * q + m // TILE) * 64 + 32 * h + m % TILE
    assert np.array_equal(filt[at].view(np.uint32), fwant.view(np.uint32))
    fused = np.zeros(filt.size, dtype=bool)
    fused[at.ravel()] = True
    assert fused.sum() == bins * K and not filt[~fused].any()


def test_sanitized_probe_gives_the_same_answers(probe, tmp_path):
    """Every case the tests above ran, through the -fsanitize=address,undefined build."""
    exe = _build("mel_probe_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    cases = list(probe.ran)
    if not any(a[0] == "tables" for a, _ in cases):  # (run alone)
        cases += [(["tables", "30", "7", "33", str(tmp_path / "t.f32")], "0 %d %d\n" % (30 * 64, 16 * 2 * 64)),
                  (["create", "-1", "0", "0", "0", "1", "2048", "2048", "256", "0", "0", "0"], None),
                  (["create", "-1", "0", "0", "0", "1", "400", "160", "80", "0", "0", "16"], None),
                  (["run", "1", str(WAVE), "5", "1000", "1000", "0", "7", str(DST), "11200", "400", "160", "80", "0"], None)]
    assert cases
    for args, out in cases:
        if args[0] == "tables":
            args = args[:-1] + [str(tmp_path / "san.f32")]
        p = subprocess.run([exe, *args], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.stderr[-2000:])
        assert out is None or p.stdout == out, args
