"""The dense exports' host planning (zflac_amd/csrc/export_plan.cpp: which error an argument draws,
which path a row takes, the grid, the coefficient table, the row records) without a GPU. The
planner is built here with plain g++: that it compiles is the check that it is free of HIP.
Expected values are arithmetic written here, tests/resample_ref.py and the tile rule as
tests/test_resample_plan.py pins it; the destination is a made-up address."""
from __future__ import annotations

import ctypes
import math
import os
import struct
import subprocess

import pytest

from zflac_amd import _lib

from . import resample_ref as ref
from .test_resample_plan import probe as resample_probe  # noqa: F401  (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zflac_amd", "csrc")

E_OK, E_INVALID = 0, 14
EXPORT_TILE = 4096  # 256 lanes x 16 frames, common.h
GRID_MAX = 0x7FFFFFFF
DST = 0x7F4200000000  # a made-up device address, 16-byte aligned
TAPS, TAPS_STEP = 0x7F5000000000, 0x100000  # made-up tap table addresses: TAPS + k * TAPS_STEP
SENTINEL = 0xA5A5A5A5A5A5A5A5
S8, S16, S32 = 0, 1, 2
U64 = ctypes.c_uint64


class Stream(ctypes.Structure):
    _fields_ = [("samples", U64), ("n_frames", U64), ("rate", ctypes.c_uint), ("nch", ctypes.c_ubyte),
                ("kind", ctypes.c_ubyte)]


class Plan(ctypes.Structure):
    _fields_ = [("C", U64), ("T", U64), ("tiles", U64), ("need_floats", U64), ("vec", ctypes.c_uint),
                ("mixed", ctypes.c_uint), ("table_len", ctypes.c_uint), ("n_needs", ctypes.c_uint),
                ("at", ctypes.c_ushort * 9), ("table", ctypes.c_float * 289)] + [
        (f"need_{k}", ctypes.c_uint * 8) for k in ("fin", "L", "M", "W", "K")]


class ExportRow(ctypes.Structure):  # common.h: the 32-byte record of k_export
    _fields_ = [("src", U64), ("n_frames", U64), ("start", U64), ("nch", ctypes.c_ubyte), ("kind", ctypes.c_ubyte),
                ("mix", ctypes.c_ushort), ("pad_", ctypes.c_ubyte * 4)]


class ResampleRow(ctypes.Structure):  # common.h: the 72-byte record of k_resample
    _fields_ = [("e", ExportRow), ("taps", U64), ("n_out", U64), ("L", ctypes.c_uint), ("M", ctypes.c_uint),
                ("W", ctypes.c_uint), ("K", ctypes.c_uint), ("tile", ctypes.c_uint), ("cg", ctypes.c_ubyte),
                ("tab_lds", ctypes.c_ubyte), ("pad_", ctypes.c_ubyte * 2)]


assert ctypes.sizeof(ExportRow) == 32 and ctypes.sizeof(ResampleRow) == 72


@pytest.fixture(scope="module")
def planner():
    srcs = [os.path.join(ROOT, "tests", "c", "export_plan_probe.cpp"), os.path.join(CSRC, "export_plan.cpp"),
            os.path.join(CSRC, "resample_plan.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("export_plan.h", "resample_plan.h", "common.h")] + [
        os.path.join(ROOT, "include", "zflac_hip.h")]
    lib = os.path.join(ROOT, "tests", "c", "_build", "libexport_plan_probe.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Werror", "-O2", "-shared", "-fPIC", "-I", CSRC, "-I",
                               os.path.join(ROOT, "include"), *srcs, "-o", lib])
    dll = ctypes.CDLL(lib)
    dll.export_probe.argtypes = [ctypes.POINTER(Stream), ctypes.c_size_t, ctypes.POINTER(_lib.zflac_export_desc),
                                 ctypes.POINTER(_lib.zflac_resample_desc), ctypes.POINTER(_lib.zflac_mix_desc), U64, U64,
                                 ctypes.POINTER(U64), ctypes.POINTER(Plan), ctypes.POINTER(ctypes.c_int),
                                 ctypes.POINTER(U64), ctypes.c_void_p, U64, U64]
    dll.export_probe.restype = ctypes.c_int
    return dll


def stream(nch=2, frames=5000, rate=44100, kind=S16, samples=0x7F1000000000):
    return Stream(samples, frames, rate, nch, kind)


NO_SAMPLES = Stream(0, 0, 0, 0, S16)  # an error, zero channels, nothing decoded: one state
ESZ = {_lib.EXPORT_F32: 4, _lib.EXPORT_F16: 2, _lib.EXPORT_BF16: 2, _lib.EXPORT_I32: 4}


def plain_desc(C=2, T=1000, dtype=_lib.EXPORT_F32, layout=_lib.LAYOUT_PLANAR, starts=None):
    return _lib.zflac_export_desc(ctypes.sizeof(_lib.zflac_export_desc), dtype, layout, C, T, starts)


def resample_desc(C=2, T=1000, dtype=_lib.EXPORT_F32, layout=_lib.LAYOUT_PLANAR, starts=None, rate=16000, zeros=ref.ZEROS,
                  reserved=0, rolloff=ref.ROLLOFF, beta=ref.BETA):
    return _lib.zflac_resample_desc(ctypes.sizeof(_lib.zflac_resample_desc), dtype, layout, C, T, starts, rate, zeros,
                                    reserved, rolloff, beta)


def mix_desc(matrices=None, C=2):
    """zflac_mix_desc with matrix[n - 1] = matrices[n] (a flat list of C x n floats); the arrays are
    kept alive on the descriptor."""
    m = _lib.zflac_mix_desc(ctypes.sizeof(_lib.zflac_mix_desc), 0)
    m._keep = []
    for n, coef in (matrices or {}).items():
        assert len(coef) == C * n
        arr = (ctypes.c_float * len(coef))(*coef)
        m._keep.append(arr)
        m.matrix[n - 1] = ctypes.cast(arr, ctypes.POINTER(ctypes.c_float))
    return m


class Result:
    pass


def run(planner, streams, desc, mix=None, dst=DST, dst_bytes=None, rows=False):
    """One planning call. dst_bytes: exactly what the call needs unless given."""
    n = len(streams)
    resampled = isinstance(desc, _lib.zflac_resample_desc)
    if dst_bytes is None:
        dst_bytes = n * desc.channels * desc.frames * ESZ.get(desc.dtype, 4)
    r = Result()
    sv = (Stream * max(n, 1))(*streams)
    r.valid = (U64 * max(n, 1))(*[SENTINEL] * max(n, 1))
    r.plan = Plan()
    ratio_of = (ctypes.c_int * max(n, 1))()
    n_out = (U64 * max(n, 1))()
    rec = ((ResampleRow if resampled else ExportRow) * max(n, 1))()
    r.rc = planner.export_probe(sv, n, None if resampled else ctypes.byref(desc), ctypes.byref(desc) if resampled else None,
                                ctypes.byref(mix) if mix is not None else None, dst, dst_bytes, r.valid, ctypes.byref(r.plan),
                                ratio_of, n_out, ctypes.cast(rec, ctypes.c_void_p) if rows else None, TAPS, TAPS_STEP)
    r.valid = list(r.valid)[:n]
    r.ratio_of, r.n_out, r.rows = list(ratio_of)[:n], list(n_out)[:n], list(rec)[:n]
    return r


def tile_of(resample_probe, fin, fout, channels, Z=ref.ZEROS):
    """(tile, cg, tab_lds) of the kernel's tile rule (pinned by tests/test_resample_plan.py)"""
    tile, cg, tab, lds = (ctypes.c_uint() for _ in range(4))
    resample_probe.resample_probe_tile(fin, fout, Z, ref.ROLLOFF, channels, tile, cg, tab, lds)
    return tile.value, cg.value, tab.value


# ---- refusals -----------------------------------------------------------------------------

STREAMS3 = [stream(2, 5000, 44100), stream(1, 3000, 16000), NO_SAMPLES]
NAN, INF = float("nan"), float("inf")


def _set(**kw):
    def f(call):
        for k, v in kw.items():
            setattr(call["desc"], k, v)
    return f


def _key(**kw):
    return lambda call: call.update(kw)


def _one_short(call):
    d = call["desc"]
    call["dst_bytes"] = 3 * d.channels * d.frames * ESZ[d.dtype] - ESZ[d.dtype]


def _mix(matrices=None, C=2, **fields):
    def f(call):
        call["desc"].channels = C
        call["mix"] = mix_desc(matrices, C)
        for k, v in fields.items():
            setattr(call["mix"], k, v)
    return f


def _coef(x, n=2):
    """a stereo (or n-channel) matrix for C = 2 with one coefficient x"""
    return _mix({n: [0.5] * (2 * n - 1) + [x]})


# (id, which calls, the offending change, the same change repaired)
BOTH, PLAIN, RESAMPLED = ("plain", "resampled"), ("plain",), ("resampled",)
REFUSALS = [
    ("size", BOTH, lambda c: setattr(c["desc"], "size", c["desc"].size + 1), lambda c: None),
    ("dtype_4", PLAIN, _set(dtype=4), _set(dtype=_lib.EXPORT_I32)),
    ("dtype_i32", RESAMPLED, _set(dtype=_lib.EXPORT_I32), _set(dtype=_lib.EXPORT_BF16)),
    ("layout_2", BOTH, _set(layout=2), _set(layout=_lib.LAYOUT_INTERLEAVED)),
    ("channels_0", BOTH, _set(channels=0), _set(channels=1)),
    ("frames_0", BOTH, _set(frames=0), _set(frames=1)),
    ("null_dst", BOTH, _key(dst=0), _key(dst=DST)),
    ("dst_one_element_short", BOTH, _one_short, lambda c: None),
    ("reserved", RESAMPLED, _set(reserved=1), _set(reserved=0)),
    ("rate_0", RESAMPLED, _set(sample_rate=0), _set(sample_rate=16000)),
    ("rate_2p20", RESAMPLED, _set(sample_rate=1048576), _set(sample_rate=1048575)),
    ("zeros_0", RESAMPLED, _set(zeros=0), _set(zeros=1)),
    ("rolloff_0", RESAMPLED, _set(rolloff=0.0), _set(rolloff=1.0)),
    ("rolloff_1_5", RESAMPLED, _set(rolloff=1.5), _set(rolloff=1.0)),
    ("beta_neg", RESAMPLED, _set(beta=-1.0), _set(beta=0.0)),
    ("mix_size", BOTH, _mix(size=71), _mix(size=72)),
    ("mix_reserved", BOTH, _mix(reserved=1), _mix(reserved=0)),
    ("mix_i32", PLAIN, lambda c: (_set(dtype=_lib.EXPORT_I32)(c), _coef(0.5)(c)), _coef(0.5)),
    ("mix_c9", BOTH, _mix({1: [0.5] * 9}, C=9), _mix({1: [0.5] * 8}, C=8)),
    ("coef_nan", BOTH, _coef(NAN), _coef(1.0)),
    ("coef_inf", BOTH, _coef(INF), _coef(1.0)),
    ("coef_2p-65", BOTH, _coef(2.0 ** -65), _coef(2.0 ** -64)),
    ("coef_2p65", BOTH, _coef(2.0 ** 65), _coef(-2.0 ** 64)),
    # no stream of the batch has 8 channels: its matrix is checked all the same
    ("coef_of_absent_channel_count", BOTH, _coef(-2.0 ** 65, n=8), _coef(-0.0, n=8)),
]


@pytest.mark.parametrize("which,offend,repair", [(w, r[2], r[3]) for r in REFUSALS for w in r[1]],
                         ids=[f"{r[0]}-{w}" for r in REFUSALS for w in r[1]])
def test_refusals_write_nothing(planner, which, offend, repair):
    for change, want in ((offend, E_INVALID), (repair, E_OK)):
        call = dict(desc=plain_desc() if which == "plain" else resample_desc(), mix=None, dst=DST, dst_bytes=None)
        change(call)
        r = run(planner, STREAMS3, call["desc"], call["mix"], call["dst"], call["dst_bytes"])
        assert r.rc == want
        if want == E_INVALID:
            assert r.valid == [SENTINEL] * 3
        else:
            assert SENTINEL not in r.valid and r.valid[2] == 0


def test_all_null_descriptor_is_the_unmixed_call(planner):
    # C = 9 and, in the plain call, I32: refused only together with a matrix
    for desc in (plain_desc(C=9), plain_desc(dtype=_lib.EXPORT_I32), plain_desc(C=9, dtype=_lib.EXPORT_I32),
                 resample_desc(C=9)):
        r = run(planner, STREAMS3, desc, mix_desc())
        assert r.rc == E_OK and r.plan.mixed == 0 and r.plan.table_len == 0 and list(r.plan.at) == [0] * 9


def test_tap_limit(planner):
    """768 kHz to 16 kHz at zeros 64: W = ceil(64 * 48 / 0.85) = 3,615, K = 7,231 > 4,096."""
    assert ref.ratio(768000, 16000, 64)[3] == 7231
    s = [stream(1, 100000, 768000)]
    r = run(planner, s, resample_desc(zeros=64))
    assert r.rc == E_INVALID and r.valid == [SENTINEL]
    assert ref.ratio(768000, 16000, 36)[3] == 4067
    assert run(planner, s, resample_desc(zeros=36)).rc == E_OK


def test_table_budget_is_per_call(planner):
    """Two source rates whose tables each fit 4 Mi floats and together do not."""
    fout, rates = 1048575, (11 * 1024, 11 * 2048)
    floats = []
    for fin in rates:
        L, M, W, K, _ = ref.ratio(fin, fout)
        assert (L, K) == (fout // 11, 39) and L == fout // math.gcd(fin, fout)
        floats.append(L * K)
    assert max(floats) < 4 << 20 < sum(floats)
    r = run(planner, [stream(1, 1000, f) for f in rates], resample_desc(rate=fout))
    assert r.rc == E_INVALID and r.valid == [SENTINEL] * 2
    for fin, fl in zip(rates, floats):  # either alone, twice: one table
        r = run(planner, [stream(1, 1000, fin)] * 2, resample_desc(rate=fout))
        assert r.rc == E_OK and r.plan.n_needs == 1 and r.plan.need_floats == fl and r.ratio_of == [0, 0]


# ---- the grid limit, at its edge ----------------------------------------------------------------

def test_grid_limit_plain(planner):
    two = [stream(1, 10, 44100)] * 2
    T = 1 << 42  # 2 rows x 2^30 tiles = 2^31
    assert 2 * (T // EXPORT_TILE) == GRID_MAX + 1
    r = run(planner, two, plain_desc(C=1, T=T))
    assert r.rc == E_INVALID and r.valid == [SENTINEL] * 2
    T -= EXPORT_TILE
    r = run(planner, two, plain_desc(C=1, T=T))
    assert r.rc == E_OK and 2 * r.plan.tiles == GRID_MAX - 1 and r.valid == [10, 10]


def test_grid_limit_of_a_filtered_row(planner, resample_probe):
    one = [stream(2, 5000, 44100)]
    tile = tile_of(resample_probe, 44100, 16000, 2)[0]
    assert tile == 512
    T = 1 << 40
    assert T // tile == GRID_MAX + 1 and -(-T // EXPORT_TILE) <= GRID_MAX
    r = run(planner, one, resample_desc(T=T))
    assert r.rc == E_INVALID and r.valid == [SENTINEL]
    r = run(planner, one, plain_desc(T=T))
    assert r.rc == E_OK and r.plan.tiles == T // EXPORT_TILE
    T -= tile
    r = run(planner, one, resample_desc(T=T))
    assert r.rc == E_OK and r.plan.tiles == GRID_MAX and r.valid == [ref.out_frames(5000, 44100, 16000)]
    assert run(planner, one, plain_desc(T=T)).rc == E_OK


# ---- the records --------------------------------------------------------------------------------

FOUT, C_REC, T_REC = 16000, 2, 1100
A_FRAMES = 2823
A_OUT = 1025  # ceil(2823 * 160 / 441)
SRC = [0x7F1000000000 + 0x10000 * i for i in range(7)]
VIEWS = [
    stream(2, A_FRAMES, 44100, S16, SRC[0]),  # (a) filtered
    stream(1, 3000, FOUT, S32, SRC[1]),       # (b) already at the target rate
    Stream(0, 0, 0, 0, S8),                   # (c) in error
    stream(2, 700, 0, S16, SRC[3]),           # (d) OK, rate 0
    stream(1, 900, 8000, S8, SRC[4]),         # (e) upsampled
    stream(2, A_FRAMES, 44100, S16, SRC[5]),  # (f) as (a), its window at the resampled stream's end
    stream(1, 5000, 11025, S16, SRC[6]),      # (g) its table stays in global memory
]
STARTS = [0, 2500, 0, 10, 3, A_OUT, 40]
RATIO_OF = [0, -1, -1, -1, 1, 0, 2]  # in order of first appearance: 44,100, 8,000, 11,025 Hz


def expected_resample_rows(resample_probe, starts, mix_at=None, C=C_REC):
    """The seven 72-byte records and valid lengths, from the rules of include/zflac_hip.h and common.h."""
    rows, valid, tiles = [], [], -(-T_REC // EXPORT_TILE)
    for v, start, k in zip(VIEWS, starts, RATIO_OF):
        r = ResampleRow()
        r.e.start, r.e.kind = start, v.kind
        if v.samples:
            r.e.nch, r.e.n_frames = v.nch, v.n_frames
        r.e.mix = (mix_at or {}).get(v.nch, 0) if v.samples else 0
        if k < 0:  # k_export's paths, counted in the stream's own frames
            n_out = v.n_frames if v.rate == FOUT else 0
            if start < n_out:
                r.e.src = v.samples
        else:
            L, M, W, K, _ = ref.ratio(v.rate, FOUT)
            n_out = r.n_out = ref.out_frames(v.n_frames, v.rate, FOUT)
            staged = C if r.e.mix else min(v.nch, C)
            tile, cg, tab = tile_of(resample_probe, v.rate, FOUT, staged)
            tiles = max(tiles, -(-T_REC // tile))
            if start < n_out:
                r.e.src, r.taps = v.samples, TAPS + k * TAPS_STEP
                r.L, r.M, r.W, r.K, r.tile, r.cg, r.tab_lds = L, M, W, K, tile, cg, tab
        rows.append(r)
        valid.append(min(max(n_out - start, 0), T_REC))
    return rows, valid, tiles


def test_records_of_the_resampled_call(planner, resample_probe):
    assert ref.out_frames(A_FRAMES, 44100, FOUT) == A_OUT
    for starts in (STARTS, STARTS[:5] + [A_OUT - 1] + STARTS[6:]):
        d = resample_desc(C=C_REC, T=T_REC, rate=FOUT, starts=(U64 * 7)(*starts))
        r = run(planner, VIEWS, d, rows=True)
        want, valid, tiles = expected_resample_rows(resample_probe, starts)
        assert r.rc == E_OK and r.ratio_of == RATIO_OF and r.valid == valid
        for i, (got, exp) in enumerate(zip(r.rows, want)):
            assert bytes(got) == bytes(exp), f"row {i} with starts {starts}"
        p = r.plan
        assert (p.C, p.T, p.tiles, p.vec, p.mixed, p.n_needs) == (C_REC, T_REC, tiles, 1, 0, 3)  # 4,400-byte rows: 275 x 16
        assert list(p.need_fin)[:3] == [44100, 8000, 11025]
        for k, fin in enumerate((44100, 8000, 11025)):
            assert (p.need_L[k], p.need_M[k], p.need_W[k], p.need_K[k]) == ref.ratio(fin, FOUT)[:4]
        assert p.need_floats == sum(ref.ratio(f, FOUT)[0] * ref.ratio(f, FOUT)[3] for f in (44100, 8000, 11025))
        # what the figures above amount to
        a, f, g = r.rows[0], r.rows[5], r.rows[6]
        assert (a.n_out, a.tile, a.cg, a.tab_lds, a.taps) == (A_OUT, 512, 2, 1, TAPS)
        assert tiles == 3 and g.tab_lds == 0 and g.taps == TAPS + 2 * TAPS_STEP
        assert r.rows[1].taps == 0 and r.rows[1].e.src == SRC[1] and r.valid[1] == 500
        assert (r.rows[2].e.src, r.valid[2], r.rows[3].e.src, r.valid[3]) == (0, 0, 0, 0)
        assert r.rows[4].L == 2 and r.rows[4].M == 1
        if starts[5] == A_OUT:
            assert (f.e.src, f.taps, f.tile, r.valid[5]) == (0, 0, 0, 0)
        else:
            assert (f.e.src, f.taps, f.tile, r.valid[5]) == (SRC[5], TAPS, 512, 1)


def test_records_of_the_plain_call(planner):
    starts = [0, 2500, 0, 10, 3, 2822, 40]
    d = plain_desc(C=C_REC, T=T_REC, starts=(U64 * 7)(*starts))
    r = run(planner, VIEWS, d, rows=True)
    assert r.rc == E_OK and r.plan.tiles == 1 and r.plan.n_needs == 0
    for i, (v, start, got) in enumerate(zip(VIEWS, starts, r.rows)):
        exp = ExportRow()
        exp.start, exp.kind = start, v.kind
        if v.samples:
            exp.nch, exp.n_frames = v.nch, v.n_frames
            exp.src = v.samples if start < v.n_frames else 0
        assert bytes(got) == bytes(exp), i
        assert r.valid[i] == min(max(v.n_frames - start, 0), T_REC)
    # the rows the resampled call does not filter are these records (a rate of 0 aside: zeroed there)
    rs = run(planner, VIEWS, resample_desc(C=C_REC, T=T_REC, rate=FOUT, starts=(U64 * 7)(*starts)), rows=True)
    assert rs.rc == E_OK
    for i in (1, 2):
        assert bytes(rs.rows[i].e) == bytes(r.rows[i]) and bytes(rs.rows[i])[32:] == bytes(40)
    assert r.rows[3].src == SRC[3] and rs.rows[3].e.src == 0


# ---- the coefficient table -----------------------------------------------------------------------

def bits(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


def test_mix_table_and_rows(planner, resample_probe):
    C = 4
    m1 = [1.0, -0.0, 0.25, -2.0 ** 64]
    m6 = [((c * 6 + j) % 11 + 1) * (-0.125 if j & 1 else 0.125) for c in range(C) for j in range(6)]
    m6[7] = -0.0
    m6[13] = 2.0 ** -64
    mix = mix_desc({1: m1, 6: m6}, C)
    views = [stream(1, 5000, 44100), NO_SAMPLES, stream(6, 800, FOUT), stream(2, 5000, 44100)]
    r = run(planner, views, resample_desc(C=C, T=T_REC), mix, rows=True)
    assert r.rc == E_OK and r.plan.mixed == 1
    assert list(r.plan.at) == [0, 1, 0, 0, 0, 0, 1 + C * 1, 0, 0] and r.plan.table_len == 1 + C * 1 + C * 6
    table = [bits(x) for x in list(r.plan.table)[:r.plan.table_len]]
    assert table == [bits(0.0)] + [bits(0.0 if x == 0 else x) for x in m1 + m6]  # row-major, -0.0 as +0.0
    assert table[2] == 0 and table[5 + 7] == 0 and table[4] == bits(-2.0 ** 64)
    mono, err, six, stereo = r.rows
    assert (mono.e.mix, err.e.mix, six.e.mix, stereo.e.mix) == (1, 0, 5, 0)
    # mixed first, a mono stream is staged as C channels; the unmixed stereo stream as its own two
    assert (mono.tile, mono.cg, mono.tab_lds) == tile_of(resample_probe, 44100, FOUT, C)
    # by hand: the 16,800-float table in LDS leaves 3,680 floats, 920 frames of 4 channels, 815 past the
    # K = 105 taps: floor(815 * 160 / 441) + 1 = 296 output frames, 256 in whole waves. One channel has
    # 3,575 frames past the taps: 1,298 output frames, 1,024 as a multiple of the 512 lanes.
    assert (mono.tile, mono.cg, mono.tab_lds) == (256, 4, 1)
    assert (stereo.tile, stereo.cg, stereo.tab_lds) == tile_of(resample_probe, 44100, FOUT, 2)
    assert r.plan.tiles == max(-(-T_REC // mono.tile), -(-T_REC // stereo.tile), 1) and r.ratio_of == [0, -1, -1, 0]
    plain = run(planner, views, resample_desc(C=C, T=T_REC), rows=True)
    assert plain.rc == E_OK and plain.plan.mixed == 0 and [x.e.mix for x in plain.rows] == [0] * 4
    assert (plain.rows[0].tile, plain.rows[0].cg, plain.rows[0].tab_lds) == tile_of(resample_probe, 44100, FOUT, 1)
    assert (plain.rows[0].tile, plain.rows[0].cg, plain.rows[0].tab_lds) == (1024, 1, 1)
    assert tile_of(resample_probe, 44100, FOUT, 1) != tile_of(resample_probe, 44100, FOUT, C)
    # the plain call lays the same table out and marks the same rows
    r = run(planner, views, plain_desc(C=C, T=T_REC), mix, rows=True)
    assert r.rc == E_OK and [bits(x) for x in list(r.plan.table)[:r.plan.table_len]] == table
    assert [x.mix for x in r.rows] == [1, 0, 5, 0]


# ---- the 16-byte store paths -----------------------------------------------------------------------

def test_vec(planner):
    s = [stream(1, 5000, 44100)]
    il, f16 = _lib.LAYOUT_INTERLEAVED, _lib.EXPORT_F16
    assert run(planner, s, plain_desc(C=1, T=1104, dtype=f16, layout=il)).plan.vec == 1  # 2,208 = 138 x 16
    assert run(planner, s, plain_desc(C=1, T=1104, dtype=f16, layout=il), dst=DST + 4).plan.vec == 0
    assert run(planner, s, plain_desc(C=1, T=1101, dtype=f16, layout=il)).plan.vec == 0  # 2,202-byte rows
    assert run(planner, s, plain_desc(C=2, T=1000)).plan.vec == 1  # planar f32: 4,000-byte rows
    assert run(planner, s, plain_desc(C=2, T=1001)).plan.vec == 0
    assert run(planner, s, plain_desc(C=4, T=1001, layout=il)).plan.vec == 1  # interleaved: T x C x 4 bytes
    assert run(planner, s, resample_desc(C=2, T=1000)).plan.vec == 1
    assert run(planner, s, resample_desc(C=2, T=1000), dst=DST + 4).plan.vec == 0
