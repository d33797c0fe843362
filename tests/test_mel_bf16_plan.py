"""The split-bf16 half of the feature plan's host side (zflac_amd/csrc/mel_plan.cpp:
mel_plan_create_ex, mel_bf16_tables, mel_bf16_basis_index) without a GPU: the math argument and
where it is checked, the F32 plan through the new entry, and the piece table against the
round-to-nearest-even chain written here on the bits. tests/c/mel_bf16_probe.cpp is a program of its
own linked with mel_plan.cpp by plain g++; the same cases run once more through a build of it with
-fsanitize=address,undefined."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zflac_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "c", "_build")
E_OK, E_INVALID = 0, 14
F32, X6, X3 = 0, 1, 2
TILE, KB, GROUP = 32, 16, 2  # an MFMA tile's edge; samples per bf16 MFMA; bin tiles per group (common.h)
PIECES = {X6: 3, X3: 2}


def _build(name, extra):
    srcs = [os.path.join(ROOT, "tests", "c", "mel_bf16_probe.cpp"), os.path.join(CSRC, "mel_plan.cpp")]
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
    exe = _build("mel_bf16_probe", [])
    ran = []

    def run(*args):
        args = [str(a) for a in args]
        out = subprocess.run([exe, *args], capture_output=True, text=True, check=True).stdout
        ran.append((args, out))
        return out

    run.ran = ran
    return run


def create(probe, math, size=-1, dtype=0, layout=0, scale=0, center=1, n=400, hop=160, bins=80, reserved=0, floor=None,
           flags=0):
    if floor is None:
        floor = 0 if scale == 0 else 1e-10
    return [int(v) for v in probe("create", math, size, dtype, layout, scale, center, n, hop, bins, reserved, floor,
                                  flags).split()]


def test_known_and_unknown_math(probe):
    for n in (2, 16, 30, 400, 2048):
        bt, kbs = -(-(n // 2 + 1) // TILE), -(-n // KB)
        assert create(probe, F32, n=n, hop=1) == [E_OK, F32, 0, 0, 0]
        assert create(probe, X6, n=n, hop=1) == [E_OK, X6, kbs, 3, bt * kbs * 2 * 3 * 512]
        assert create(probe, X3, n=n, hop=1) == [E_OK, X3, kbs, 2, bt * kbs * 2 * 2 * 512]
    for math in (3, 4, 255, 256, 0x80000000, 0xFFFFFFFF):
        assert create(probe, math) == [E_INVALID, 0, 0, 0, 0], math


# one bad descriptor per rule of mel_plan_create, in its documented order
EARLIER_RULES = [dict(flags=1), dict(flags=2), dict(size=39), dict(dtype=3), dict(layout=2), dict(scale=3), dict(center=2),
                 dict(n=401), dict(hop=0), dict(bins=257), dict(reserved=1), dict(scale=1, floor=0), dict(flags=4),
                 dict(flags=8), dict(flags=16), dict(flags=32)]


@pytest.mark.parametrize("kw", EARLIER_RULES, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_math_is_checked_after_the_descriptor(probe, kw):
    """A bad descriptor answers with a bad math as it does with a good one: refused, the plan
    untouched, and nothing of the descriptor read beyond what refused it (NULL tables included)."""
    alone = create(probe, F32, **kw)
    assert alone == [E_INVALID, 0, 0, 0, 0]
    for math in (X6, 3, 0xFFFFFFFF):
        assert create(probe, math, **kw) == alone, (kw, math)


def piece_index(N, n_pieces, k, n, im, piece):
    """[group][sample block][bin tile of the group][re, im][piece][lane][j], written from mel_plan.h's words:
    lane = 32 (half of the block) + bin of the tile, j = sample of the half. numpy arrays or ints."""
    bt, kbs = -(-(N // 2 + 1) // TILE), -(-N // KB)
    b = k // TILE
    g, bi = b // GROUP, b % GROUP
    tg = np.minimum(GROUP, bt - GROUP * g)
    operand = ((g * GROUP * kbs + (n // KB) * tg + bi) * 2 + im) * n_pieces + piece
    lane = 32 * ((n % KB) // 8) + k % TILE
    return (operand * 64 + lane) * 8 + n % 8


@pytest.mark.parametrize("math,N,bins", [(X6, 2, 2), (X6, 16, 5), (X6, 30, 33), (X3, 30, 33), (X6, 400, 80)])
def test_index_rule_and_lane_map(probe, math, N, bins):
    P = PIECES[math]
    bt, kbs = -(-(N // 2 + 1) // TILE), -(-N // KB)
    got = np.array(probe("index", math, N, bins).split(), dtype=np.int64).reshape(2, P, kbs * KB, bt * TILE)
    im, piece, n, k = np.meshgrid(np.arange(2), np.arange(P), np.arange(kbs * KB), np.arange(bt * TILE), indexing="ij")
    assert np.array_equal(got, piece_index(N, P, k, n, im, piece))
    # every place of the table is taken exactly once
    assert np.array_equal(np.sort(got.ravel()), np.arange(bt * kbs * 2 * P * 512))
    # the lane map of v_mfma_f32_32x32x16_bf16's A operand: lane l holds A[row l & 31][k = 8 (l >> 5) + j]
    lane, j = (got // 8) % 64, got % 8
    assert np.array_equal(lane & 31, k % TILE) and np.array_equal(8 * (lane >> 5) + j, n % KB)
    # one operand (bin tile, re/im, piece, sample block) is 512 consecutive entries, a block of a group contiguous
    operand = got // 512
    assert np.array_equal(operand, np.broadcast_to(operand[:, :, ::KB, ::TILE].repeat(KB, 2).repeat(TILE, 3), got.shape))
    for g in range(-(-bt // GROUP)):
        tg = min(GROUP, bt - GROUP * g)
        for kb in range(kbs):
            blk = got[:, :, kb * KB:(kb + 1) * KB, g * GROUP * TILE:(g * GROUP + tg) * TILE]
            assert blk.max() - blk.min() + 1 == blk.size == tg * 2 * P * 512


def bf16_rne(v):
    """f32 -> bf16 bits, round to nearest, ties to even: the integer rule on the bits."""
    u = v.astype(np.float32).view(np.uint32).astype(np.uint64)
    low, odd = u & 0xFFFF, (u >> 16) & 1
    up = (low > 0x8000) | ((low == 0x8000) & (odd == 1))
    return ((u >> 16) + up).astype(np.uint16)


def bf16_value(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def split(v):
    """The chain v0 = b(v), v1 = b(v - v0), v2 = b(v - v0 - v1), every subtraction checked exact."""
    out, r = [], v.astype(np.float32)
    for _ in range(3):
        h = bf16_rne(r)
        nxt = r - bf16_value(h)
        assert np.array_equal(nxt.astype(np.float64), r.astype(np.float64) - bf16_value(h).astype(np.float64))
        out.append(h)
        r = nxt
    assert not r.any()  # three pieces hold all 24 bits
    return out


def test_split_rounds_ties_to_even(probe):
    cases = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F808001: 0x3F81, 0x3F807FFF: 0x3F80, 0xBF818000: 0xBF82,
             0x00000000: 0x0000, 0x80000000: 0x8000, 0x3F800000: 0x3F80, 0x5F7F8000: 0x5F80, 0x3EAAAAAB: 0x3EAB}
    bits = np.array(list(cases), dtype=np.uint32)
    got = np.array(probe("split", *bits).split(), dtype=np.int64).reshape(-1, 3)
    assert [int(v) for v in got[:, 0]] == list(cases.values())
    want = split(bits.view(np.float32))
    for i in range(3):
        assert np.array_equal(got[:, i], want[i].astype(np.int64)), i


@pytest.mark.parametrize("N,hop,bins", [(2, 1, 2), (16, 3, 5), (30, 7, 33), (400, 160, 80), (2048, 2048, 256)])
def test_tables(probe, tmp_path, N, hop, bins):
    K = N // 2 + 1
    bt, kbs = -(-K // TILE), -(-N // KB)
    q = next(q for q in (1, 2, 4, 8) if q * TILE >= bins)
    nb, nf = bt * N * 64, bt * 16 * q * 64
    path = tmp_path / "tables.bin"
    # F32 through mel_plan_create_ex: byte for byte mel_plan_create's tables
    assert [int(v) for v in probe("tables", F32, N, hop, bins, path).split()] == [E_OK, nb, nf, 0]
    raw = np.fromfile(path, dtype=np.uint8)
    assert raw.size == 2 * 4 * (nb + nf) and np.array_equal(raw[:4 * (nb + nf)], raw[4 * (nb + nf):])
    n, k = np.arange(N, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    for math, P in PIECES.items():
        ne = bt * kbs * 2 * P * 512
        assert [int(v) for v in probe("tables", math, N, hop, bins, path).split()] == [E_OK, nb, nf, ne]
        raw = np.fromfile(path, dtype=np.uint8)
        assert raw.size == 4 * (nb + nf) + 2 * ne + 4 * nf
        basis = raw[:4 * nb].view(np.float32)
        pieces = raw[4 * (nb + nf):4 * (nb + nf) + 2 * ne].view(np.uint16)
        assert np.array_equal(raw[4 * nb:4 * (nb + nf)], raw[4 * (nb + nf) + 2 * ne:])  # the filter table is unchanged
        used = np.zeros(ne, dtype=bool)
        for im in (0, 1):
            f32 = basis[(((((k // TILE) * (N // 2) + n // 2) * 2 + im) * 2 + n % 2) * TILE + k % TILE)]  # test_mel_plan.py
            want = split(f32)
            total = np.zeros(f32.shape, dtype=np.float64)
            for piece in range(P):
                at = piece_index(N, P, k, n, im, piece)
                used[at.ravel()] = True
                got = pieces[at]
                assert np.array_equal(got, want[piece]), (math, im, piece)
                total += bf16_value(got).astype(np.float64)
            if P == 3:
                assert np.array_equal(total, f32.astype(np.float64))  # the pieces sum to the entry exactly
            else:
                assert np.all(np.abs(total - f32.astype(np.float64)) <= 2.0 ** -17 * np.abs(f32.astype(np.float64)))  # two roundings to 8 bits
            if im:
                for piece in range(P):
                    s = bf16_value(pieces[piece_index(N, P, k, n, 1, piece)])  # (the f32 entry is -w * 0 = -0)
                    assert not s[:, 0].any() and not s[:, N // 2].any()
        assert used.sum() == 2 * P * N * K
        assert not pieces[~used].any()  # samples N .. 16 kbs - 1 and bins K .. 32 bt - 1: zero pieces


def test_sanitized_probe_gives_the_same_answers(probe, tmp_path):
    """Every case the tests above ran, through the -fsanitize=address,undefined build."""
    exe = _build("mel_bf16_probe_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    cases = list(probe.ran)
    if not any(a[0] == "tables" for a, _ in cases):  # (run alone)
        cases += [(["tables", "1", "30", "7", "33", str(tmp_path / "t.bin")], None),
                  (["tables", "2", "400", "160", "80", str(tmp_path / "t.bin")], None),
                  (["create", "3", "-1", "0", "0", "0", "1", "400", "160", "80", "0", "0", "4"], "14 0 0 0 0\n"),
                  (["create", "1", "-1", "0", "0", "0", "1", "2048", "2048", "256", "0", "0", "0"], None),
                  (["index", "1", "30", "33"], None),
                  (["split", "1065385984", "0"], None)]
    assert cases
    for args, out in cases:
        if args[0] == "tables":
            args = args[:-1] + [str(tmp_path / "san.bin")]
        p = subprocess.run([exe, *args], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.stderr[-2000:])
        assert out is None or p.stdout == out, args
