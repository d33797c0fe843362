"""The host side of framed plans, mirror padding and the CMVN call (zflac_amd/csrc/mel_plan.cpp:
mel_plan_create_framed, the folded tables, mel_plan_frames, mel_plan_run_ex, mel_plan_cmvn) without
a GPU. tests/c/fbank_probe.cpp is a program of its own linked with mel_plan.cpp by plain g++; the
same cases run once more through a build of it with -fsanitize=address,undefined."""
from __future__ import annotations

import os
import struct
import subprocess

import numpy as np
import pytest

from . import fbank_ref as R
from .test_mel_bf16_plan import bf16_value, split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zflac_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "c", "_build")
E_OK, E_INVALID = 0, 14
F32, X6, X3 = 0, 1, 2
TILE, KB, GROUP = 32, 16, 2
PIECES = {X6: 3, X3: 2}
STFT, SNIP, KALDI = 0, 1, 2


def fbits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _build(name, extra):
    srcs = [os.path.join(ROOT, "tests", "c", "fbank_probe.cpp"), os.path.join(CSRC, "mel_plan.cpp")]
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
    exe = _build("fbank_probe", [])
    ran = []

    def run(*args):
        args = [str(a) for a in args]
        out = subprocess.run([exe, *args], capture_output=True, text=True, check=True).stdout
        ran.append((args, out))
        return out

    run.ran = ran
    return run


def create(probe, math=F32, size=-1, dtype=0, layout=0, scale=0, center=0, n=512, hop=160, bins=80, reserved=0, floor=None,
           flags=0, fsize=-1, nw=400, framing=SNIP, dc=1, a=0.97, g=32768.0, freserved=0):
    if floor is None:
        floor = 0 if scale == 0 else 1e-10
    a = a if isinstance(a, int) else fbits(a)
    g = g if isinstance(g, int) else fbits(g)
    return [int(v) for v in probe("create", math, size, dtype, layout, scale, center, n, hop, bins, reserved, floor, flags,
                                  fsize, nw, framing, dc, a, g, freserved).split()]


REFUSED = [E_INVALID, 0, 0, 0, 0, 0, 0, 0]


def test_good_plans(probe):
    # rc win_length span off framing math k_blocks n_pieces
    assert create(probe) == [E_OK, 400, 400, 0, SNIP, F32, 0, 0]
    assert create(probe, framing=KALDI) == [E_OK, 400, 400, 200 - 80, KALDI, F32, 0, 0]
    assert create(probe, framing=STFT, center=1) == [E_OK, 400, 400, 256 - 56, STFT, F32, 0, 0]
    assert create(probe, framing=STFT, center=0) == [E_OK, 400, 400, -56, STFT, F32, 0, 0]
    assert create(probe, math=X6) == [E_OK, 400, 400, 0, SNIP, X6, 25, 3]
    assert create(probe, math=X3, n=2048, nw=1201, hop=1201, bins=256) == [E_OK, 1201, 1202, 0, SNIP, X3, 76, 2]
    assert create(probe, n=16, nw=11, hop=3, bins=5, framing=KALDI) == [E_OK, 11, 12, 5 - 1, KALDI, F32, 0, 0]
    assert create(probe, n=2, nw=1, hop=1, bins=2) == [E_OK, 1, 2, 0, SNIP, F32, 0, 0]
    assert create(probe, n=2, nw=2, hop=1, bins=2, framing=STFT, center=1) == [E_OK, 2, 2, 1, STFT, F32, 0, 0]


NAN, INF = 0x7FC00000, 0x7F800000
# one bad argument per rule, each rule at its edge, in the documented order: (refused, accepted neighbour)
RULES = [
    (dict(flags=1), None), (dict(flags=2), None), (dict(size=39), None), (dict(dtype=3), dict(dtype=2)),
    (dict(layout=2), dict(layout=1)), (dict(scale=3), dict(scale=2)), (dict(center=2), None),
    (dict(n=513), dict(n=2048, nw=400)), (dict(n=2050), None), (dict(hop=0), dict(hop=1)), (dict(n=512, hop=513), None),
    (dict(bins=0), dict(bins=1)), (dict(bins=257), dict(bins=256)), (dict(reserved=1), None), (dict(scale=1, floor=0), None),
    (dict(flags=64), None), (dict(fsize=19), None), (dict(fsize=24), None), (dict(nw=0), dict(nw=160)),
    (dict(nw=513), dict(nw=512)), (dict(framing=3), dict(framing=2)), (dict(dc=2), dict(dc=1)),
    (dict(a=fbits(-1e-45) | 0), dict(a=0.0)), (dict(a=0x3F800001), dict(a=1.0)), (dict(a=NAN), None),
    (dict(g=0.0), None), (dict(g=fbits(2.0 ** -64) - 1), dict(g=2.0 ** -64)), (dict(g=fbits(2.0 ** 64) + 1), dict(g=-2.0 ** 64)),
    (dict(g=INF), None), (dict(g=NAN), None), (dict(freserved=1), None),
    (dict(flags=4), None), (dict(flags=8), None), (dict(flags=16), dict(flags=128)), (dict(flags=32), None),
    (dict(framing=SNIP, center=1), dict(framing=STFT, center=1)), (dict(framing=KALDI, center=1), None),
    (dict(nw=159), dict(nw=160)), (dict(math=3), dict(math=2)), (dict(math=0xFFFFFFFF), None),
]


@pytest.mark.parametrize("i", range(len(RULES)), ids=lambda i: "-".join(f"{k}{v}" for k, v in RULES[i][0].items()))
def test_every_refusal_at_its_edge_and_in_order(probe, i):
    """Rule i refuses, its neighbour on the good side is accepted, and with any later rule broken
    as well the answer is still rule i's (the plan untouched): later rules are not reached, the
    NULL tables and descriptor of the later rules included."""
    bad, good = RULES[i]
    assert create(probe, **bad) == REFUSED
    if good is not None:
        assert create(probe, **good)[0] == E_OK, good
    for later, _ in RULES[i + 1:]:
        both = dict(later)
        both.update(bad)
        if "flags" in bad and "flags" in later:
            both["flags"] = bad["flags"] | later["flags"]
        assert create(probe, **both) == REFUSED, (bad, later)


def test_a_negative_zero_preemphasis_is_zero(probe):
    assert create(probe, a=0x80000000)[0] == E_OK


def basis_index(span, n, k, im):
    return ((((k // TILE) * (span // 2) + n // 2) * 2 + im) * 2 + n % 2) * TILE + k % TILE


def piece_index(Nw, K, n_pieces, k, n, im, piece):
    bt, kbs = -(-K // TILE), -(-Nw // KB)
    b = k // TILE
    g, bi = b // GROUP, b % GROUP
    tg = np.minimum(GROUP, bt - GROUP * g)
    operand = ((g * GROUP * kbs + (n // KB) * tg + bi) * 2 + im) * n_pieces + piece
    return (operand * 64 + 32 * ((n % KB) // 8) + k % TILE) * 8 + n % 8


def probe_window(Nw):
    return (0.25 + ((np.arange(Nw) * 37) % 101) / 128.0).astype(np.float32)


def ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("N,Nw,hop,bins", [(2, 1, 1, 2), (2, 2, 1, 2), (16, 11, 3, 5), (32, 30, 7, 33), (512, 400, 160, 80),
                                            (2048, 1201, 1201, 256)])
@pytest.mark.parametrize("a,dc,g", [(0.97, 1, 32768.0), (0.0, 0, 1.0), (1.0, 1, -0.75)])
def test_tables(probe, tmp_path, N, Nw, hop, bins, a, dc, g):
    K = N // 2 + 1
    bt, kbs, span = -(-K // TILE), -(-Nw // KB), Nw + (Nw & 1)
    q = next(q for q in (1, 2, 4, 8) if q * TILE >= bins)
    nb, nf = bt * span * 64, bt * 16 * q * 64
    path = tmp_path / "tables.bin"
    w = probe_window(Nw)
    c, s = R.folded(w, N, np.float64(np.float32(a)), bool(dc), np.float64(np.float32(g)))
    # the pre-rounding difference of two builders: 2^-40 sum_m |w[m] A[m][n]|; then one f32 ulp of rounding
    pre = 2.0 ** -40 * np.abs(R.operator_matrix(w, a, bool(dc), g)).sum(axis=0)[:, None]
    n, k = np.arange(Nw, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    assert [int(v) for v in probe("tables", F32, N, Nw, hop, bins, SNIP, 0, dc, fbits(a), fbits(g), path).split()] == \
        [E_OK, nb, 0, nf, span, 0]
    raw = np.fromfile(path, dtype=np.float32)
    assert raw.size == nb + nf
    basis = raw[:nb]
    used = np.zeros(nb, dtype=bool)
    f32 = {}
    for im, want in ((0, c), (1, s)):
        at = basis_index(span, n, k, im)
        used[at.ravel()] = True
        got = basis[at].astype(np.float64)
        f32[im] = basis[at]
        # |got - fl(want')| with |want' - want| <= pre: got lies within pre of want, widened by the rounding
        assert np.all(np.abs(got - want) <= pre + 0.5 * ulp32(want) + 0.5 * ulp32(got)), (im, np.max(np.abs(got - want)))
        exact = np.abs(want) > 2.0 ** 20 * pre  # away from a rounding tie the entry is the rounded reference or its neighbour
        assert np.all(np.abs(got - want.astype(np.float32).astype(np.float64))[exact] <= ulp32(want)[exact])
    assert used.sum() == 2 * Nw * K and not basis[~used].any()     # the zero row of an odd Nw, bins K .. 32 bt - 1
    if a == 0.0 and not dc:
        assert not f32[1][:, 0].any() and not f32[1][:, N // 2].any()  # the sine columns 0 and N / 2
    for math, P in PIECES.items():
        ne = bt * kbs * 2 * P * 512
        assert [int(v) for v in probe("tables", math, N, Nw, hop, bins, SNIP, 0, dc, fbits(a), fbits(g), path).split()] == \
            [E_OK, 0, ne, nf, span, kbs]
        rawb = np.fromfile(path, dtype=np.uint8)
        assert rawb.size == 2 * ne + 4 * nf
        pieces = rawb[:2 * ne].view(np.uint16)
        assert np.array_equal(rawb[2 * ne:].view(np.float32), raw[nb:])  # the filter table is the f32 plan's
        usedp = np.zeros(ne, dtype=bool)
        for im in (0, 1):
            want = split(f32[im])
            total = np.zeros(f32[im].shape, dtype=np.float64)
            for piece in range(P):
                at = piece_index(Nw, K, P, k, n, im, piece)
                usedp[at.ravel()] = True
                assert np.array_equal(pieces[at], want[piece]), (math, im, piece)
                total += bf16_value(pieces[at]).astype(np.float64)
            if P == 3:
                assert np.array_equal(total, f32[im].astype(np.float64))  # the pieces sum to the f32 entry exactly
        assert usedp.sum() == 2 * P * Nw * K and not pieces[~usedp].any()  # samples Nw .. 16 kbs - 1: zero pieces


def test_sine_columns_are_zero_before_the_folding(probe, tmp_path):
    """With pre-emphasis but no DC removal, column k = 0 and k = N / 2 of s' stay exactly 0: they are
    combinations of exact zeros."""
    path = tmp_path / "t.bin"
    N, Nw = 32, 30
    probe("tables", F32, N, Nw, 7, 33, SNIP, 0, 0, fbits(0.97), fbits(32768.0), path)
    basis = np.fromfile(path, dtype=np.float32)
    n = np.arange(Nw)
    for k in (0, N // 2):
        assert not basis[basis_index(Nw, n, k, 1)].any()


@pytest.mark.parametrize("math", [F32, X6, X3])
@pytest.mark.parametrize("N,hop,bins,center", [(2, 1, 2, 1), (30, 7, 33, 0), (400, 160, 80, 1), (2048, 2048, 256, 0)])
def test_identity_plan_has_mel_tables_bytes(probe, math, N, hop, bins, center):
    assert probe("identity", math, N, hop, bins, center).split() == ["0", "1"]


@pytest.mark.parametrize("N,Nw,hop", [(2, 1, 1), (16, 11, 3), (32, 30, 7), (512, 400, 160), (2048, 1201, 1201)])
def test_plan_frames(probe, N, Nw, hop):
    ns = sorted({0, 1, 2, max(Nw // 2 - 1, 0), Nw // 2, Nw - 1, Nw, Nw + 1, 20 * hop - 1, 20 * hop, 20 * hop + 1, 2 ** 40,
                 2 ** 63})
    for framing, center in ((STFT, 0), (STFT, 1), (SNIP, 0), (KALDI, 0)):
        got = [int(v) for v in probe("frames", framing, N, Nw, hop, center, *ns).split()]
        assert got == [R.plan_frames(framing, n, N, Nw, hop, center) for n in ns], (framing, center)


def test_mirror_needs_a_kaldi_center_plan(probe):
    ZEROS, REFLECT, MIRROR = 0, 1, 2
    for framing, center in ((STFT, 0), (STFT, 1), (SNIP, 0), (KALDI, 0)):
        for nw in (11, 16):
            assert int(probe("runex", ZEROS, framing, center, nw)) == E_OK
            assert int(probe("runex", REFLECT, framing, center, nw)) == (E_OK if center else E_INVALID)
            assert int(probe("runex", MIRROR, framing, center, nw)) == (E_OK if framing == KALDI else E_INVALID)
            assert int(probe("runex", 3, framing, center, nw)) == E_INVALID


def cmvn(probe, size=-1, mode=1, ddof=0, reserved=0, feat=0x1000, rows=3, frames=7, valid=0x2000, mean=0x3000, std=0x4000,
         eps=1e-5, pad=0.0, layout=0, flags=0):
    eps = eps if isinstance(eps, int) else fbits(eps)
    pad = pad if isinstance(pad, int) else fbits(pad)
    return [int(v) for v in probe("cmvn", size, mode, ddof, reserved, feat, rows, frames, valid, mean, std, eps, pad, layout,
                                  flags).split()]


CMVN_RULES = [dict(flags=1), dict(flags=2), dict(size=63), dict(mode=2), dict(ddof=2), dict(reserved=1), dict(feat=0),
              dict(frames=0), dict(rows=2 ** 62, frames=2 ** 10), dict(valid=0x2004), dict(mean=0x3002), dict(std=0x4001),
              dict(eps=fbits(-1e-45)), dict(pad=INF)]


def test_cmvn_checks_in_order(probe):
    assert cmvn(probe) == [E_OK, 3 * 80]
    assert cmvn(probe, layout=1) == [E_OK, 3]
    assert cmvn(probe, rows=0) == [E_OK, 0]
    assert cmvn(probe, mode=0, ddof=1, valid=0, mean=0, std=0, eps=0.0, pad=-1e30) == [E_OK, 240]
    assert cmvn(probe, eps=NAN) == [E_INVALID, 0] and cmvn(probe, eps=INF) == [E_INVALID, 0] and cmvn(probe, pad=NAN) == [E_INVALID, 0]
    assert cmvn(probe, rows=2 ** 40, frames=2 ** 13)[0] == E_OK and cmvn(probe, rows=2 ** 41, frames=2 ** 14)[0] == E_INVALID
    for i, bad in enumerate(CMVN_RULES):
        assert cmvn(probe, **bad) == [E_INVALID, 0], bad
        for later in CMVN_RULES[i + 1:]:
            both = dict(later)
            both.update(bad)
            if "flags" in bad and "flags" in later:
                both["flags"] = bad["flags"] | later["flags"]
            assert cmvn(probe, **both) == [E_INVALID, 0], (bad, later)


def test_sanitized_probe_gives_the_same_answers(probe, tmp_path):
    """Every case the tests above ran, through the -fsanitize=address,undefined build."""
    exe = _build("fbank_probe_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    cases = list(probe.ran)
    if not any(a[0] == "tables" for a, _ in cases):  # (run alone)
        t = str(tmp_path / "t.bin")
        cases += [(["tables", "0", "16", "11", "3", "5", "1", "0", "1", str(fbits(0.97)), str(fbits(32768.0)), t], None),
                  (["tables", "1", "2048", "1201", "1201", "256", "1", "0", "1", str(fbits(0.97)), str(fbits(32768.0)), t], None),
                  (["tables", "2", "2", "1", "1", "2", "1", "0", "1", str(fbits(1.0)), str(fbits(1.0)), t], None),
                  (["identity", "1", "30", "7", "33", "0"], "0 1\n"),
                  (["frames", "2", "16", "11", "3", "0", "0", "1", "18446744073709551615"], None),
                  (["runex", "2", "2", "0", "11"], "0\n")]
    assert cases
    for args, out in cases:
        if args[0] == "tables":
            args = args[:-1] + [str(tmp_path / "san.bin")]
        p = subprocess.run([exe, *args], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.stderr[-2000:])
        assert out is None or p.stdout == out, args
