"""The host side of the cepstra plans (zflac_amd/csrc/cepstra_plan.cpp: the argument checks of
zflac_hip_cepstra_create / _project / _cmvn / _deltas in their documented order, the delta scale
tables, the grids) without a GPU. tests/c/cepstra_probe.cpp is a program of its own linked with
cepstra_plan.cpp and mel_plan.cpp by plain g++; the same cases run once more through a build of it
with -fsanitize=address,undefined."""
from __future__ import annotations

import os
import struct
import subprocess

import numpy as np
import pytest

from . import cepstra_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zflac_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "c", "_build")
E_OK, E_INVALID = 0, 14
F32, F16, BF16 = 0, 1, 2
NAN, INF = 0x7FC00000, 0x7F800000
MAX_GRID = 2 ** 31 - 1


def fbits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _build(name, extra):
    srcs = [os.path.join(ROOT, "tests", "c", "cepstra_probe.cpp"), os.path.join(CSRC, "cepstra_plan.cpp"),
            os.path.join(CSRC, "mel_plan.cpp")]
    deps = srcs + [os.path.join(CSRC, "cepstra_plan.h"), os.path.join(CSRC, "mel_plan.h"), os.path.join(CSRC, "common.h"),
                   os.path.join(ROOT, "include", "zflac_hip.h")]
    exe = os.path.join(BUILD, name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Werror", "-O1", "-g", *extra, "-I", CSRC, "-I",
                               os.path.join(ROOT, "include"), *srcs, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def probe():
    exe = _build("cepstra_probe", [])
    ran = []

    def run(*args):
        args = [str(a) for a in args]
        out = subprocess.run([exe, *args], capture_output=True, text=True, check=True).stdout
        ran.append((args, out))
        return out

    run.ran = ran
    return run


def ints(out):
    return [int(v) for v in out.split()]


def create(probe, size=-1, i=F32, o=F32, layout=0, order=2, n_in=80, n_out=13, window=2, r0=0, r1=0, r2=0, flags=0):
    return ints(probe("create", size, i, o, layout, order, n_in, n_out, window, r0, r1, r2, flags))


CREATE_REFUSED = [E_INVALID] + [0] * 9


def test_good_plans(probe):
    # rc in out layout has_matrix n_in n_out order window features
    assert create(probe) == [E_OK, F32, F32, 0, 1, 80, 13, 2, 2, 39]
    assert create(probe, i=BF16, o=F16, layout=1, order=0, window=0) == [E_OK, BF16, F16, 1, 1, 80, 13, 0, 0, 13]
    assert create(probe, n_in=1, n_out=1, order=3, window=5) == [E_OK, F32, F32, 0, 1, 1, 1, 3, 5, 4]
    assert create(probe, n_in=256, n_out=256, order=1, window=1) == [E_OK, F32, F32, 0, 1, 256, 256, 1, 1, 512]
    assert create(probe, n_in=1, n_out=256, order=0, window=0)[0] == E_OK  # more features than bins: any matrix
    assert create(probe, flags=4, n_in=13, n_out=13, i=F16, o=F16) == [E_OK, F16, F16, 0, 0, 13, 13, 2, 2, 39]  # deltas only
    assert create(probe, flags=16)[0] == E_OK  # what lies behind the matrix is not read


# one bad argument per rule, each rule at its edge, in the documented order: (refused, accepted neighbour)
CREATE_RULES = [
    (dict(flags=1), None), (dict(flags=2), None), (dict(size=23), None), (dict(size=25), None),
    (dict(i=3), dict(i=2)), (dict(o=3), dict(o=2)), (dict(layout=2), dict(layout=1)), (dict(order=4), dict(order=3)),
    (dict(n_in=0), dict(n_in=1)), (dict(n_in=257), dict(n_in=256)), (dict(n_out=0), dict(n_out=1)),
    (dict(n_out=257), dict(n_out=256)), (dict(window=0), dict(window=1)), (dict(window=6), dict(window=5)),
    (dict(order=0, window=1), dict(order=0, window=0)), (dict(r0=1), None), (dict(r1=1), None), (dict(r2=128), None),
    (dict(flags=4, n_in=13, n_out=12), dict(flags=4, n_in=13, n_out=13)),
    (dict(flags=4, n_in=13, n_out=13, i=F32, o=F16), dict(flags=4, n_in=13, n_out=13, i=F16, o=F16)),
    (dict(flags=4, n_in=13, n_out=13, order=0, window=0), dict(flags=4, n_in=13, n_out=13, order=1, window=1)),
    (dict(flags=8), None),
]


def clash(bad, later):
    """The two rules are broken through the same argument: together they are not both broken."""
    return bool((set(bad) & set(later)) - {"flags"})


def merged(bad, later):
    both = dict(later)
    both.update(bad)
    if "flags" in bad and "flags" in later:
        both["flags"] = bad["flags"] | later["flags"]
    return both


@pytest.mark.parametrize("i", range(len(CREATE_RULES)), ids=lambda i: "-".join(f"{k}{v}" for k, v in CREATE_RULES[i][0].items()))
def test_every_create_refusal_at_its_edge_and_in_order(probe, i):
    """Rule i refuses, its neighbour on the good side is accepted, and with any later rule broken
    as well the answer is still rule i's, the plan untouched."""
    bad, good = CREATE_RULES[i]
    assert create(probe, **bad) == CREATE_REFUSED
    if good is not None:
        assert create(probe, **good)[0] == E_OK, good
    for later, _ in CREATE_RULES[i + 1:]:
        if clash(bad, later):
            continue
        assert create(probe, **merged(bad, later)) == CREATE_REFUSED, (bad, later)


@pytest.mark.parametrize("window", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_scale_tables(probe, order, window):
    lines = probe("scales", order, window).splitlines()
    got = np.array([struct.unpack("<f", struct.pack("<I", int(v)))[0] for v in lines[0].split()], dtype=np.float32)
    want = R.delta_scales(order, window)
    assert got.shape == want.shape == (2 * order * window + 1,)
    # two float64 builds of a tap differ by parts in 2^-50; then one f32 rounding
    assert np.all(np.abs(got.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 2.0 ** -60)
    assert int(lines[1]) == sum(2 * o * window + 1 for o in range(1, order))
    if (order, window) == (1, 2):
        assert np.array_equal(got, (np.array([-2, -1, 0, 1, 2]) / 10.0).astype(np.float32))
    if (order, window) == (2, 2):
        assert np.allclose(got * 100.0, [4, 4, 1, -4, -10, -4, 1, 4, 4], rtol=2.0 ** -22, atol=0)
    if window == 1:  # dyadic taps are exact
        assert np.array_equal(got.astype(np.float64), want)


def project(probe, size=-1, reserved=0, src=0x1000, dst=0x9000, rows=3, frames=130, flags=0, n_in=80, n_out=13, i=F32, o=F32):
    return ints(probe("project", size, reserved, src, dst, rows, frames, flags, n_in, n_out, i, o))


PROJECT_RULES = [
    (dict(flags=1), None), (dict(flags=2), None), (dict(size=39), None), (dict(reserved=1), None), (dict(flags=4), None),
    (dict(src=0), None), (dict(dst=0), None), (dict(src=0x9000), None), (dict(src=0x1002), dict(src=0x1004)),
    (dict(dst=0x9001), dict(dst=0x9004)), (dict(frames=0), dict(frames=1)),
    (dict(rows=2 ** 41, frames=2 ** 14, n_in=256, n_out=1), dict(rows=2 ** 40, frames=2 ** 13, n_in=256, n_out=1)),
    (dict(rows=2 ** 41, frames=2 ** 14, n_in=1, n_out=256), dict(rows=2 ** 40, frames=2 ** 13, n_in=1, n_out=256)),
]


def test_project_checks_in_order_and_grids(probe):
    assert project(probe) == [E_OK, 3, 9, 9]                      # rc, tiles of 64 frames, passes, blocks
    assert project(probe, frames=64) == [E_OK, 1, 3, 3] and project(probe, frames=65) == [E_OK, 2, 6, 6]
    assert project(probe, rows=0) == [E_OK, 3, 0, 0]
    assert project(probe, i=F16, src=0x1002) == [E_OK, 3, 9, 9] and project(probe, o=BF16, dst=0x9002)[0] == E_OK
    # the grid stops at 2^31 - 1 workgroups, each striding over the passes
    assert project(probe, rows=MAX_GRID, frames=64) == [E_OK, 1, MAX_GRID, MAX_GRID]
    assert project(probe, rows=MAX_GRID + 1, frames=64) == [E_OK, 1, MAX_GRID + 1, MAX_GRID]
    assert project(probe, rows=2 ** 31, frames=65, n_in=1, n_out=1) == [E_OK, 2, 2 ** 32, MAX_GRID]
    # 63 bits: 2^40 * 256 * 2^13 * 4 = 2^63 is refused, one row fewer is not
    assert project(probe, rows=2 ** 40, frames=2 ** 13, n_in=256, n_out=1)[0] == E_INVALID
    assert project(probe, rows=2 ** 40 - 1, frames=2 ** 13, n_in=256, n_out=1)[0] == E_OK
    assert project(probe, rows=2 ** 40, frames=2 ** 13, n_in=256, n_out=1, i=F16)[0] == E_OK  # half the bytes
    assert project(probe, rows=2 ** 64 - 1, frames=2 ** 64 - 1)[0] == E_INVALID
    rules = [(b, g) for b, g in PROJECT_RULES]
    rules[11] = (dict(rows=2 ** 40, frames=2 ** 13, n_in=256, n_out=1), dict(rows=2 ** 40 - 1, frames=2 ** 13, n_in=256, n_out=1))
    rules[12] = (dict(rows=2 ** 40, frames=2 ** 13, n_in=1, n_out=256), dict(rows=2 ** 40 - 1, frames=2 ** 13, n_in=1, n_out=256))
    for i, (bad, good) in enumerate(rules):
        assert project(probe, **bad) == [E_INVALID, 0, 0, 0], bad
        if good is not None:
            assert project(probe, **good)[0] == E_OK, good
        for later, _ in rules[i + 1:]:
            if clash(bad, later):
                continue
            assert project(probe, **merged(bad, later)) == [E_INVALID, 0, 0, 0], (bad, later)


def deltas(probe, size=-1, reserved=0, reserved2=0, src=0x1000, dst=0x9000, rows=3, frames=133, valid=0x2000, pad=0.0, flags=0,
           C=13, dtype=F32, layout=0, order=2, window=2):
    pad = pad if isinstance(pad, int) else fbits(pad)
    return ints(probe("deltas", size, reserved, reserved2, src, dst, rows, frames, valid, pad, flags, C, dtype, layout, order, window))


DELTA_RULES = [
    (dict(flags=1), None), (dict(flags=2), None), (dict(size=55), None), (dict(reserved=1), None), (dict(reserved2=1), None),
    (dict(flags=4), None), (dict(src=0), None), (dict(dst=0), None), (dict(src=0x9000), None),
    (dict(src=0x1002), dict(src=0x1004)), (dict(dst=0x9003), dict(dst=0x9004)), (dict(frames=0), dict(frames=1)),
    (dict(rows=2 ** 40, frames=2 ** 13, C=256, order=1, window=1), dict(rows=2 ** 39, frames=2 ** 13, C=256, order=1, window=1)),
    (dict(valid=0x2004), dict(valid=0)), (dict(pad=INF), dict(pad=-1e30)), (dict(pad=NAN), None),
]


def test_deltas_checks_in_order_and_grids(probe):
    # bins first: tiles of 256 frames per (row, feature); frames first: 256 // C frames of a row per pass
    assert deltas(probe) == [E_OK, 1, 3 * 13, 39]
    assert deltas(probe, frames=256) == [E_OK, 1, 39, 39] and deltas(probe, frames=257) == [E_OK, 2, 78, 78]
    assert deltas(probe, layout=1) == [E_OK, 7, 21, 21]           # 256 // 13 = 19 frames a pass, ceil(133 / 19) = 7
    assert deltas(probe, layout=1, C=256) == [E_OK, 133, 399, 399] and deltas(probe, layout=1, C=1)[1:] == [1, 3, 3]
    assert deltas(probe, layout=1, C=129) == [E_OK, 133, 399, 399] and deltas(probe, layout=1, C=128)[1] == 67
    assert deltas(probe, rows=0) == [E_OK, 1, 0, 0]
    assert deltas(probe, dtype=BF16, src=0x1002, dst=0x9002)[0] == E_OK
    assert deltas(probe, rows=MAX_GRID, C=1, frames=256) == [E_OK, 1, MAX_GRID, MAX_GRID]
    assert deltas(probe, rows=MAX_GRID + 1, C=1, frames=256) == [E_OK, 1, MAX_GRID + 1, MAX_GRID]
    assert deltas(probe, rows=MAX_GRID + 1, C=1, frames=256, layout=1) == [E_OK, 1, MAX_GRID + 1, MAX_GRID]
    # 63 bits: 2^40 rows * 2 * 256 features * 2^13 frames * 4 bytes = 2^64; 2^39 rows: 2^63, one fewer fits
    assert deltas(probe, rows=2 ** 39, frames=2 ** 13, C=256, order=1, window=1)[0] == E_INVALID
    assert deltas(probe, rows=2 ** 39 - 1, frames=2 ** 13, C=256, order=1, window=1)[0] == E_OK
    rules = list(DELTA_RULES)
    rules[12] = (dict(rows=2 ** 39, frames=2 ** 13, C=256, order=1, window=1), dict(rows=2 ** 39 - 1, frames=2 ** 13, C=256, order=1, window=1))
    for i, (bad, good) in enumerate(rules):
        assert deltas(probe, **bad) == [E_INVALID, 0, 0, 0], bad
        if good is not None:
            assert deltas(probe, **good)[0] == E_OK, good
        for later, _ in rules[i + 1:]:
            if clash(bad, later):
                continue
            assert deltas(probe, **merged(bad, later)) == [E_INVALID, 0, 0, 0], (bad, later)


def cmvn(probe, size=-1, mode=1, ddof=0, reserved=0, feat=0x1000, rows=3, frames=7, valid=0x2000, mean=0x3000, std=0x4000,
         eps=1e-5, pad=0.0, layout=0, flags=0, n_out=13, dtype=F32):
    eps = eps if isinstance(eps, int) else fbits(eps)
    pad = pad if isinstance(pad, int) else fbits(pad)
    return ints(probe("cmvn", size, mode, ddof, reserved, feat, rows, frames, valid, mean, std, eps, pad, layout, flags, n_out, dtype))


# zflac_hip_mel_cmvn's rules in zflac_hip_mel_cmvn's order (tests/test_fbank_plan.py)
CMVN_RULES = [dict(flags=1), dict(flags=2), dict(size=63), dict(mode=2), dict(ddof=2), dict(reserved=1), dict(feat=0),
              dict(frames=0), dict(rows=2 ** 62, frames=2 ** 10), dict(valid=0x2004), dict(mean=0x3002), dict(std=0x4001),
              dict(eps=fbits(-1e-45)), dict(pad=INF)]


def test_cmvn_checks_are_mel_cmvns(probe):
    assert cmvn(probe) == [E_OK, 3 * 13]            # bins first: a pass per (row, feature) of n_out
    assert cmvn(probe, layout=1) == [E_OK, 3] and cmvn(probe, rows=0) == [E_OK, 0]
    assert cmvn(probe, n_out=256) == [E_OK, 768]
    assert cmvn(probe, eps=NAN) == [E_INVALID, 0] and cmvn(probe, pad=NAN) == [E_INVALID, 0]
    # the bytes are n_out's and out_dtype's: 2^40 * 256 * 2^13 * 4 = 2^63
    assert cmvn(probe, rows=2 ** 40, frames=2 ** 13, n_out=256)[0] == E_INVALID
    assert cmvn(probe, rows=2 ** 40, frames=2 ** 13, n_out=256, dtype=F16)[0] == E_OK
    assert cmvn(probe, rows=2 ** 40, frames=2 ** 13, n_out=255)[0] == E_OK
    for i, bad in enumerate(CMVN_RULES):
        assert cmvn(probe, **bad) == [E_INVALID, 0], bad
        for later in CMVN_RULES[i + 1:]:
            if clash(bad, later):
                continue
            assert cmvn(probe, **merged(bad, later)) == [E_INVALID, 0], (bad, later)


def test_grid_rule(probe):
    for passes, blocks in ((0, 0), (1, 1), (MAX_GRID - 1, MAX_GRID - 1), (MAX_GRID, MAX_GRID), (MAX_GRID + 1, MAX_GRID),
                           (2 ** 63, MAX_GRID), (2 ** 64 - 1, MAX_GRID)):
        assert int(probe("grid", passes)) == blocks


def test_sanitized_probe_gives_the_same_answers(probe):
    """Every case the tests above ran, through the -fsanitize=address,undefined build."""
    exe = _build("cepstra_probe_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    cases = list(probe.ran)
    if len(cases) < 10:  # (run alone)
        cases += [(["create", "-1", "0", "0", "0", "2", "80", "13", "2", "0", "0", "0", "0"], None),
                  (["create", "-1", "0", "0", "0", "3", "256", "256", "5", "0", "0", "0", "8"], None),
                  (["scales", "3", "5"], None), (["scales", "0", "1"], None),
                  (["project", "-1", "0", "4096", "36864", str(2 ** 64 - 1), str(2 ** 64 - 1), "0", "256", "256", "0", "0"], None),
                  (["deltas", "-1", "0", "0", "4096", "36864", str(2 ** 63), "133", "0", "0", "0", "256", "0", "1", "3", "5"], None),
                  (["cmvn", "-1", "1", "0", "0", "4096", "3", "7", "0", "0", "0", str(fbits(1e-5)), "0", "0", "0", "13", "0"], None),
                  (["grid", str(2 ** 64 - 1)], f"{MAX_GRID}\n")]
    for args, out in cases:
        p = subprocess.run([exe, *args], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.stderr[-2000:])
        assert out is None or p.stdout == out, args
