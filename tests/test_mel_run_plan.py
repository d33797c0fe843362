"""zflac_hip_mel_run_ex's host half (mel_plan_run_ex, zflac_amd/csrc/mel_plan.cpp) without a GPU:
every refusal at its edge, pairs of broken rules, and the grid, which is mel_plan_run's for the
shared arguments. tests/c/mel_run_probe.cpp is a program of its own linked with mel_plan.cpp by
plain g++; the same cases run once more through a build of it with -fsanitize=address,undefined
(as a program: nothing is loaded into Python under a sanitizer).

Every refusal is the one code ZFLAC_E_INVALID_ARGUMENT, so the order of the checks shows in two
places only: a descriptor that breaks two rules is refused whichever comes first, and a descriptor
shorter than the struct is refused on its size before any field behind it is read, which the
sanitized build would report."""
from __future__ import annotations

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zflac_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "c", "_build")
E_OK, E_INVALID = 0, 14
F32, F16, BF16 = 0, 1, 2
POWER, LOG10, LN = 0, 1, 2
ZEROS, REFLECT, NONE, ROW_MAX = 0, 1, 0, 1
FRAMES = 128
GRID_MAX = 0x7FFFFFFF
WAVE, DST, LEN, RMAX = 0x7F4200000000, 0x7F5200000000, 0x7F6200000000, 0x7F7200000000  # made-up device addresses
WHISPER = dict(norm=ROW_MAX, row_max=RMAX, range=8, add=4, mul=0.25)


def _build(name, extra):
    srcs = [os.path.join(ROOT, "tests", "c", "mel_run_probe.cpp"), os.path.join(CSRC, "mel_plan.cpp")]
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
    exe = _build("mel_run_probe", [])
    ran = []

    def run(*args):
        args = [str(a) for a in args]
        out = subprocess.run([exe, *args], capture_output=True, text=True, check=True).stdout
        ran.append((args, out))
        return out

    run.ran = ran
    return run


def run_ex(probe, **kw):
    """-> [rc, tiles, blocks, mel_plan_run's rc, tiles, blocks, plain]"""
    return [int(v) for v in probe("run_ex", *[f"{k}={v}" for k, v in kw.items()]).split()]


def rc(probe, **kw):
    return run_ex(probe, **kw)[0]


def test_accepts(probe):
    assert run_ex(probe) == [E_OK, 1, 5, E_OK, 1, 5, 1]                        # the plain descriptor
    assert run_ex(probe, pad=REFLECT)[:3] + run_ex(probe, pad=REFLECT)[6:] == [E_OK, 1, 5, 0]
    assert run_ex(probe, lengths=LEN)[6] == 0 and run_ex(probe, row_max=RMAX)[6] == 0
    assert rc(probe, pad=REFLECT, lengths=LEN, **WHISPER) == E_OK
    for scale in (LOG10, LN):
        for dtype in (F32, F16, BF16):
            assert rc(probe, scale=scale, dtype=dtype, **WHISPER) == E_OK
    assert rc(probe, scale=POWER, row_max=RMAX) == E_OK                        # the maxima alone: any scale
    assert rc(probe, scale=POWER, pad=REFLECT, lengths=LEN) == E_OK
    assert rc(probe, norm=NONE, range="-0.0", add="-0.0", mul="-0.0") == E_OK  # zero is zero


def test_refusals_at_their_edges(probe):
    bad = [dict(plan=0), dict(desc=0), dict(plan=0, desc=0),
           dict(size=0), dict(size=103), dict(size=105), dict(size=96), dict(size=40),
           dict(pad=2), dict(pad=255), dict(norm=2), dict(norm=255),
           dict(reserved=1), dict(reserved=0x8000), dict(reserved2=1), dict(reserved2=0x80000000),
           dict(lengths=LEN + 1), dict(lengths=LEN + 4), dict(lengths=LEN + 7),
           dict(row_max=RMAX + 1), dict(row_max=RMAX + 2), dict(row_max=RMAX + 3),
           dict(pad=REFLECT, center=0),                                       # reflect with an uncentred plan
           dict(WHISPER, scale=POWER),                                        # ROW_MAX with the POWER scale
           dict(WHISPER, row_max=0),                                          # ... with a NULL row_max
           dict(WHISPER, mul=0), dict(WHISPER, mul="-0.0"),                   # ... with mul = 0
           dict(WHISPER, range="nan"), dict(WHISPER, range="inf"), dict(WHISPER, range="-1e-30"),
           dict(WHISPER, add="nan"), dict(WHISPER, add="inf"), dict(WHISPER, add="-inf"),
           dict(WHISPER, mul="nan"), dict(WHISPER, mul="inf"),
           dict(range=8), dict(add=4), dict(mul=0.25), dict(range="nan"), dict(mul=1e-45),  # NORM_NONE: all 0
           dict(row_max=RMAX, range=8, add=4, mul=0.25)]
    for kw in bad:
        assert rc(probe, **kw) == E_INVALID, kw
    # the exact edges that pass
    for kw in (dict(lengths=LEN + 8), dict(row_max=RMAX + 4), dict(WHISPER, range=0), dict(WHISPER, range="-0.0"),
               dict(WHISPER, add=0), dict(WHISPER, add="-3e38"), dict(WHISPER, mul=-0.25), dict(WHISPER, mul=1e-45),
               dict(WHISPER, range=3e38), dict(pad=REFLECT, center=1), dict(pad=ZEROS, center=0, lengths=LEN)):
        assert rc(probe, **kw) == E_OK, kw


def test_shared_arguments_are_mel_plan_runs(probe):
    """What zflac_hip_mel_run refuses, the new call refuses; what it accepts gives the same grid."""
    shared = [dict(wave=0), dict(dst=0), dict(wave=WAVE + 1), dict(wave=WAVE + 2), dict(wave_frames=1001), dict(frames=0),
              dict(dst_bytes=5 * 80 * 7 * 4 - 1), dict(dtype=F16, dst_bytes=5 * 80 * 7 * 2 - 1),
              dict(rows=1 << 40, frames=1 << 40, dst_bytes=(1 << 64) - 1),
              dict(first=(1 << 63) // 160, dst_bytes=1 << 40), dict(first=(1 << 64) - 1, dst_bytes=1 << 40),
              dict(rows=GRID_MAX + 1, frames=1, bins=1, dst_bytes=1 << 40),
              dict(rows=(GRID_MAX // 2) + 1, frames=129, bins=1, dst_bytes=1 << 50), dict(rows=0, frames=0)]
    for kw in shared:
        for more in (dict(), dict(pad=REFLECT, lengths=LEN, **WHISPER)):
            got = run_ex(probe, **kw, **more)
            assert got[0] == E_INVALID and got[3] == E_INVALID and got[1:3] == [0, 0], (kw, more)
    ok = [dict(wave=WAVE + 4), dict(dst=DST + 1), dict(wave_frames=0, row_stride=0), dict(rows=0),
          dict(dst_bytes=5 * 80 * 7 * 4), dict(first=(1 << 63) // 160 - 7, dst_bytes=1 << 40),
          dict(rows=GRID_MAX, frames=128, bins=1, dst_bytes=1 << 50), dict(rows=GRID_MAX // 2, frames=129, bins=1, dst_bytes=1 << 50)]
    ok += [dict(rows=r, frames=f) for r, f in ((1, 1), (1, 127), (1, 128), (1, 129), (3, 256), (3, 257), (7, 100000))]
    for kw in ok:
        for more in (dict(), dict(pad=REFLECT, lengths=LEN, **WHISPER)):
            got = run_ex(probe, **kw, **more)
            assert got[0] == E_OK and got[:3] == got[3:6], (kw, more)
            tiles = -(-kw.get("frames", 7) // FRAMES)
            assert got[1:3] == [tiles, kw.get("rows", 5) * tiles]
    assert run_ex(probe, rows=0, pad=REFLECT)[:3] == [E_OK, 1, 0]            # no workgroups ...
    assert run_ex(probe, rows=0, pad=REFLECT, center=0)[0] == E_INVALID      # ... but every other check applies
    assert run_ex(probe, rows=0, pad=2)[0] == E_INVALID


def test_two_broken_rules(probe):
    """No rule hides another: a pair of violations is refused whichever check comes first, and fixing
    either one alone still leaves a refusal."""
    rules = [dict(size=103), dict(pad=2), dict(norm=3), dict(reserved=1), dict(reserved2=1), dict(wave=0), dict(frames=0),
             dict(dst_bytes=16), dict(lengths=LEN + 4), dict(row_max=RMAX + 2), dict(range="nan")]
    for i, a in enumerate(rules):
        for b in rules[i + 1:]:
            assert rc(probe, **a, **b) == E_INVALID, (a, b)
    uncentred = dict(pad=REFLECT, center=0)
    triples = [(uncentred, dict(WHISPER, scale=POWER), dict(uncentred, **WHISPER, scale=POWER)),
               (uncentred, dict(WHISPER, row_max=0), dict(uncentred, **dict(WHISPER, row_max=0))),
               (uncentred, dict(lengths=LEN + 1), dict(uncentred, lengths=LEN + 1)),
               (dict(WHISPER, mul=0), dict(WHISPER, range="nan"), dict(WHISPER, mul=0, range="nan")),
               (dict(WHISPER, row_max=0), dict(WHISPER, scale=POWER), dict(WHISPER, row_max=0, scale=POWER))]
    for a, b, both in triples:
        assert rc(probe, **a) == E_INVALID and rc(probe, **b) == E_INVALID and rc(probe, **both) == E_INVALID, (a, b)


def test_size_is_checked_before_the_fields_behind_it(probe):
    for size in (4, 8, 40, 100):
        assert [int(v) for v in probe("short", size).split()] == [E_INVALID, 0, 0]


def test_layout(probe):
    want = [104, 0, 4, 5, 6, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 92, 96, 100]
    assert [int(v) for v in probe("layout").split()] == want


def test_sanitized_probe_gives_the_same_answers(probe):
    """Every case the tests above ran, through the -fsanitize=address,undefined build."""
    exe = _build("mel_run_probe_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    cases = list(probe.ran)
    if not cases:  # (run alone)
        cases = [(["run_ex"], None), (["run_ex", "pad=1", "norm=1", f"row_max={RMAX}", "range=8", "add=4", "mul=0.25"], None),
                 (["run_ex", "size=40"], None), (["short", "8"], "14 0 0\n"), (["layout"], None)]
    for args, out in cases:
        p = subprocess.run([exe, *args], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.stderr[-2000:])
        assert out is None or p.stdout == out, args
