"""Which lanes of a write-back row store (zflac::row_lane_mask, csrc/decode/row_mask.h): the
function the 16-bit kernels run at every chunk start, built for the host as a program of its own
(tests/c/row_mask_probe.cpp, with the address and undefined-behaviour sanitizers) and compared
with a plain model of the output stage's lane layout (Stage in csrc/decode/pcm_stage.h):

* stereo: 32 frames a wave, row t = frames 8t..8t+7, lane L a piece of frame 8t + L // 8;
* mono: 64 frames a wave, row t = frames 16t..16t+15, lane L a piece of frame 16t + L // 4.

A lane stores exactly when its frame's bit is set in the stage's frame mask."""
from __future__ import annotations

import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zflac_amd", "csrc")


@pytest.fixture(scope="module")
def probe():
    src = os.path.join(ROOT, "tests", "c", "row_mask_probe.cpp")
    hdr = os.path.join(CSRC, "decode", "row_mask.h")
    exe = os.path.join(ROOT, "tests", "c", "_build", "row_mask_probe")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe])
    return exe


def model(mono: bool, frames: int, row: int) -> int:
    """Stage's lane layout, lane by lane."""
    pieces = 4 if mono else 8        # 16-byte pieces (lanes) per frame
    row_frames = 64 // pieces
    out = 0
    for lane in range(64):
        frame = row * row_frames + lane // pieces
        if (frames >> frame) & 1:
            out |= 1 << lane
    return out


def masks(mono: bool):
    n = 64 if mono else 32
    full = (1 << n) - 1
    rng = random.Random(20 + mono)
    alt = int("01" * (n // 2), 2)
    return ([full, 0, alt, full ^ alt] + [1 << i for i in range(n)] + [full ^ (1 << i) for i in range(0, n, 7)] +
            [rng.getrandbits(n) for _ in range(64)])


@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
def test_row_lane_mask_matches_the_stage_layout(probe, mono):
    cases = [(m, t) for m in masks(mono) for t in range(4)]
    text = "".join(f"{int(mono)} {t} {m:x}\n" for m, t in cases)
    r = subprocess.run([probe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [int(x, 16) for x in r.stdout.split()]
    assert len(got) == len(cases)
    for (m, t), g in zip(cases, got):
        assert g == model(mono, m, t), (hex(m), t, hex(g))


@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
def test_rows_partition_the_frames(probe, mono):
    """Every frame's lanes belong to exactly one row: over the four rows the lane masks of a
    frame mask hold (lanes per frame) x (frames set) bits."""
    ms = masks(mono)
    text = "".join(f"{int(mono)} {t} {m:x}\n" for m in ms for t in range(4))
    r = subprocess.run([probe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [int(x, 16) for x in r.stdout.split()]
    for i, m in enumerate(ms):
        assert sum(bin(g).count("1") for g in got[4 * i:4 * i + 4]) == (4 if mono else 8) * bin(m).count("1")
