"""The k_decode instantiation matrix: container kind x layout x history bucket x MIX, 63 kernels.

`cells()` gives, for every (kind, layout, MB, mix), the flacgen configs whose frame groups that
kernel and no other must decode; the sweeps and `every_bucket_stream` cover what the cells hold
fixed (every predictor order, sample depth, Rice parameter, block sizes at or below the order,
and the routing of one stream's groups to all seven launches). A builder module like edges.py:
tests/test_decode_matrix.py holds the assertions.

How a frame group is classified (k_decode, the order-8 launch): the frames of a class (same
container, same channel count) are numbered in batch order and taken 64 / channels at a time;
a group's order is the highest predictor order among the subframes of its frames (LPC 1..32,
fixed 0..4, else 0), and it is MIX when any of them is CONSTANT or VERBATIM. Pure groups go to
the smallest of 4, 8, 12, 16, 32 that holds the order, MIX groups to MIX 8 (order <= 8) or
MIX 32."""
from __future__ import annotations

import functools
import hashlib

import numpy as np

import oracle
import synth
from zflac_amd import _lib

from .util import splice_many

BS = 200                 # six 32-sample chunks + 8 samples; the 8-bit block-size field
N_SAMPLES = BS * 4 + 5   # four full frames and a 5-sample one
KINDS = (0, 1, 2)        # i8, i16, i32 containers
LAYOUTS = {"mono": (1,), "stereo": (2,), "multi": (3, 8)}  # multi: 21 and 8 frames per wave
BUCKETS = ((4, False), (8, False), (12, False), (16, False), (32, False), (8, True), (32, True))
ORDERS = {4: (4, 1), 8: (8, 5), 12: (12, 9), 16: (16, 13), 32: (32, 17)}  # MB: (top, bottom)
MIX_ORDER = {8: 7, 32: 17}
DEPTHS = {0: (4, 8), 1: (9, 12, 16), 2: (17, 24, 32)}
PRECISION = {4: 3, 8: 7, 9: 10, 12: 12, 16: 12, 17: 14, 24: 15, 32: 15}
STEREO_MODES = (1, 8, 9, 10)
FLAVOURS = ("quiet", "loud", "escape", "wasted", "rice2", "edge")
# (kind, channels, MB, mix, flavour) whose seed is moved on: at 4 bits its 5-sample last frame came
# out as one value in some channel, a CONSTANT subframe that would turn a pure cell into a MIX one
# (tests/test_decode_matrix.py checks every pure cell for such blocks)
RESEED = {(0, 8, 32, False, "quiet"): 0x10000}


def bucket_bit(mb: int, mix: bool) -> int:
    return getattr(_lib, f"BUCKET_{'MIX_' if mix else ''}{mb}")


def order_of_type(t: int) -> int:
    """Predictor order of a subframe type (header bits 1..6), as k_decode sizes its history."""
    return t - 31 if t >= 32 else (t - 8 if 8 <= t <= 12 else 0)


def bucket_of_order(order: int) -> int:
    return next(mb for mb in (4, 8, 12, 16, 32) if order <= mb)


def ch0_types(st) -> list:
    """Channel 0's subframe type of every frame, read from the bytes after each frame header."""
    return [(st.flac[synth.header_crc8_index(st.flac, int(off)) + 1] >> 1) & 63 for off in st.frame_offsets]


def _signal(bps: int, flavour: str) -> dict:
    """quiet: the writer's default tones over a noise floor of at most 64 LSB (small Rice
    parameters; scaled down for depths the default would saturate). loud: white-ish noise at a
    quarter of full scale (long codes). The 25..32-bit depths take the existing 32-bit configs'
    floor, so the residual is wider than 16 bits."""
    if flavour == "loud":
        return dict(tone_amp=0.0, noise_lsb=float(2 ** (bps - 3)))
    if bps > 24:
        return dict(tone_amp=0.2, noise_lsb=1e6)
    return dict(tone_amp=0.25, noise_lsb=max(2.0, min(64.0, float(2 ** (bps - 6)))))


def _cell_configs(kind: int, nch: int, mb: int, mix: bool) -> list:
    """Six streams, one per flavour. Stream 0 carries the bucket's top order, stream 1 its
    bottom order; depth and stereo mode rotate with the flavour and the bucket, so that over a
    container's seven cells every flavour meets every depth and mode. The wasted-bits flavour
    keeps the container's widest depth (two of four bits would leave a constant block), and
    `edge` is that depth in mid/side: for i32 stereo the 32-bit stream of the wide form."""
    bi = BUCKETS.index((mb, mix))
    depths = DEPTHS[kind]
    top, bottom = (MIX_ORDER[mb],) * 2 if mix else ORDERS[mb]
    out = []
    for i, fl in enumerate(FLAVOURS):
        bps = depths[-1] if fl in ("wasted", "edge") else depths[(i + bi) % len(depths)]
        c = dict(channels=nch, bps=bps, block_size=BS, n_samples=N_SAMPLES, predictor=synth.FG_LPC,
                 order=bottom if i % 2 else top, precision=PRECISION[bps], max_shift=15,
                 seed=0x0DEC0000 + (kind * 3 + nch) * 1000 + bi * 10 + i + RESEED.get((kind, nch, mb, mix, fl), 0),
                 **_signal(bps, fl))
        if nch == 2:
            c["stereo_mode"] = 10 if fl == "edge" else STEREO_MODES[(i + bi) % 4]
        if fl == "escape":
            c["escape_every"] = 3
        elif fl == "wasted":
            c["wasted_bits"] = 2
        elif fl == "rice2":
            c["rice2"] = 1
        if mix:  # digital silence (CONSTANT) and VERBATIM subframes, alternating over the flavours
            if i % 2 == 0:
                c["silence_every"] = 2
                if nch == 2 and c["stereo_mode"] in (9, 10):  # channel 0 must be the silent left
                    c["stereo_mode"] = 8 if c["stereo_mode"] == 9 else 1
            else:
                c["verbatim_every"] = 3 if nch % 3 else 4  # (every third subframe of 3 channels is channel 0)
        out.append(c)
    return out


def cells() -> dict:
    """(kind, layout, MB, mix) -> one list of configs per batch: one batch for mono and stereo,
    two (3 and 8 channels) for multi. 63 cells, 84 batches."""
    return {(k, lay, mb, mix): [_cell_configs(k, nch, mb, mix) for nch in widths]
            for k in KINDS for lay, widths in LAYOUTS.items() for mb, mix in BUCKETS}


def batch_ids() -> list:
    """(cell key, batch index) of every batch of every cell, in a stable order."""
    return [(key, j) for key, batches in cells().items() for j in range(len(batches))]


def batch_name(key, j) -> str:
    k, lay, mb, mix = key
    return f"k{k}-{lay}{LAYOUTS[lay][j]}-{'mix' if mix else 'mb'}{mb}"


class Decoded:
    """A generated stream with the oracle's verdict, computed once and shared by the tests."""

    def __init__(self, flac: bytes, pcm: np.ndarray, st=None):
        self.flac, self.pcm, self.st = flac, pcm, st
        self.ref = oracle.decode(flac)


def generate(cfgs) -> list:
    return [Decoded(st.flac, st.pcm, st) for st in (synth.generate(**c) for c in cfgs)]


@functools.lru_cache(maxsize=None)
def cell_streams(key, j) -> tuple:
    return tuple(generate(cells()[key][j]))


def md5_pre_justify(v: np.ndarray, bps: int) -> bytes:
    """hashlib MD5 of decoded samples as zflac hashes them: the justify shift undone,
    17..24-bit depths as 3 bytes."""
    js = 16 - bps if 9 <= bps <= 15 else 32 - bps if 17 <= bps <= 31 else 0
    x = v >> js
    if v.dtype == np.int32 and (bps + 7) // 8 == 3:
        return hashlib.md5(np.ascontiguousarray(x.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()).digest()
    return hashlib.md5(x.astype(v.dtype.newbyteorder("<")).tobytes()).digest()


# ---- sweeps: one batch per container, block size 200, five frames ---------------------------
SWEEP_DEPTH = {0: 8, 1: 16, 2: 24}


def _sweep_base(kind: int, nch: int, i: int, bps: int | None = None) -> dict:
    bps = bps or SWEEP_DEPTH[kind]
    c = dict(channels=nch, bps=bps, block_size=BS, n_samples=N_SAMPLES, precision=PRECISION.get(bps, 12),
             seed=0x5EEB0000 + kind * 4096 + nch * 1024 + i, **_signal(bps, "quiet"))
    if nch == 2:
        c["stereo_mode"] = STEREO_MODES[i % 4]
    return c


def order_sweep(kind: int) -> list:
    """Every LPC order 1..32 and fixed order 0..4, mono and stereo."""
    out = []
    for nch in (1, 2):
        for o in range(1, 33):
            out.append(dict(_sweep_base(kind, nch, o), predictor=synth.FG_LPC, order=o))
        for o in range(5):
            out.append(dict(_sweep_base(kind, nch, 40 + o), predictor=synth.FG_FIXED, order=o))
    return out


def depth_sweep(kind: int) -> list:
    """Every depth of the container (4..8, 9..16, 17..32), mono and mid/side stereo."""
    lo, hi = ((4, 8), (9, 16), (17, 32))[kind]
    out = []
    for nch in (1, 2):
        for bps in range(lo, hi + 1):
            c = dict(_sweep_base(kind, nch, bps, bps), order=8, precision=min(12, bps - 1))
            if nch == 2:
                c["stereo_mode"] = 10
            out.append(c)
    return out


def rice_sweep(kind: int) -> list:
    """Forced Rice parameters: 0..14 with the 4-bit parameter, 15..30 with `rice2` as far as the
    container's InterType goes (15 for i8, whose writer stops there), mono and stereo. The noise
    floor is 2**k where the depth has room (k <= depth - 3), so the quotients stay short and the
    low bits are busy; beyond that the codes are all low bits. On i16 k = 1, 2, 9, 10 are the
    limits of the paired-code form."""
    bps = {0: 8, 1: 16, 2: 32}[kind]
    ks = list(range(15)) + (list(range(15, 16)) if kind == 0 else list(range(15, 31)))
    out = []
    for nch in (1, 2):
        for k in ks:
            c = dict(_sweep_base(kind, nch, 100 + k, bps), order=4, precision=PRECISION[bps], rice_k=k,
                     rice2=1 if k >= 15 else 0, partition_order=1 + k % 3, tone_amp=0.0,
                     noise_lsb=float(2 ** min(k, bps - 3)))
            out.append(c)
    return out


BLOCK_ORDER = ((16, 16), (31, 12), (32, 32), (33, 32), (40, 17))


def block_order_sweep(kind: int) -> list:
    """Block sizes at or just above the order: the warm-up fills the whole first chunk. Mono,
    stereo and 3 channels, 70 frames each, so every class has several frame groups."""
    out = []
    for nch in (1, 2, 3):
        for i, (bs, o) in enumerate(BLOCK_ORDER):
            out.append(dict(_sweep_base(kind, nch, 200 + i), block_size=bs, n_samples=bs * 70, predictor=synth.FG_LPC,
                            order=o))
    return out


@functools.lru_cache(maxsize=None)
def sweep_streams(name: str, kind: int) -> tuple:
    return tuple(generate({"order": order_sweep, "depth": depth_sweep, "rice": rice_sweep,
                           "block_order": block_order_sweep}[name](kind)))


# ---- one stream through all seven launches ---------------------------------------------------
EVERY_BUCKET = ((8, False), (4, False), (12, False), (16, False), (32, False), (8, True), (32, True))


@functools.lru_cache(maxsize=None)
def every_bucket_stream(kind: int, layout: str) -> Decoded:
    """One stream whose consecutive frame groups (64 / channels frames each; multi: 3 channels)
    lie in buckets 8, 4, 12, 16, 32, MIX 8, MIX 32, in that order. The host predicts bucket 8
    from the first frame, so the first run decodes the other six through the `rest` launch."""
    nch = LAYOUTS[layout][0]
    F = 64 // nch
    parts = []
    for p, (mb, mix) in enumerate(EVERY_BUCKET):
        bps = SWEEP_DEPTH[kind]
        c = dict(channels=nch, bps=bps, block_size=BS, n_samples=BS * F * len(EVERY_BUCKET), predictor=synth.FG_LPC,
                 order=MIX_ORDER[mb] if mix else ORDERS[mb][0], precision=PRECISION[bps],
                 seed=0xEB000000 + kind * 256 + nch * 16 + p, **_signal(bps, "quiet"))
        if nch == 2:
            c["stereo_mode"] = STEREO_MODES[p % 4]
        if mix:
            c["verbatim_every"] = 3
        parts.append(synth.generate(**c))
    flac, pcm = splice_many(parts, [F * (p + 1) for p in range(len(parts) - 1)])
    return Decoded(flac, pcm)
