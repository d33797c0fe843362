"""Crafted streams for k_crc16 (zflac_amd/csrc/crc16.hip) and a model of how a wave splits a frame.

The kernel gives one wave to a frame. With lo the frame's first byte and hi its trailer's, the wave
cuts the aligned dwords [d0, d1) = [lo / 4, ceil(hi / 4)) into 64 pieces of per = ceil((d1 - d0) / 64)
dwords, a lane hashes the bytes of its piece that lie in [lo, hi), multiplies its remainder by
x^(8 * bytes after the piece) out of a table of squares p[k] = x^(8 * 2^k), and the wave xors the
lanes. `split()` restates that from a frame's offset and length alone and `crc_by_pieces()` computes
the CRC that way in Python; neither looks at anything the kernel computes.

The streams are written with tests/craft.py from VERBATIM and CONSTANT subframes of whole-byte
depths, so a frame's byte count is chosen to the byte (`shape_for`), and behind a PADDING block, so
its offset modulo 4 is chosen too. No sample byte is 0xFF (they are 0x00..0x7E, and a flipped bit
never makes one), so no byte-aligned sync pattern exists outside the real headers (`false_syncs`
checks the finished bytes, trailers included) and the parallel pass certifies every stream.

Every family is a list of `Case`s: a clean stream and bad twins of it, each twin with the one byte
position it differs at. What a twin must decode to without the CRC check is the oracle's business;
with it, FrameCrcMismatch."""
from __future__ import annotations

import dataclasses
import functools
import random

import numpy as np

from . import craft
from .test_crc16 import crc16_ref

P = 0x18005  # x^16 + x^15 + x^2 + 1
LANES = 64
FLIP = 4  # the bit flipped in a sample byte: 0x00..0x7E stays below 0x7F


# ---- arithmetic over GF(2), written for the test (no table, no Horner) ---------------------------
def polymod(a: int) -> int:
    """a(x) mod P by long division."""
    while a.bit_length() > 16:
        a ^= P << (a.bit_length() - 17)
    return a


def mulmod(a: int, b: int) -> int:
    r = 0
    for i in range(b.bit_length()):
        if (b >> i) & 1:
            r ^= a << i
    return polymod(r)


def xpow_by_shifts(n: int) -> int:
    """x^n mod P, one multiplication by x per step."""
    r = 1
    for _ in range(n):
        r <<= 1
        if r & 0x10000:
            r ^= P
    return r


X_ORDER = 32767  # P = (x + 1)(x^15 + x + 1), the second factor primitive: x^32767 = 1 mod P


@functools.lru_cache(maxsize=None)
def pow_entry(k: int) -> int:
    """p[k] = x^(8 * 2^k) mod P without squaring: the exponent reduced by the order of x."""
    return xpow_by_shifts((8 << k) % X_ORDER)


_T0 = [polymod(v << 16) for v in range(256)]


def crc16_fast(data: bytes) -> int:
    """crc16_ref a byte at a time (for the frames of megabytes); pinned against it in the tests."""
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T0[(c >> 8) ^ b]
    return c


# ---- the model of the split --------------------------------------------------------------------
@dataclasses.dataclass
class Split:
    lo: int
    hi: int
    d0: int
    d1: int
    per: int
    pieces: list      # per lane (first byte, one past the last byte) hashed by it; empty: (hi, hi)
    rems: list        # per lane: bytes after its piece
    powers: set       # indices k of p[k] some lane multiplies by

    @property
    def span(self) -> int:
        return self.d1 - self.d0

    @property
    def live(self) -> list:
        return [i for i, (a, b) in enumerate(self.pieces) if b > a]

    @property
    def lane_at_d1(self) -> bool:
        """some lane's piece would start exactly at d1 (an empty piece at the very end)"""
        return any(self.d0 + i * self.per == self.d1 for i in range(LANES))

    @property
    def last_lane_bytes(self) -> int:
        a, b = self.pieces[self.live[-1]]
        return b - a


def split(pos: int, end: int) -> Split:
    """Frame bytes [pos, end), the last two the trailer."""
    lo, hi = pos, end - 2
    assert hi > lo
    d0, d1 = lo // 4, (hi + 3) // 4
    per = (d1 - d0 + LANES - 1) // LANES
    pieces, rems, powers = [], [], set()
    for lane in range(LANES):
        my0 = d0 + lane * per
        my1 = min(my0 + per, d1)
        a, b = (max(lo, 4 * my0), min(hi, 4 * my1)) if my1 > my0 else (hi, hi)
        pieces.append((a, b))
        rems.append(hi - b)
        if b > a:
            powers |= {k for k in range(rems[-1].bit_length()) if (rems[-1] >> k) & 1}
    assert pieces[0][0] == lo and max(b for _, b in pieces) == hi
    assert sum(b - a for a, b in pieces) == hi - lo  # the pieces tile [lo, hi)
    return Split(lo, hi, d0, d1, per, pieces, rems, powers)


def crc_by_pieces(data: bytes, pos: int, end: int, crc=crc16_ref) -> int:
    """The frame's CRC-16 the way the wave computes it: per lane, shifted, xored."""
    s = split(pos, end)
    out = 0
    for (a, b), rem in zip(s.pieces, s.rems):
        c = crc(data[a:b])
        k = 0
        while rem:
            if rem & 1:
                c = mulmod(c, pow_entry(k))
            rem >>= 1
            k += 1
        out ^= c
    return out


# ---- frames of a chosen byte count ---------------------------------------------------------------
def shape_for(hashed: int) -> dict:
    """A frame of exactly `hashed` bytes before its trailer: `const` CONSTANT channels, then `verb`
    VERBATIM channels of `bs` samples of `bps` bits, the block size in a field of `bs_field` bits.
    Header: sync and two parameter bytes (4), a one-byte frame number, the block size, the CRC-8;
    a subframe: one header byte and its samples (CONSTANT: one)."""
    for bps in (8, 16, 24, 32):
        B = bps // 8
        for const in range(1, 9):  # CONSTANT only: 16 samples
            if 7 + const * (1 + B) == hashed:
                return dict(bps=bps, bs=16, verb=0, const=const, bs_field=8)
    for bps in (8, 16, 24, 32):
        B = bps // 8
        for verb in range(1, 9):
            for const in range(0, 9 - verb):
                for hdr, bs_field, top in ((7, 8, 255), (8, 16, 65535)):  # bs 256 in 8 bits: an FF byte
                    rest = hashed - hdr - const * (1 + B) - verb
                    if rest > 0 and rest % (verb * B) == 0 and 16 <= rest // (verb * B) <= top:
                        return dict(bps=bps, bs=rest // (verb * B), verb=verb, const=const, bs_field=bs_field)
    raise ValueError(hashed)


def padded(flac: bytes, k) -> bytes:
    """`flac` (STREAMINFO only, frames at byte 42) with a PADDING block of k zero bytes: the frames
    begin 4 + k bytes later. k None: as it is."""
    if k is None:
        return flac
    d = bytearray(flac[:42])
    assert d[:4] == b"fLaC" and d[4] == 0x80
    d[4] = 0x00
    return bytes(d) + bytes([0x81]) + k.to_bytes(3, "big") + bytes(k) + flac[42:]  # (a 24-bit length)


def unknown_total(flac: bytes) -> bytes:
    """STREAMINFO's 36-bit total set to 0 (unknown), as synth's write_total=0."""
    d = bytearray(flac)
    d[21] &= 0xF0
    d[22:26] = bytes(4)
    return bytes(d)


def false_syncs(data: bytes, frames) -> list:
    """Byte-aligned FF F8 / FF F9 from the first frame on that is not a frame's first byte."""
    b = np.frombuffer(data, np.uint8)
    at = np.flatnonzero((b[:-1] == 0xFF) & ((b[1:] & 0xFE) == 0xF8))
    starts = {a for a, _ in frames}
    return [int(x) for x in at if x >= frames[0][0] and int(x) not in starts]


def flip(data: bytes, pos: int, bit: int = FLIP) -> bytes:
    b = bytearray(data)
    b[pos] ^= 1 << bit
    return bytes(b)


@dataclasses.dataclass
class Stream:
    data: bytes
    frames: list       # (pos, end) of every frame in `data`
    samples: list      # per frame: the byte ranges (a, b) that hold VERBATIM sample bytes
    values: list       # per frame: the byte positions of CONSTANT values' last bytes
    shape: dict

    def split(self, f: int) -> Split:
        return split(*self.frames[f])

    def last_hashed(self, f: int) -> int:
        return self.frames[f][1] - 3

    def is_sample(self, f: int, pos: int) -> bool:
        return any(a <= pos < b for a, b in self.samples[f])

    def is_body(self, f: int, pos: int) -> bool:
        """a byte a single flipped bit changes the decoded samples of, and nothing else"""
        return self.is_sample(f, pos) or pos in self.values[f]


def stream(hashed: int, n_frames: int = 3, seed: int = 1, pad=None, tail_const: bool = False) -> Stream:
    """`n_frames` frames of `hashed` bytes each before the trailer. `tail_const`: every frame after
    the first holds CONSTANT subframes only (a big frame with a tiny one behind it)."""
    sh = shape_for(hashed)
    rng = np.random.default_rng(seed)
    B, bs, ch = sh["bps"] // 8, sh["bs"], sh["verb"] + sh["const"]
    frames = []
    for f in range(n_frames):
        subs = []
        for c in range(ch):
            if c < sh["const"] or (tail_const and f):
                subs.append(craft.Sub(kind="const", samples=[0x21 + c]))
            else:
                by = rng.integers(0, 0x7F, size=(bs, B)).astype(np.int64)  # every byte 0x00..0x7E
                subs.append(craft.Sub(kind="verbatim", samples=sum(by[:, i] << (8 * (B - 1 - i)) for i in range(B))))
        frames.append(subs)
    cr = craft.write(ch, sh["bps"], bs, frames, bs_field=sh["bs_field"])
    return _finish(cr, pad, sh)


def _finish(cr, pad, sh) -> Stream:
    data = padded(cr.flac, pad)
    shift = len(data) - len(cr.flac)
    offs = [o + shift for o in cr.frame_offsets] + [len(data)]
    samples, values = [], []
    for lays in cr.layout:
        samples.append([(int(L.cpos[0]) // 8 + shift, (L.end + 7) // 8 + shift) for L in lays if L.kind == "verbatim"])
        values.append([L.end // 8 - 1 + shift for L in lays if L.kind == "const"])
    return Stream(data, list(zip(offs[:-1], offs[1:])), samples, values, sh)


def stream12(bs: int = 17, n_frames: int = 3, seed: int = 5, pad=None) -> Stream:
    """12-bit mono VERBATIM frames of an odd block size: the last hashed byte ends in four padding
    bits. Samples 0x000..0x3FE with a low byte below 0xFF: no byte of the packed pairs is 0xFF."""
    assert bs % 2 == 1
    rng = np.random.default_rng(seed)
    frames = [[craft.Sub(kind="verbatim", samples=rng.integers(0, 4, bs) * 256 + rng.integers(0, 0xFF, bs))]
              for _ in range(n_frames)]
    return _finish(craft.write(1, 12, bs, frames), pad, dict(bps=12, bs=bs, verb=1, const=0, bs_field=8))


@dataclasses.dataclass
class Case:
    name: str
    st: Stream
    frame: int            # the frame the case is about
    twins: dict           # name -> bytes of a bad twin (differs from st.data in `frame` only)

    @property
    def split(self) -> Split:
        return self.st.split(self.frame)


def pad_for(hashed: int, frame: int, lo_mod: int) -> int:
    """The PADDING size that puts frame `frame` of a stream of equal frames at lo % 4 == lo_mod."""
    lo = 46 + frame * (hashed + 2)
    return (lo_mod - lo) % 4


def _basic_twins(st: Stream, f: int) -> dict:
    last, end = st.last_hashed(f), st.frames[f][1]
    assert st.is_body(f, last)
    return {"last_hashed_byte": flip(st.data, last), "trailer": flip(st.data, end - 1, 3)}


def _case(name: str, hashed: int, lo_mod: int, seed: int, frame: int = 1) -> Case:
    st = stream(hashed, 3, seed, pad_for(hashed, frame, lo_mod))
    return Case(name, st, frame, _basic_twins(st, frame))


@functools.lru_cache(maxsize=None)
def alignment_cases() -> tuple:
    """All 16 (lo % 4, hi % 4) at 6 to 8 dwords and at 75 or more; the smallest legal frame (16
    samples, mono, 8 bits, CONSTANT: 9 hashed bytes, always 3 dwords) at every offset, and one of
    10 hashed bytes at lo % 4 == 3, which straddles into a fourth dword."""
    out = []
    for lo_mod in range(4):
        for hi_mod in range(4):
            for tag, base in (("small", 24), ("large", 300)):
                hashed = base + (hi_mod - lo_mod - base) % 4
                out.append(_case(f"align_{tag}_lo{lo_mod}_hi{hi_mod}", hashed, lo_mod, 100 + 4 * lo_mod + hi_mod))
        out.append(_case(f"align_smallest_lo{lo_mod}", 9, lo_mod, 0))
    out.append(_case("align_10_bytes_lo3", 10, 3, 0))
    return tuple(out)


SPLIT_SPANS = (63, 64, 65, 66, 126, 127, 128, 129, 319, 320, 321)  # per 1 | 2 | 2, 3 | 5, 5, 6


@functools.lru_cache(maxsize=None)
def split_cases() -> tuple:
    """Spans of exactly SPLIT_SPANS dwords, each as whole dwords (lo % 4 == 0, hi % 4 == 0) and with
    one byte in the first and in the last dword (lo % 4 == 3, hi % 4 == 1)."""
    out = []
    for span in SPLIT_SPANS:
        out.append(_case(f"split_{span}_whole", 4 * span, 0, 200 + span))
        out.append(_case(f"split_{span}_ragged", 4 * span - 6, 3, 600 + span))
    return tuple(out)


SHIFT_LENGTHS = (2 ** 15 - 1, 2 ** 15, 2 ** 16, 2 ** 16 + 1, 2 ** 20 + 1, 8 + 8 * (1 + 4 * 65535))


@functools.lru_cache(maxsize=None)
def shift_cases() -> tuple:
    """Hashed lengths around 2^15, 2^16 and 2^20 and the largest VERBATIM frame there is (8 channels
    of 65,535 32-bit samples), each followed by a frame of CONSTANT subframes."""
    out = []
    for i, hashed in enumerate(SHIFT_LENGTHS):
        st = stream(hashed, 2, 300 + i, pad=i % 4, tail_const=True)
        first = st.samples[0][0][0]
        tw = {"first_body_byte": flip(st.data, first), "last_hashed_byte": flip(st.data, st.last_hashed(0))}
        assert st.is_sample(0, st.last_hashed(0))
        out.append(Case(f"shift_{hashed}", st, 0, tw))
    return tuple(out)


COVER_LANES = (0, 1, 31, 32, 62, 63)
COVER_SPANS = (64, 100, 128, 192)  # per 1, 2 (50 lanes), 2, 3; lo % 4 == 1, hi % 4 == 3


def cover_positions(st: Stream, f: int) -> dict:
    """name -> byte position, for the places of the frame a flipped bit must be seen at: those of
    them that are VERBATIM sample bytes (the first pieces of a small frame are its header)."""
    s = st.split(f)
    want = {"first_body_byte": st.samples[f][0][0], "last_hashed_byte": s.hi - 1,
            "last_live_lane_last": s.pieces[s.live[-1]][1] - 1}
    for lane in COVER_LANES:
        a, b = s.pieces[lane]
        if b > a:
            want[f"lane{lane}_first"], want[f"lane{lane}_last"] = a, b - 1
    return {k: p for k, p in want.items() if st.is_sample(f, p)}


@functools.lru_cache(maxsize=None)
def coverage_cases() -> tuple:
    out = []
    for span in COVER_SPANS:
        hashed = 4 * span - 2
        st = stream(hashed, 3, 400 + span, pad_for(hashed, 1, 1))
        out.append(Case(f"cover_{span}", st, 1, {k: flip(st.data, p) for k, p in cover_positions(st, 1).items()}))
    st = stream12(pad=1)
    out.append(Case("cover_padding_bits", st, 1, {"padding_bit": flip(st.data, st.last_hashed(1), 0),
                                                  "last_sample_bit": flip(st.data, st.last_hashed(1), 4)}))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def trailer_case() -> Case:
    """Every single-bit flip of one trailer, and the trailer replaced by 0 and by 0xFFFF."""
    st = stream(301, 3, 77, pad=2)
    end = st.frames[1][1]
    tw = {f"bit{i}": flip(st.data, end - 1 - i // 8, i % 8) for i in range(16)}
    assert st.data[end - 2:end] not in (b"\0\0", b"\xff\xff")
    tw["zero"] = st.data[:end - 2] + b"\0\0" + st.data[end:]
    tw["ones"] = st.data[:end - 2] + b"\xff\xff" + st.data[end:]
    return Case("trailer", st, 1, tw)


# ---- the grid ------------------------------------------------------------------------------------
GRID_COPIES, GRID_FRAMES = 2070, 16   # 33,120 candidates: 352 past the 32,768 waves of the largest grid
GRID_WAVES = 8192 * 4


@functools.lru_cache(maxsize=None)
def grid_streams(variant: int = 0):
    """(clean stream, [bytes per copy], {copy: bad frame}). Copies of one stream of 16 smallest
    frames; a bad trailer in the copies holding candidates 0, 32767, 32768 (variant 1: 32769
    instead), in the last frame of the last copy, and in a dozen copies picked by a fixed seed."""
    st = stream(9, GRID_FRAMES, 0)
    cand = (0, GRID_WAVES - 1, GRID_WAVES + variant, GRID_COPIES * GRID_FRAMES - 1)
    bad = {c // GRID_FRAMES: c % GRID_FRAMES for c in cand}
    rng = random.Random(0xC16)
    while len(bad) < len(cand) + 12:
        bad.setdefault(rng.randrange(GRID_COPIES), rng.randrange(GRID_FRAMES))
    twins = {f: flip(st.data, st.frames[f][1] - 2, 6) for f in set(bad.values())}
    return st, [twins[bad[i]] if i in bad else st.data for i in range(GRID_COPIES)], bad


# ---- streams for the sequential planner ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unknown_total_cases() -> dict:
    """name -> (bytes, bad): crafted frames under an unknown STREAMINFO total, clean and with frame
    2's trailer flipped, as they are and with 3 and 8 bytes of garbage behind the last frame."""
    st = stream(120, 5, 88)
    clean = unknown_total(st.data)
    bad = flip(clean, st.frames[2][1] - 1, 2)
    out = {}
    for tag, tail in (("", b""), ("_garbage3", b"\x11" * 3), ("_garbage8", b"\x11" * 8)):
        out["unknown_clean" + tag] = (clean + tail, False)
        out["unknown_bad" + tag] = (bad + tail, True)
    return out
