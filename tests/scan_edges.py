"""Crafted streams for the frame scan (k_scan, k_compact and candidate_ok: zflac_amd/csrc/scan.hip,
frame_header.h) and a model of where the scan meets each frame start.

A mistake in the scan cannot change a decoded sample: a candidate it misses or invents breaks the
chain k_verify checks, the sequential planner decodes the stream on the host, and the result still
equals the oracle. What it changes is `timings().sequential_streams`. So every case here names the
edge it sits on and whether the parallel pass must certify it (`seq` 0) or the planner must finish
it (`seq` 1), and the GPU half asserts the count exactly.

The model restates the layout rules of pipeline.cpp `alloc_class` and scan.hip, and calls nothing:

  * a stream lies 16-byte aligned in its class's input, so positions relative to the stream's first
    byte keep their residue modulo 16;
  * its chunk grid starts at `frames_begin & ~15` (the grid base) and steps by CHUNK_BYTES; a chunk
    ends at the next grid step or at the stream's end; the first chunk begins at `frames_begin`;
  * inside a chunk, window w = (p - chunk base) // 16 is loaded in round w // SCAN_THREADS by thread
    w % SCAN_THREADS, lane = thread % 64, and the sync code sits at byte b = p % 16 of the window;
  * the 16 bytes after a window come from the next lane's registers (DPP) unless the lane is 63 or
    the next window lies at or past the chunk's end; then they are read from memory.

`parse_header`, `candidate_ok` and `expected_candidates` restate the parser and the filter in
Python (src/zflac.zig:343-407 through frame_header.h); the CPU tests compare them with the compiled
ones (tests/c/scan_probe.cpp).

The frames are written with tests/craft.py: mono VERBATIM (or all-CONSTANT) subframes of whole-byte
depths whose sample bytes are 0x00..0x7E, each frame's byte count chosen to the byte, the header form
chosen per stream, behind a PADDING block that sets `frames_begin`."""
from __future__ import annotations

import dataclasses
import functools
import hashlib

import numpy as np

from . import craft
from .crc16_edges import crc16_fast, padded, unknown_total

CHUNK_BYTES, SCAN_THREADS, SCAN_BYTES_PER_THREAD, CHUNK_CAP = 32768, 256, 128, 64
WINDOW = 16
ROUNDS = SCAN_BYTES_PER_THREAD // WINDOW


# ---- the parser and the filter, restated ----------------------------------------------------------
def crc8(data) -> int:
    c = 0
    for x in data:
        c ^= x
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


@dataclasses.dataclass
class Hdr:
    err: str = ""           # "" or the reader's error before the consistency checks
    bs: int = 0
    rate: int = 0
    hdr_len: int = 0
    chan_code: int = 0
    dcode: int = 0
    byte1: int = 0
    zero_bit: int = 0
    crc_eof: bool = False
    crc_ok: bool = False

    @property
    def nch(self) -> int:
        return self.chan_code + 1 if self.chan_code <= 7 else (2 if self.chan_code <= 10 else 0)


def parse_header(data: bytes, p: int, end: int, si_rate: int) -> Hdr:
    """The header at `p` of a stream that ends at `end`, as zflac's frame loop reads it."""
    avail = end - p
    h = Hdr()
    if avail < 4:
        return dataclasses.replace(h, err="EndOfStream")
    b0, b1, b2, b3 = data[p:p + 4]
    h.byte1, h.chan_code, h.dcode, h.zero_bit = b1, b3 >> 4, (b3 >> 1) & 7, b3 & 1
    if b0 != 0xFF or b1 & 0xFE != 0xF8:
        return dataclasses.replace(h, err="InvalidFrameHeader")
    i = 4
    if avail <= i:
        return dataclasses.replace(h, err="EndOfStream")
    first = data[p + i]
    i += 1
    ones = 0
    while ones < 8 and first & (0x80 >> ones):
        ones += 1
    if first == 0xFF or ones == 1:
        return dataclasses.replace(h, err="InvalidCodedNumber")
    if ones >= 2:
        if avail < i + ones - 1:
            return dataclasses.replace(h, err="EndOfStream")
        i += ones - 1
    bc, rc = b2 >> 4, b2 & 15
    if bc == 0:
        return dataclasses.replace(h, err="InvalidFrameHeader")
    if bc == 6:
        if avail <= i:
            return dataclasses.replace(h, err="EndOfStream")
        h.bs = data[p + i] + 1
        i += 1
    elif bc == 7:
        if avail < i + 2:
            return dataclasses.replace(h, err="EndOfStream")
        v = data[p + i] << 8 | data[p + i + 1]
        i += 2
        if v == 0xFFFF:
            return dataclasses.replace(h, err="InvalidFrameHeader")
        h.bs = v + 1
    else:
        h.bs = 192 if bc == 1 else (144 << bc if bc <= 5 else 1 << bc)
    if rc == 0:
        h.rate = si_rate
    elif rc == 12:
        if avail <= i:
            return dataclasses.replace(h, err="EndOfStream")
        h.rate = data[p + i]
        i += 1
    elif rc in (13, 14):
        if avail < i + 2:
            return dataclasses.replace(h, err="EndOfStream")
        h.rate = (data[p + i] << 8 | data[p + i + 1]) * (10 if rc == 14 else 1)
        i += 2
    elif rc == 15:
        return dataclasses.replace(h, err="InvalidFrameHeader")
    else:
        h.rate = craft.RATE_TABLE[rc]
    h.hdr_len = i + 1
    if avail <= i:
        h.crc_eof = True
        return h
    h.crc_ok = crc8(data[p:p + i]) == data[p + i]
    return h


FILTER_TERMS = ("parse", "crc_eof", "crc8", "zero_bit", "byte1", "channels", "depth", "rate")


def rejected_by(h: Hdr, first: Hdr) -> list:
    """The terms of candidate_ok that `h` fails in a stream whose first frame parsed as `first`."""
    if h.err:
        return ["parse"]
    if h.crc_eof:
        return ["crc_eof"]
    out = []
    if not h.crc_ok:
        out.append("crc8")
    if h.zero_bit:
        out.append("zero_bit")
    if h.byte1 != first.byte1:
        out.append("byte1")
    if h.nch != first.nch:
        out.append("channels")
    if h.dcode != first.dcode:
        out.append("depth")
    if h.rate != first.rate:
        out.append("rate")
    return out


def candidate_ok(h: Hdr, first: Hdr) -> bool:
    return not rejected_by(h, first)


def frames_begin_of(data: bytes) -> int:
    assert data[:4] == b"fLaC"
    p = 4
    while True:
        last, n = data[p] & 0x80, int.from_bytes(data[p + 1:p + 4], "big")
        p += 4 + n
        if last:
            return p


def si_rate_of(data: bytes) -> int:
    return int.from_bytes(data[18:21], "big") >> 4


def si_total_of(data: bytes) -> int:
    return int.from_bytes(data[21:26], "big") & ((1 << 36) - 1)


def sync_codes(data: bytes, lo: int) -> list:
    b = np.frombuffer(data, np.uint8)
    at = np.flatnonzero((b[:-1] == 0xFF) & ((b[1:] & 0xFE) == 0xF8))
    return [int(x) for x in at if x >= lo]


def expected_candidates(data: bytes) -> list:
    """[(position, block size, header length)] of every position from frames_begin on that the
    scan front must take for a candidate: a sync code whose header parses and passes the filter
    against the stream's first frame."""
    fb, rate, end = frames_begin_of(data), si_rate_of(data), len(data)
    first = parse_header(data, fb, end, rate)
    out = []
    for p in sync_codes(data, fb):
        h = parse_header(data, p, end, rate)
        if candidate_ok(h, first):
            out.append((p, h.bs, h.hdr_len))
    return out


# ---- the layout model -----------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Place:
    chunk: int
    round: int
    thread: int
    lane: int
    b: int
    hdr_len: int
    source: str            # of the window after this one: "dpp", "lane", "round", "chunk_end"
    sync_crosses: bool     # 0xFF in byte 15, 0xF8 / 0xF9 in the next window
    header_crosses: bool   # some header byte lies in the next window
    crc8_only_crosses: bool


def grid_base(frames_begin: int) -> int:
    return frames_begin & ~15


def chunk_ranges(frames_begin: int, length: int) -> list:
    """[(begin, end)] of the stream's chunks (alloc_class)."""
    out = []
    a = grid_base(frames_begin)
    while a < length:
        out.append((max(a, frames_begin), min(a + CHUNK_BYTES, length)))
        a += CHUNK_BYTES
    return out


def place(p: int, hdr_len: int, frames_begin: int, length: int) -> Place:
    """Where the scan meets a sync code at `p` (relative to the stream's first byte)."""
    assert frames_begin <= p < length
    rel = p - grid_base(frames_begin)
    chunk = rel // CHUNK_BYTES
    base = grid_base(frames_begin) + chunk * CHUNK_BYTES
    end = min(base + CHUNK_BYTES, length)
    w = (p - base) // WINDOW
    rnd, thread = w // SCAN_THREADS, w % SCAN_THREADS
    lane, b = thread % 64, p % WINDOW
    ws = base + w * WINDOW
    if ws + WINDOW >= end:
        source = "chunk_end"
    elif lane == 63:
        source = "round" if thread == SCAN_THREADS - 1 else "lane"
    else:
        source = "dpp"
    return Place(chunk, rnd, thread, lane, b, hdr_len, source, b == 15, b + hdr_len > WINDOW, b + hdr_len == WINDOW + 1)


def chunk_counts(data: bytes, cands=None) -> list:
    """Candidates per chunk of the stream."""
    cands = expected_candidates(data) if cands is None else cands
    pos = np.asarray([c[0] for c in cands], np.int64)
    return [int(((pos >= a) & (pos < e)).sum()) for a, e in chunk_ranges(frames_begin_of(data), len(data))]


# ---- streams of frames chosen to the byte -----------------------------------------------------------
@dataclasses.dataclass
class Built:
    data: bytes
    frames: list         # (pos, end)
    hdr_lens: list
    samples: list        # per frame (a, b): the bytes of its VERBATIM samples ((0, 0): none)
    pcm: np.ndarray      # what the stream decodes to (as zflac hands it out)
    B: int               # bytes per sample

    @property
    def frames_begin(self) -> int:
        return self.frames[0][0]

    def place(self, f: int) -> Place:
        return place(self.frames[f][0], self.hdr_lens[f], self.frames_begin, len(self.data))

    def frame_at(self, pos: int) -> int:
        return [a for a, _ in self.frames].index(pos)

    def patched(self, patch: dict) -> "Built":
        """Sample bytes replaced ({position: byte}; mono VERBATIM streams): the frames' CRC-16, the
        decoded samples and STREAMINFO's MD5 follow."""
        d = bytearray(self.data)
        for p, v in patch.items():
            assert any(a <= p < b for a, b in self.samples), p
            d[p] = v
        for a, e in self.frames:
            if any(a <= p < e for p in patch):
                d[e - 2:e] = crc16_fast(bytes(d[a:e - 2])).to_bytes(2, "big")
        raw = b"".join(bytes(d[a:b]) for a, b in self.samples)
        pcm = np.frombuffer(raw, {1: ">i1", 2: ">i2"}[self.B]).astype({1: np.int8, 2: np.int16}[self.B])
        d[26:42] = hashlib.md5(pcm.astype({1: "<i1", 2: "<i2"}[self.B]).tobytes()).digest()
        return Built(bytes(d), self.frames, self.hdr_lens, self.samples, pcm, self.B)


def _number_len(n: int) -> int:
    return len(craft._utf8(n))


def make(sizes, *, B: int = 1, nconst: int = 0, const_only: bool = False, bs_field=16, rate: int = 44100,
         rate_code=None, blocking: str = "fixed", first_number: int = 0, pad=None, seed: int = 0,
         known_total: bool = True, bs_table=None) -> Built:
    """A stream whose frame f is exactly sizes[f] bytes. One VERBATIM channel of B-byte samples
    (every sample byte 0x00..0x7E) and `nconst` CONSTANT channels; `const_only`: CONSTANT channels
    alone, 16 samples a frame. The header form comes from `bs_field` (8, 16, or "table" with the
    block size `bs_table` in every frame), `rate_code`, `blocking` and `first_number`."""
    rc = rate_code if rate_code is not None else (9 if rate == 44100 else 0)
    rate_bytes = {12: 1, 13: 2, 14: 2}.get(rc, 0)
    rng = np.random.default_rng(seed)
    ch = nconst + (0 if const_only else 1)
    number, blocks, frames, hdr_lens = first_number, [], [], []
    for size in sizes:
        bsb = 0 if bs_field == "table" else bs_field // 8
        L = 4 + _number_len(number) + bsb + rate_bytes + 1
        body = size - L - 2 - nconst * (1 + B)
        if const_only:
            bs = 16
            assert body == 0, (size, L)
        else:
            assert (body - 1) % B == 0 and body > 1, (size, L)
            bs = (body - 1) // B
        if bs_field == "table":
            assert bs == bs_table, (bs, size)
        subs = [craft.Sub(kind="const", samples=[0x21 + c]) for c in range(nconst)]
        if not const_only:
            by = rng.integers(0, 0x7F, size=(bs, B)).astype(np.int64)
            subs.append(craft.Sub(kind="verbatim", samples=sum(by[:, i] << (8 * (B - 1 - i)) for i in range(B))))
        blocks.append(bs)
        frames.append(subs)
        hdr_lens.append(L)
        number += 1 if blocking == "fixed" else bs
    cr = craft.write(ch, 8 * B, blocks[0] if blocks[0] >= 16 else 16, frames, rate=rate, bs_field=bs_field, rate_code=rate_code,
                     blocking=blocking, first_number=first_number, block_sizes=blocks)
    data = padded(cr.flac, pad)
    if not known_total:
        data = unknown_total(data)
    shift = len(data) - len(cr.flac)
    offs = [o + shift for o in cr.frame_offsets] + [len(data)]
    got = [b - a for a, b in zip(offs[:-1], offs[1:])]
    assert got == list(sizes), (got[:4], list(sizes)[:4])
    samples = []
    for lays in cr.layout:
        v = [L for L in lays if L.kind == "verbatim"]
        samples.append((int(v[0].cpos[0]) // 8 + shift, v[0].end // 8 + shift) if v else (0, 0))
    return Built(data, list(zip(offs[:-1], offs[1:])), hdr_lens, samples, cr.justified(), B)


def pad_for(mod16: int, at_least: int = 0) -> int:
    """The PADDING size that puts frames_begin (46 + k) at `mod16` modulo 16."""
    k = (mod16 - 46) % 16
    while k < at_least:
        k += 16
    return k


def sizes_to(targets, start: int, last: int, lo: int = 40, piece: int = 2000) -> list:
    """Frame sizes such that frames start exactly at `targets` (ascending positions; `start` is
    frames_begin), filler frames of about `piece` bytes in between, and a frame of `last` bytes at
    the end."""
    out, pos = [], start
    for t in targets:
        gap = t - pos
        assert gap == 0 or gap >= lo, (t, pos)
        if gap:
            n = -(-gap // piece)
            base = gap // n
            assert base >= lo
            out += [base] * (n - 1) + [gap - base * (n - 1)]
        pos = t
    return out + [last]


# ---- cases --------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    name: str
    st: Built
    seq: int = 0
    error: str = "OK"      # what the oracle must say
    at: tuple = ()         # the frames (or, for planted headers, positions) the case is about
    extra: tuple = ()      # planted headers: candidates that are no frame starts (the seq 1 controls), or,
                           # in front of frames_begin, headers that must be ignored
    note: str = ""         # cap cases: the candidates per chunk

    @property
    def data(self) -> bytes:
        return self.st.data


# header length -> the form that gives it (20 or so frames: the coded number keeps its length)
LENGTH_FORMS = {
    6: dict(bs_field="table", bs_table=256, nconst=4),
    7: dict(bs_field=8),
    8: dict(bs_field=16),
    9: dict(bs_field=16, rate_code=12, rate=200),
    10: dict(bs_field=16, rate_code=13, rate=44100),
    11: dict(bs_field=16, rate_code=13, rate=65535, first_number=0x80),
    12: dict(bs_field=16, rate_code=14, rate=655350, first_number=0x800),
    13: dict(bs_field=16, rate_code=14, rate=10, first_number=0x10000),
    14: dict(bs_field=16, rate_code=13, rate=1, first_number=0x200000),
    15: dict(bs_field=16, rate_code=14, rate=48000, first_number=0x4000000),
    16: dict(bs_field=16, rate_code=13, rate=32000, first_number=1 << 31, blocking="variable"),
}
LENGTH_FRAMES = 36


@functools.lru_cache(maxsize=None)
def length_cases() -> tuple:
    """byte x length: per header length 6..16 a stream of frames of 1 (mod 16) bytes, so successive
    frame starts step through every byte of a window."""
    out = []
    for L, form in LENGTH_FORMS.items():
        size = 273 if L == 6 else 81 + 16 * (L % 3)
        st = make([size] * LENGTH_FRAMES, seed=L, pad=pad_for(L % 16), **form)
        out.append(Case(f"len{L}", st, at=tuple(range(LENGTH_FRAMES))))
    return tuple(out)


RATE_OF_CODE = {**craft.RATE_TABLE, 12: 255, 13: 65535, 14: 655350}
TABLE_BLOCKS = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, **{k: 1 << k for k in range(8, 16)}}


@functools.lru_cache(maxsize=None)
def form_cases() -> tuple:
    """Every rate code 1..14 and every table block-size code 1..5 and 8..15, three frames each; a
    fixed-blocking stream that ends in a shorter frame; variable blocking with a block size per frame."""
    out = [Case("rate_code0", make([90, 91, 92], rate=12345, seed=99, bs_field=8))]  # (STREAMINFO's rate)
    for rc, rate in RATE_OF_CODE.items():
        out.append(Case(f"rate_code{rc}", make([90, 91, 92], rate=rate, rate_code=rc, seed=rc, bs_field=8)))
    for code, bs in TABLE_BLOCKS.items():
        out.append(Case(f"bs_code{code}", make([6 + 1 + bs + 2] * 3, bs_field="table", bs_table=bs, seed=code)))
    out.append(Case("fixed_short_last", make([300, 300, 300, 57], seed=3)))
    out.append(Case("variable_sizes", make([300, 57, 1200, 64, 4000], blocking="variable", seed=4)))
    out.append(Case("variable_7_byte_numbers", make([300, 57, 1200], blocking="variable", first_number=(1 << 36) - 2000,
                                                    seed=5)))
    return tuple(out)


def _window_pos(fb: int, chunk: int, rnd: int, thread: int, b: int) -> int:
    return grid_base(fb) + chunk * CHUNK_BYTES + (rnd * SCAN_THREADS + thread) * WINDOW + b


SOURCES = {"lane63": (0, 0, 63, "lane"), "lane127": (0, 0, 127, "lane"), "lane191": (0, 0, 191, "lane"),
           "round0": (0, 0, 255, "round"), "round6": (0, 6, 255, "round"), "chunk0_end": (0, 7, 255, "chunk_end")}
SOURCE_L = 8
SOURCE_BYTES = (15, 12, 17 - SOURCE_L)


@functools.lru_cache(maxsize=None)
def source_cases() -> tuple:
    """One frame start per next-window source and byte: the sync code split (b 15), the coded number
    opening the next window (b 12), only the CRC-8 byte crossing (b 17 - header length)."""
    out = []
    for name, (chunk, rnd, thread, _) in SOURCES.items():
        for b in SOURCE_BYTES:
            pad = pad_for((len(name) + b) % 16)
            fb = 46 + pad
            t = _window_pos(fb, chunk, rnd, thread, b)
            sizes = sizes_to([t], fb, 700)
            st = make(sizes, seed=100 + b, pad=pad)
            out.append(Case(f"source_{name}_b{b}", st, at=(st.frame_at(t),)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def chunk_edge_cases() -> tuple:
    out = []
    pad = pad_for(5)
    fb = 46 + pad
    end0 = grid_base(fb) + CHUNK_BYTES
    L = 8
    for name, t in (("first_byte_of_chunk1", end0), ("last_byte_of_chunk0", end0 - 1), ("end_minus_hdr", end0 - L),
                    ("end_minus_hdr_plus1", end0 - L + 1)):
        st = make(sizes_to([t], fb, 300), seed=len(name), pad=pad)
        out.append(Case("edge_" + name, st, at=(st.frame_at(t),)))
    for name, extra in (("exactly_one_chunk", 0), ("one_chunk_and_a_byte", 1)):
        total = grid_base(fb) + CHUNK_BYTES + extra - fb
        st = make(sizes_to([fb + total - 500], fb, 500), seed=7 + extra, pad=pad)
        assert len(st.data) - grid_base(fb) == CHUNK_BYTES + extra
        out.append(Case("edge_" + name, st))
    st = make([401, 2 * 35000 + 11, 401], B=2, seed=9, pad=pad)
    out.append(Case("edge_frame_over_two_chunks", st))
    return tuple(out)


def _planted_header(number: int = 0) -> bytes:
    """A complete 6-byte header of a mono 8-bit 44.1 kHz stream (block-size code 8), CRC-8 right."""
    h = bytes([0xFF, 0xF8, 0x89, 0x02, number])
    return h + bytes([crc8(h)])


@functools.lru_cache(maxsize=None)
def first_chunk_cases() -> tuple:
    """frames_begin at every residue modulo 16; and, where the window in front of it has room, a
    complete valid header in the metadata bytes of that window (ignored: before ch.begin)."""
    out = []
    for m in range(16):
        st = make([100, 101, 102, 103], seed=m, pad=pad_for(m), bs_field=8)
        assert st.frames_begin % 16 == m
        out.append(Case(f"first_fb{m}", st, at=(0,)))
        if m >= 6:
            k = pad_for(m, 16)
            st = make([100, 101, 102, 103], seed=m, pad=k, bs_field=8)
            fb = st.frames_begin
            d = bytearray(st.data)
            spots = ([grid_base(fb)] if m >= 12 else []) + [fb - 6]  # (two where both fit)
            for at in spots:
                d[at:at + 6] = _planted_header(3)
            out.append(Case(f"first_fb{m}_planted", dataclasses.replace(st, data=bytes(d)), at=(0,), extra=tuple(spots)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def end_cases() -> tuple:
    """Known total: the last frame ends on the stream's last byte at four residues of the length;
    a stream cut inside its last, 16-byte header at each of its bytes 4..15."""
    out = []
    for mod in (1, 8, 15, 0):
        fb = 46 + pad_for(3)
        last = 200 + (mod - (fb + 3 * 150 + 200)) % 16
        st = make([150, 150, 150, last], seed=mod, pad=pad_for(3))
        assert len(st.data) % 16 == mod
        out.append(Case(f"end_len_mod{mod}", st, at=(3,)))
    form = LENGTH_FORMS[16]
    whole = make([150, 150, 150, 150], seed=21, pad=pad_for(9), **form)
    assert whole.hdr_lens[3] == 16
    for cut in range(4, 16):
        st = dataclasses.replace(whole, data=whole.data[:whole.frames[3][0] + cut])
        out.append(Case(f"end_cut_at_header_byte{cut}", st, seq=1, error="EndOfStream", at=(3,)))
    return tuple(out)


def with_trailer(st: Built, f: int, target: int) -> Built:
    """Frame f's last three sample bytes chosen (within 0x00..0x7E) so that its CRC-16 is `target`.
    The CRC is linear (initial value 0): changing byte i by d xors CRC(d, then the bytes after i as
    zeros) into it, so two bytes are tabulated and the third is looked up."""
    a, e = st.frames[f]
    at = [st.samples[f][1] - 1 - k for k in range(3)]
    assert e - 2 == st.samples[f][1]
    need = crc16_fast(st.data[a:e - 2]) ^ target
    tabs = [[crc16_fast(bytes([st.data[p] ^ b]) + bytes(e - 3 - p)) for b in range(0x7F)] for p in at]
    two = {x ^ y: (i, j) for i, x in enumerate(tabs[0]) for j, y in enumerate(tabs[1])}
    for k, z in enumerate(tabs[2]):
        if need ^ z in two:
            i, j = two[need ^ z]
            out = st.patched(dict(zip(at, (i, j, k))))
            assert int.from_bytes(out.data[e - 2:e], "big") == target
            return out
    raise ValueError(target)


NEAR_MISSES = ((0x00, 0xFF), (0xFF, 0x00), (0xF8, 0xFF), (0xFF, 0xF7), (0xFF, 0xFA))


@functools.lru_cache(maxsize=None)
def neighbour_cases() -> tuple:
    out = []
    # the previous frame's CRC-16 ends in 0xFF: FF | FF F8
    for seed in range(4000):
        st = make([60, 61, 62], seed=seed, bs_field=8)
        if st.data[st.frames[1][0] - 1] == 0xFF:
            out.append(Case("crc16_low_byte_ff", st, at=(1,)))
            break
    # the trailer itself reads FF F8 / FF F9, in front of a real sync code
    for target in (0xFFF8, 0xFFF9):
        st = with_trailer(make([70, 71, 72], seed=target, bs_field=8, pad=pad_for(target % 16)), 1, target)
        out.append(Case(f"trailer_{target:04x}", st, at=(2,)))
    # a real header with 0xFF as its block-size field (256 samples in 8 bits), in front of the CRC-8
    st = make([7 + 1 + 256 + 2] * 18, seed=2, bs_field=8, pad=pad_for(1))
    assert all(st.data[a + 5] == 0xFF for a, _ in st.frames)
    out.append(Case("bs_field_ff", st, at=tuple(range(18))))
    # near misses across every dword and window boundary, lane 63 and a chunk's end included
    pad = pad_for(0)
    fb = 46 + pad
    for i, (x, y) in enumerate(NEAR_MISSES):
        st = make([4000] * 9, seed=3 + i, pad=pad)
        patch = {}
        for j, at in enumerate((3, 7, 11, 15)):  # the pair straddles byte `at` | `at` + 1 of a window
            w = grid_base(fb) + (40 + 2 * j) * WINDOW
            patch[w + at], patch[w + at + 1] = x, y
        for w in (_window_pos(fb, 0, 0, 63, 0), _window_pos(fb, 0, 1, 255, 0), _window_pos(fb, 0, 7, 255, 0)):
            patch[w + 15], patch[w + 16] = x, y  # lane 63 | 64, round 1 | 2, chunk 0 | 1
        out.append(Case(f"near_miss_{x:02x}_{y:02x}", st.patched(patch), at=tuple(sorted(patch))))
    return tuple(out)


# the planted false headers of a mono 16-bit stream (true header: FF F8 79 08 nn bb bb crc): what
# follows the sync code, and the only filter term it fails
def _false_headers(byte1: int) -> dict:
    other = byte1 ^ 1
    good = [0xFF, byte1, 0x79, 0x08, 0x05, 0x01, 0x2B]
    forms = {
        "control": (good, None),
        "crc8": (good, "flip"),
        "zero_bit": ([0xFF, byte1, 0x79, 0x09, 0x05, 0x01, 0x2B], None),
        "byte1": ([0xFF, other] + good[2:], None),
        "channels": ([0xFF, byte1, 0x79, 0x18, 0x05, 0x01, 0x2B], None),
        "depth": ([0xFF, byte1, 0x79, 0x02, 0x05, 0x01, 0x2B], None),
        "rate": ([0xFF, byte1, 0x7A, 0x08, 0x05, 0x01, 0x2B], None),
        "parse_bs_code0": ([0xFF, byte1, 0x09, 0x08, 0x05], None),
        "parse_rate_code15": ([0xFF, byte1, 0x7F, 0x08, 0x05, 0x01, 0x2B], None),
        "parse_number_ff": ([0xFF, byte1, 0x79, 0x08, 0xFF, 0x01, 0x2B], None),
        "parse_number_10xxxxxx": ([0xFF, byte1, 0x79, 0x08, 0x85, 0x01, 0x2B], None),
        "parse_bs_ffff": ([0xFF, byte1, 0x79, 0x08, 0x05, 0xFF, 0xFF], None),
    }
    out = {}
    for name, (h, how) in forms.items():
        c = crc8(h)
        out[name] = bytes(h + [c ^ 0x10 if how == "flip" else c])
    return out


FILTER_PLACES = {"b3": (0, 0, 20, 3), "b15_lane63": (0, 0, 63, 15)}


@functools.lru_cache(maxsize=None)
def filter_cases() -> tuple:
    """A complete false header with a right CRC-8 in the samples of a 16-bit VERBATIM frame, failing
    exactly one term of candidate_ok (seq 0); the control fails none (seq 1). In an F8 stream and,
    for the blocking byte, in an F9 stream; at b 3 on an interior lane and at b 15 on lane 63."""
    out = []
    for blocking, byte1 in (("fixed", 0xF8), ("variable", 0xF9)):
        for term, fake in _false_headers(byte1).items():
            if blocking == "variable" and term not in ("control", "byte1"):
                continue
            for where, (chunk, rnd, thread, b) in FILTER_PLACES.items():
                pad = pad_for(7)
                fb = 46 + pad
                # (variable blocking: frame 1's number is frame 0's block size, two bytes)
                st = make([1401, 1301 + (blocking == "variable")], B=2, seed=len(term), pad=pad, blocking=blocking)
                at = _window_pos(fb, chunk, rnd, thread, b)
                st = st.patched({at + i: v for i, v in enumerate(fake)})
                tag = f"filter_{term}_{where}" + ("_f9" if blocking == "variable" else "")
                out.append(Case(tag, st, seq=int(term == "control"), at=(at,), extra=(at,) if term == "control" else ()))
    return tuple(out)


def _cap_stream(sizes, seed, **kw) -> Built:
    return make(sizes, seed=seed, pad=pad_for(0), **kw)  # frames_begin 48: the grid base itself


@functools.lru_cache(maxsize=None)
def cap_cases() -> tuple:
    """Chunks of 63, 64 and 65 candidates and far more (CHUNK_CAP is 64): the sorted LDS slots
    against the ordered rescan of an overflowed chunk, and the output offsets behind one."""
    fb = 46 + pad_for(0)
    assert fb % 16 == 0
    full = [512] * 64                      # one chunk, 64 candidates
    many = [256] * 128                     # one chunk, 128
    out = [
        Case("cap_64", _cap_stream(full + [512] * 3, 1), note="64,3"),
        Case("cap_63", _cap_stream([1024] + [512] * 62 + [512] * 3, 2), note="63,3"),
        Case("cap_65", _cap_stream([512] * 63 + [256, 256] + [512] * 3, 3), note="65,3"),
        Case("cap_65th_in_last_window", _cap_stream([512] * 63 + [506, 518] + [512] * 2, 4), note="65,2"),
        Case("cap_overflow_between_ordinary", _cap_stream(full + many + full + [300], 5), note="64,128,64,1"),
        Case("cap_four_overflowed_in_a_row", _cap_stream(full + many * 4 + full + [300], 6), note="64,128,128,128,128,64,1"),
    ]
    n = 0  # the smallest frame: 11 bytes while its number takes one byte, 12 and 13 after that
    sizes = []
    while sum(sizes) < CHUNK_BYTES + 600:
        sizes.append(10 + _number_len(n))
        n += 1
    out.append(Case("cap_smallest_frames", make(sizes, const_only=True, nconst=1, bs_field=8, pad=pad_for(0)),
                    note="smallest"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cap_beside_cases() -> tuple:
    """Four one-chunk streams of one class in a row (one k_compact workgroup): the second overflowed."""
    return (Case("beside_0", _cap_stream([512] * 20, 11)), Case("beside_1_overflowed", _cap_stream([128] * 200, 12)),
            Case("beside_2", _cap_stream([700] * 9, 13)), Case("beside_3", _cap_stream([512] * 64, 14)))


@functools.lru_cache(maxsize=None)
def unknown_total_cases() -> tuple:
    """STREAMINFO total 0: zflac reads frames until fewer than 4 bytes are left (k_verify:
    c_end + 4 > in_end ends the chain), so 1..3 bytes of garbage are never read and 4 are a header."""
    st = make([150, 151, 152, 153, 154], seed=31, pad=pad_for(11), known_total=False)
    out = [Case("unknown_ends_at_last_byte", st)]
    for n in (1, 2, 3):
        out.append(Case(f"unknown_garbage{n}", dataclasses.replace(st, data=st.data + b"\x11" * n)))
    out.append(Case("unknown_garbage4", dataclasses.replace(st, data=st.data + b"\x11" * 4), seq=1,
                    error="InvalidFrameHeader"))
    return tuple(out)


def families() -> dict:
    return {"length": length_cases(), "forms": form_cases(), "source": source_cases(), "chunk_edges": chunk_edge_cases(),
            "first_chunk": first_chunk_cases(), "end": end_cases(), "neighbours": neighbour_cases(),
            "filter": filter_cases(), "cap": cap_cases(), "cap_beside": cap_beside_cases(),
            "unknown_total": unknown_total_cases()}


# the families whose streams are fixed-blocking with a known total in every case (also run with front="hop")
HOP_FAMILIES = ("source", "chunk_edges", "first_chunk", "neighbours", "cap", "cap_beside")
