"""The Rice path's exact bit-count edges (tests/rice_edges.py), on streams written from chosen
residuals by tests/craft.py: pair fit, single-code fit, redo isolation, partition geometry,
escapes, long zero runs, bit rate, k_walk_wave's segments and scans, and the writer's other
subframe types, channel assignments and channel counts.

CPU tests hold every case to the oracle (same samples as the writer's PCM, the stated error
name), check each frame's CRC-8 and CRC-16 against bitwise references and its body for
byte-aligned sync patterns, and assert the case's claim through the writer's precondition
model: a case that drifted off its edge does not pass. `gpu` tests decode one batch per family,
twice, under every subframe walk where the family has streams of two or more channels: samples
equal the writer's PCM and the oracle's, device digests equal STREAMINFO's, the kernels and
not the host planner produced them (no sequential stream), in the bucket the streams were
built for."""
import functools

import numpy as np
import pytest

import oracle
import zflac_amd
from zflac_amd import errors

from . import craft, rice_edges
from .test_crc16 import crc16_ref

FAMILIES = rice_edges.FAMILIES
MULTI = ("A", "B", "D", "E", "H", "W")  # families with streams of two or more channels
FAMILY_WALKS = [(n, w) for n in FAMILIES for w in ((None, "lane", "wave") if n in MULTI else (None,))]


@functools.lru_cache(maxsize=None)
def _refs(name: str) -> tuple:
    """The oracle's verdict on every case of a family, computed once."""
    return tuple(oracle.decode(c.cr.flac) for c in rice_edges.family(name))


def crc_bitwise_rows(buf: np.ndarray, spans, poly: int, width: int) -> list:
    """CRC of buf[a:b] for every span, bit by bit (no table), all spans a byte at a time."""
    a = np.array([s[0] for s in spans], np.int64)
    n = np.array([s[1] - s[0] for s in spans], np.int64)
    crc = np.zeros(len(spans), np.uint32)
    top, mask = np.uint32(1 << (width - 1)), np.uint32((1 << width) - 1)
    for j in range(int(n.max())):
        live = n > j
        c = crc[live] ^ (buf[a[live] + j].astype(np.uint32) << np.uint32(width - 8))
        for _ in range(8):
            c = np.where(c & top, (c << np.uint32(1)) ^ np.uint32(poly), c << np.uint32(1)) & mask
        crc[live] = c
    return crc.tolist()


def _crc8_ref(data: bytes) -> int:
    crc = 0
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = ((crc << 1) ^ 0x07) & 0xFF if crc & 0x80 else crc << 1
    return crc


def _header_len(frame: bytes) -> int:
    """Bytes of a fixed-blocking frame header before its CRC-8 (the writer's own layout is not asked)."""
    first, ones = frame[4], 0
    while first & (0x80 >> ones):
        ones += 1
    return 4 + max(ones, 1) + {6: 1, 7: 2}.get(frame[2] >> 4, 0) + {12: 1, 13: 2, 14: 2}.get(frame[2] & 15, 0)


# ---------------------------------------------------------------------------- CPU
def test_bitwise_crc_references():
    assert crc16_ref(b"123456789") == 0xFEE8 and _crc8_ref(b"123456789") == 0xF4
    buf = np.frombuffer(bytes(range(256)) * 3 + b"123456789", np.uint8)
    spans = [(0, 700), (5, 6), (768, 777), (100, 355)]
    assert crc_bitwise_rows(buf, spans, 0x8005, 16) == [crc16_ref(buf[a:b].tobytes()) for a, b in spans]
    assert crc_bitwise_rows(buf, spans, 0x07, 8) == [_crc8_ref(buf[a:b].tobytes()) for a, b in spans]


def test_families_are_complete():
    names = [c.name for n in FAMILIES for c in rice_edges.family(n)]
    assert len(names) == len(set(names)) == 78
    for n in FAMILIES:
        cs = rice_edges.family(n)
        assert all(c.name.startswith(n + "_") and c.claim is not None for c in cs)
        assert any(c.cr.channels >= 2 for c in cs) == (n in MULTI)
        for c in cs:  # whole waves, so no two streams of a batch share one
            assert c.error != "OK" or len(c.cr.layout) % (64 // c.cr.channels) == 0, c.name
        # frames of different lengths: their starts fall on every offset modulo 16 bytes and most modulo 64
        offs = np.concatenate([np.asarray(c.cr.frame_offsets) for c in cs if c.error == "OK"])
        assert len(set((offs % 16).tolist())) == 16 and len(set((offs % 64).tolist())) >= 48, n
    assert {c.name for c in rice_edges.all_cases() if c.error != "OK"} == {"E_escw17_8bit", "F_mono8_q65535",
                                                                           "F_mono8_q65536"}


@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_decodes_what_the_writer_wrote(name):
    """The oracle's samples are the writer's PCM (left-justified as zflac does), its error name
    the case's stated one."""
    for c, r in zip(rice_edges.family(name), _refs(name)):
        assert r.error == c.error, (c.name, r.error)
        if c.error == "OK":
            assert (r.channels, r.bits_per_sample) == (c.cr.channels, c.cr.bps), c.name
            want = c.cr.justified()
            assert r.samples.dtype == want.dtype and r.samples.size == want.size, c.name
            np.testing.assert_array_equal(r.samples, want, err_msg=c.name)


@pytest.mark.parametrize("name", FAMILIES)
def test_frames_are_well_formed(name):
    """Every frame's CRC-8 and CRC-16 equal the bitwise references; no frame holds a byte-aligned
    sync pattern past its own (the device frame scan would take it for a candidate, and the
    stream would be decoded by the host's sequential planner instead of the kernels)."""
    for c in rice_edges.family(name):
        cr = c.cr
        buf = np.frombuffer(cr.flac, np.uint8)
        offs = cr.frame_offsets + [len(cr.flac)]
        hl = [_header_len(cr.flac[a:a + 16]) for a in offs[:-1]]
        got8 = crc_bitwise_rows(buf, [(a, a + h) for a, h in zip(offs, hl)], 0x07, 8)
        assert got8 == [cr.flac[a + h] for a, h in zip(offs, hl)], c.name
        got16 = crc_bitwise_rows(buf, [(a, b - 2) for a, b in zip(offs, offs[1:])], 0x8005, 16)
        assert got16 == [int.from_bytes(cr.flac[b - 2:b], "big") for b in offs[1:]], c.name
        f = len(cr.layout) // 2  # and one frame per case through the scalar references themselves
        fb = cr.frame_bytes(f)
        if len(fb) <= 4096:
            assert crc16_ref(fb[:-2]) == int.from_bytes(fb[-2:], "big") and _crc8_ref(fb[:hl[f]]) == fb[hl[f]], c.name
        assert craft.sync_frames(cr) == [], c.name
        assert all(craft.sync_positions(cr, g) == [] for g in range(0, len(cr.layout), 7)), c.name


@pytest.mark.parametrize("name", FAMILIES)
def test_cases_sit_on_their_edges(name):
    """The precondition model confirms each case's claim."""
    for c in rice_edges.family(name):
        try:
            c.claim()
        except AssertionError as e:
            raise AssertionError(f"{c.name} is not where it claims to be: {e}") from e


def test_model_knows_the_kernel_constants():
    """The model's constants are the kernels' (decode/config.h, decode/run_subframe.h)."""
    import os
    import re

    d = os.path.join(os.path.dirname(zflac_amd.__file__), "csrc", "decode")
    cfg = open(os.path.join(d, "config.h")).read()
    assert int(re.search(r"constexpr int CHUNK = (\d+);", cfg).group(1)) == craft.CHUNK
    assert int(re.search(r"constexpr uint32_t PAIR_KMAX = (\d+);", cfg).group(1)) == craft.PAIR_KMAX
    run = open(os.path.join(d, "run_subframe.h")).read()
    assert "pair_cool = BACKOFF ? 8u << (pair_fail < 4u ? pair_fail : 4u) : 8u;" in run
    assert "L.k < (WALK ? 1u : 2u) || L.k > PAIR_KMAX" in run
    inc = open(os.path.join(os.path.dirname(d), "decode.inc")).read()  # 8- and 16-bit containers: 16 quads = 64 words
    assert re.search(r"#define ZFLAC_RING_Q 16\b", inc) and craft.RING_BITS == 16 * 4 * 32


# ---------------------------------------------------------------------------- GPU
def _read(b, i):
    """(error name, samples or None, device digest) of batch member i."""
    rc, _ = b.info(i)
    if rc:
        return errors.NAMES.get(rc, f"E{rc}"), None, None
    try:
        return "OK", b.read(i, verify_md5=True).samples.values, b.md5(i)
    except errors.ZflacError as e:
        return type(e).__name__, None, None


@pytest.mark.gpu
@pytest.mark.parametrize("name,walk", FAMILY_WALKS, ids=[f"{n}-{w or 'auto'}" for n, w in FAMILY_WALKS])
def test_family_decodes_in_the_kernels(gpu_ready, name, walk):
    """One batch per family, every OK case in it, run twice: bit-exact against the writer's PCM
    and the oracle, device digests equal to STREAMINFO's, no stream handed to the sequential
    planner, and the frame groups classified into the buckets the streams were built for."""
    pairs = [(c, r) for c, r in zip(rice_edges.family(name), _refs(name)) if c.error == "OK"]
    b = zflac_amd.Batch([c.cr.flac for c, _ in pairs], timing=True, device_md5=True, check_crc16=True, walk=walk)
    try:
        for run in range(2):
            b.run()
            bad = []
            for i, (c, r) in enumerate(pairs):
                err, got, md5 = _read(b, i)
                if err != "OK" or r.error != "OK":
                    bad.append((c.name, "error", err, r.error))
                elif got.dtype != r.samples.dtype or not np.array_equal(got, r.samples):
                    bad.append((c.name, "differs from the oracle"))
                elif not np.array_equal(got, c.cr.justified()):
                    bad.append((c.name, "differs from the writer's PCM"))
                elif md5 != c.cr.md5:
                    bad.append((c.name, "device digest"))
            assert not bad, (walk, run, bad[:6], len(bad))
            assert b.timings().sequential_streams == 0, (walk, run)
        used, planned = b.decode_buckets()
        assert used == rice_edges.expected_buckets([c.cr for c, _ in pairs]), (walk, used, planned)
        assert used & ~planned == 0 and b.timings().rest_launches == 0, (walk, used, planned)
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("walk", [None, "lane", "wave"])
def test_error_cases_report_the_oracles_error(gpu_ready, walk):
    """The streams the reader refuses: the same error name as the oracle's, batched and alone."""
    cases = [(c, r) for n in FAMILIES for c, r in zip(rice_edges.family(n), _refs(n)) if c.error != "OK"]
    assert len(cases) == 3
    b = zflac_amd.Batch([c.cr.flac for c, _ in cases], device_md5=True, walk=walk)
    try:
        for run in range(2):
            b.run()
            assert [_read(b, i)[0] for i in range(len(cases))] == [r.error for _, r in cases] == ["OutOfDomain"] * 3
    finally:
        b.close()
    if walk is None:
        for c, r in cases:
            with pytest.raises(errors.ZflacError) as e:
                zflac_amd.decode(c.cr.flac)
            assert type(e.value).__name__ == r.error, c.name
