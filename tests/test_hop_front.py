"""The hop front on the GPU (k_hop, zflac_amd/csrc/hop.hip): the frame table of a class found by
hopping from header to header. Every case runs the same batch with the front forced to `hop` and
to `scan`, compares both with the oracle (samples and error names) and with each other, and
asserts what zflac_hip_batch_front reports. The front must never change a result."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import oracle
import synth
import zflac_amd
from zflac_amd import _lib, errors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN, HOP = _lib.FRONT_SCAN, _lib.FRONT_HOP
WINDOW, LANE = 1024, 64  # k_hop's probe window and a lane's piece of it (hop.hip)

LPC8 = dict(channels=2, bps=16, stereo_mode=10, predictor=synth.FG_LPC, order=8, precision=12, max_shift=12,
            partition_order=4)
FIXED2 = dict(channels=1, bps=16, predictor=synth.FG_FIXED, order=2, partition_order=0, rice_k=4, noise_lsb=4.5,
              tone_amp=0.05)
VERBATIM = dict(channels=1, bps=16, predictor=synth.FG_VERBATIM)

_ORACLE: dict = {}


def ref(data: bytes):
    if data not in _ORACLE:
        _ORACLE[data] = oracle.decode(data)
    return _ORACLE[data]


def gpu_result(b, i):
    """(error name, samples or None) of batch member i, samples also on InvalidChecksum."""
    rc, _ = b.info(i)
    if rc:
        return errors.NAMES.get(rc, f"E{rc}"), None
    d = b.read(i, verify_md5=False)
    try:
        b.read(i, verify_md5=True)
        return "OK", d.samples.values
    except errors.ZflacError as e:
        return type(e).__name__, d.samples.values


def run(streams, front, runs=1):
    """Per run: ([(error, samples)], (planned, used), streams the sequential planner finished)."""
    b = zflac_amd.Batch(streams, timing=True, front=front)
    out = []
    try:
        for _ in range(runs):
            b.run()
            out.append(([gpu_result(b, i) for i in range(len(streams))], b.front(), b.timings().sequential_streams))
    finally:
        b.close()
    return out


def check(streams, hop_fronts, scan_fronts=(SCAN, SCAN), runs=1):
    """Both fronts against the oracle and each other; `hop_fronts`: (planned, used) expected of
    each run of the batch forced to hop. Returns the hop batch's runs."""
    hop, scan = run(streams, "hop", runs), run(streams, "scan")
    assert scan[0][1] == tuple(scan_fronts)
    assert [r[1] for r in hop] == [tuple(f) for f in hop_fronts]
    for res, _, _ in hop + scan:
        for i, (data, (err, samples)) in enumerate(zip(streams, res)):
            r = ref(data)
            assert err == r.error, (i, err, r.error)
            if r.samples is not None and samples is not None:
                np.testing.assert_array_equal(samples, r.samples, err_msg=str(i))
            assert (samples is None) == (r.samples is None or err not in ("OK", "InvalidChecksum")), i
    for (e1, s1), (e2, s2) in zip(hop[0][0], scan[0][0]):
        assert e1 == e2 and (s1 is None) == (s2 is None) and (s1 is None or np.array_equal(s1, s2))
    return hop


def gen(n_samples, seed, **kw):
    return synth.generate(**dict(kw, n_samples=n_samples, seed=seed))


# ------------------------------------------------------------------ the test's header tools
def crc8(b: bytes) -> int:
    c = 0
    for x in b:
        c ^= x
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def coded(n: int) -> bytes:
    if n < 0x80:
        return bytes([n])
    for k, bits in ((2, 11), (3, 16), (4, 21), (5, 26), (6, 31)):
        if n < 1 << bits:
            cont = [(0x80 | ((n >> (6 * i)) & 0x3F)) for i in range(k - 1)][::-1]
            return bytes([((0xFF << (8 - k)) & 0xFF) | (n >> (6 * (k - 1)))] + cont)
    raise ValueError(n)


def renumbered(st, frame: int, number: int) -> bytes:
    """The header of `frame` with another coded number (same length), CRC-8 fixed up."""
    off = int(st.frame_offsets[frame])
    end = synth.header_crc8_index(st.flac, off)
    old = st.flac[off:end]
    new = old[:4] + coded(number) + old[4 + len(coded(frame)):]
    assert len(new) == len(old)
    return new + bytes([crc8(new)])


def with_bytes(data: bytes, off: int, patch: bytes) -> bytes:
    return data[:off] + patch + data[off + len(patch):]


def padded(st, k: int) -> bytes:
    """`st` with a PADDING block of k bytes after STREAMINFO: the frames begin 4 + k bytes later."""
    d = bytearray(st.flac[:st.frames_begin])
    assert d[:4] == b"fLaC" and d[4] == 0x80 and st.frames_begin == 42
    d[4] = 0x00
    return bytes(d) + bytes([0x81, 0, 0, k]) + bytes(k) + st.flac[st.frames_begin:]


def first_window_offsets(frames_begin: int, frame_offsets, length: int):
    """Where k_hop's first window of each hop finds the next header, in bytes from the window's
    start (hop.hip: the window starts 512 bytes before position + guess, 16-byte aligned against
    the stream's 16-byte aligned base, never before the current header; the guess is the previous
    frame's size, at first frame bytes / frames)."""
    ab = frames_begin & ~15
    rel = [int(o) - ab for o in frame_offsets]
    guess = (length - frames_begin) // len(rel)
    out = []
    for cur, nxt in zip(rel, rel[1:]):
        ws0 = max((cur + guess - WINDOW // 2) & ~15, (cur + 1) & ~15)
        out.append(nxt - ws0)
        guess = nxt - cur
    return out


# ---------------------------------------------------------------------------------- cases
def test_plain(gpu_ready):
    """Stereo LPC-8 and mono fixed-2 (two classes), full and short last frames, one-frame streams,
    block sizes 16 to 4,096."""
    sts = [gen(4096 * 5, 1, block_size=4096, **LPC8), gen(4096 * 3 + 1000, 2, block_size=4096, **LPC8),
           gen(1024 * 7 + 33, 3, block_size=1024, **LPC8), gen(1024 * 40, 4, block_size=1024, **LPC8),
           gen(700, 5, block_size=4096, **LPC8), gen(4096, 6, block_size=4096, **LPC8),
           gen(256 * 40, 7, block_size=256, **FIXED2), gen(256 * 9 + 5, 8, block_size=256, **FIXED2),
           gen(100, 9, block_size=256, **FIXED2), gen(16 * 30 + 1, 10, block_size=16, **FIXED2),
           gen(4096 * 2 + 1, 11, block_size=4096, **FIXED2), gen(16, 12, block_size=16, **FIXED2)]
    hop = check([s.flac for s in sts], [(HOP, HOP)])
    assert hop[0][2] == 0  # every stream certified by the parallel pass
    assert all(ref(s.flac).error == "OK" for s in sts)


def test_size_jumps(gpu_ready):
    """Silent (constant subframes, ~15 bytes) and loud frames alternate, so every guess is off by
    several windows, one way and then the other."""
    sts = [gen(bs * 9 + extra, 20 + i, block_size=bs, silence_every=2, **dict(LPC8, stereo_mode=1, noise_lsb=64.0))
           for i, (bs, extra) in enumerate([(2048, 0), (2048, 77), (4096, 0), (4096, 5), (1024, 0), (4096, 4000),
                                            (2048, 2047), (4096, 1)])]
    for s in sts:
        sizes = np.diff([int(x) for x in s.frame_offsets] + [len(s.flac)])
        assert sizes.max() - sizes.min() > WINDOW, sizes
        assert min(abs(int(a) - int(b)) for a, b in zip(sizes[:-2], sizes[1:-1])) > WINDOW, sizes
    hop = check([s.flac for s in sts], [(HOP, HOP)])
    assert hop[0][2] == 0


def test_window_edge(gpu_ready):
    """Verbatim mono streams of two frames whose sizes differ by about a window, each behind 0..15
    bytes of padding: by the model of the hop's first window (first_window_offsets) the batch
    holds a sync code on the last byte of the window (its header in the next window's bytes), on
    the last byte of a lane's 64-byte piece and on the last byte of a 16-byte load."""
    chosen, hits = [], {}
    wanted = {"window": lambda o: o == WINDOW - 1, "lane": lambda o: 0 <= o < WINDOW and o % LANE == LANE - 1,
              "load": lambda o: 0 <= o < WINDOW and o % 16 == 15 and o % LANE != LANE - 1,
              "tail": lambda o: WINDOW - 8 <= o < WINDOW - 1}
    for short in range(480, 560):  # the second header lies about 1,536 - short bytes into the window
        st = gen(1024 + short, 30, block_size=1024, **VERBATIM)
        for k in range(16):
            data = padded(st, k)
            (o,) = first_window_offsets(st.frames_begin + 4 + k, [int(x) + 4 + k for x in st.frame_offsets], len(data))
            for name, fn in wanted.items():
                if fn(o) and hits.get(name, 0) < 4:
                    hits[name] = hits.get(name, 0) + 1
                    chosen.append(data)
    assert set(hits) == set(wanted) and 8 <= len(chosen) <= 16, hits
    hop = check(chosen, [(HOP, HOP)])
    assert hop[0][2] == 0


def test_multi_byte_frame_numbers(gpu_ready, monkeypatch):
    """2,100 frames of 16 samples: coded numbers of 1, 2 and 3 bytes (128 and 2,048 on)."""
    monkeypatch.setenv("ZFLAC_HOP_MAX_FRAMES", "4096")
    st = gen(16 * 2100, 40, block_size=16, **FIXED2)
    assert len(st.frame_offsets) == 2100
    assert len(coded(2099)) == 3 and st.flac[int(st.frame_offsets[2099]) + 4:][:3] == coded(2099)
    hop = check([st.flac], [(HOP, HOP)])
    assert hop[0][2] == 0


def _planted(st, frame: int, number: int, before: int) -> bytes:
    """A copy of `frame`'s header numbered `number` (CRC-8 valid) `before` bytes ahead of the next
    frame, inside `frame`'s verbatim samples."""
    fake = renumbered(st, frame, number)
    at = int(st.frame_offsets[frame + 1]) - before
    assert at > synth.header_crc8_index(st.flac, int(st.frame_offsets[frame])) + 8
    return with_bytes(st.flac, at, fake)


def test_false_header_wrong_number(gpu_ready):
    """A well-formed header with another frame's number inside a frame: the hop passes over it
    and the table is the true chain (the scan front takes it for a candidate and needs the planner)."""
    sts = [gen(512 * 6, 50 + i, block_size=512, **VERBATIM) for i in range(8)]
    data = [s.flac for s in sts]
    data[2] = _planted(sts[2], 3, 9, 100)
    data[5] = _planted(sts[5], 0, 3, 40)
    hop = check(data, [(HOP, HOP)])
    assert hop[0][2] == 0


def test_false_header_right_number(gpu_ready):
    """A well-formed header with the wanted number ahead of the true one: the hop takes it, the
    chain check rejects the stream and the sequential planner finishes it, as under the scan front."""
    sts = [gen(512 * 6, 60 + i, block_size=512, **VERBATIM) for i in range(8)]
    data = [s.flac for s in sts]
    data[4] = _planted(sts[4], 2, 3, 120)
    hop = check(data, [(HOP, HOP)])
    assert hop[0][2] == 1


def test_broken_numbering(gpu_ready):
    """One stream whose frame 3 is numbered 9 (zflac never looks): the hop loses it, the class is
    redone with the scan front and stays there."""
    sts = [gen(1024 * 6 + 5, 70 + i, block_size=1024, **LPC8) for i in range(8)]
    data = [s.flac for s in sts]
    off = int(sts[3].frame_offsets[3])
    data[3] = with_bytes(sts[3].flac, off, renumbered(sts[3], 3, 9))
    assert ref(data[3]).error == "OK"
    hop = check(data, [(HOP, SCAN), (SCAN, SCAN)], runs=2)
    assert hop[0][2] == hop[1][2] == 0


def crc16(b: bytes) -> int:
    c = 0
    for x in b:
        c ^= x << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


def stream_of_blocks(pcm: np.ndarray, block: int, sizes) -> bytes:
    """Mono verbatim frames of `sizes` samples, numbered 0, 1, 2, ..., under the metadata of the
    same PCM written in blocks of `block` (STREAMINFO min block == max block == block, the total
    and the MD5 of the PCM): a stream zflac decodes to `pcm` whatever the sizes are."""
    assert sum(sizes) == pcm.size
    meta = synth.generate(pcm=pcm, block_size=block, **VERBATIM)
    out, at = meta.flac[:meta.frames_begin], 0
    for i, n in enumerate(sizes):
        one = synth.generate(pcm=pcm[at:at + n], block_size=n, **VERBATIM)
        assert len(one.frame_offsets) == 1
        frame = one.flac[one.frames_begin:]
        hdr = renumbered(one, 0, i)
        frame = hdr + frame[len(hdr):-2]
        out += frame + crc16(frame).to_bytes(2, "big")
        at += n
    return out


def test_block_size_differs_mid_stream(gpu_ready):
    """Fixed-blocking metadata and frame numbers in order, but one frame in the middle codes half
    the block and one more frame makes up for it. zflac never looks at numbers or at STREAMINFO's
    block sizes and decodes the frames one after the other; a table that places frame i at i x
    block would leave a gap and shift the rest. The hop must lose such a stream (the class is
    redone with the scan front) and the samples equal the oracle's and the scan front's."""
    rng = np.random.default_rng(7)
    pcm = rng.integers(-20000, 20000, 512 * 5).astype(np.int32)
    short_mid = stream_of_blocks(pcm, 512, [512, 512, 256, 512, 512, 256])
    long_mid = stream_of_blocks(pcm, 256, [256, 256, 512, 256, 256, 256, 256, 256, 256])
    plain = stream_of_blocks(pcm, 512, [512] * 5)
    for odd in (short_mid, long_mid):
        assert ref(odd).error == "OK" and np.array_equal(ref(odd).samples, pcm)
    assert plain == synth.generate(pcm=pcm, block_size=512, **VERBATIM).flac  # the builder writes real frames
    sts = [gen(512 * 6, 130 + i, block_size=512, **VERBATIM).flac for i in range(6)]
    check(sts + [plain], [(HOP, HOP)])
    for odd in (short_mid, long_mid):
        hop = check(sts[:3] + [odd] + sts[3:], [(HOP, SCAN), (SCAN, SCAN)], runs=2)
        assert hop[0][2] == hop[1][2] == 0


@pytest.mark.parametrize("where", ["in_header", "in_frame", "one_byte_short"])
def test_truncation(gpu_ready, where):
    sts = [gen(1024 * 6, 80 + i, block_size=1024, **LPC8) for i in range(8)]
    data = [s.flac for s in sts]
    o = [int(x) for x in sts[6].frame_offsets]
    cut = {"in_header": o[4] + 3, "in_frame": (o[2] + o[3]) // 2, "one_byte_short": len(data[6]) - 1}[where]
    data[6] = data[6][:cut]
    assert ref(data[6]).error != "OK"
    # a missing header ends the hop (redone with the scan front); with every header there it holds
    check(data, [(HOP, HOP if where == "one_byte_short" else SCAN)])


def test_auto_rule(gpu_ready):
    """Left to itself a class takes the hop front from HOP_MIN_STREAMS streams on; a lone long
    stream keeps the scan front."""
    text = open(os.path.join(ROOT, "zflac_amd", "csrc", "common.h")).read()
    min_streams = int(re.search(r"#define ZFLAC_HOP_MIN_STREAMS (\d+)", text).group(1))
    tiny = [s.flac for s in synth.generate_many([dict(FIXED2, block_size=16, n_samples=32, seed=900 + i)
                                                 for i in range(min_streams)])]
    long_one = gen(1024 * 64, 99, block_size=1024, **LPC8).flac
    for streams, want in ((tiny, HOP), (tiny[:-1], SCAN), ([long_one], SCAN)):
        (res, fronts, seq), = run(streams, None)
        assert fronts == (want, want) and seq == 0
        for data, (err, samples) in zip(streams, res):
            assert err == ref(data).error == "OK"
            np.testing.assert_array_equal(samples, ref(data).samples)


def test_mixed_batch(gpu_ready):
    """A stereo class the hop can follow beside a mono class of unknown totals: each takes its own front."""
    sts = [gen(1024 * 5 + i, 110 + i, block_size=1024, **LPC8) for i in range(6)] + \
          [gen(256 * 7 + i, 120 + i, block_size=256, write_total=0, **FIXED2) for i in range(4)]
    hop = check([s.flac for s in sts], [(HOP | SCAN, HOP | SCAN)])
    assert hop[0][2] == 0
