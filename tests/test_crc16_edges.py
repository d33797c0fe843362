"""k_crc16 (zflac_amd/csrc/crc16.hip) at every piece, alignment, shift and grid edge.

CPU half: the constants the kernel is compiled with (zflac_amd/csrc/crc16_math.h through
tests/c/crc16_probe.cpp, plain g++) against arithmetic written here, the model of the wave's split
(tests/crc16_edges.py) against the bitwise CRC and the trailers craft wrote, and every crafted case
on the edge it names.

GPU half: every family in pairs. A clean stream is OK and bit-exact against the oracle with
ZFLAC_FLAG_CHECK_CRC16; its bad twins are FrameCrcMismatch with the flag and exactly the oracle's
error and samples without it. Expected values come from the oracle, from crc16_ref and from craft's
own bytes, none from the kernel."""
from __future__ import annotations

import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import oracle
import synth

from . import crc16_edges as E
from . import edges
from .test_crc16 import STEREO, crc16_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zflac_amd", "csrc")


# ---- CPU: the constants ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    src = os.path.join(ROOT, "tests", "c", "crc16_probe.cpp")
    deps = [src, os.path.join(CSRC, "crc16_math.h")]
    lib = os.path.join(ROOT, "tests", "c", "_build", "libcrc16_probe.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Werror", "-O2", "-shared", "-fPIC", "-I", CSRC, src,
                               "-o", lib])
    dll = ctypes.CDLL(lib)
    dll.crc16_probe_mulmod.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    dll.crc16_probe_mulmod.restype = ctypes.c_uint32
    return dll


def test_python_arithmetic_is_sound():
    """What the other CPU tests lean on: x has order 32,767 modulo P (so pow_entry may reduce the
    exponent), the byte-wise CRC equals the bitwise one, and both give the CRC-16/BUYPASS check value."""
    assert E.xpow_by_shifts(E.X_ORDER) == 1
    assert E.mulmod(0x8000, 2) == 0x8005 and E.mulmod(0x1234, 1) == 0x1234  # x^15 * x = x^15 + x^2 + 1
    assert E.crc16_fast(b"123456789") == crc16_ref(b"123456789") == 0xFEE8
    data = random.Random(5).randbytes(3000)
    assert E.crc16_fast(data) == crc16_ref(data)
    for k in range(10):  # the reduced exponent against the plain one
        assert E.pow_entry(k) == E.xpow_by_shifts(8 << k)


def test_slice_tables(probe):
    """All 1,024 entries: t[k][v] = v(x) * x^(8k + 16) mod P, by long division."""
    t = (ctypes.c_uint16 * 1024)()
    probe.crc16_probe_tables(t)
    for k in range(4):
        for v in range(256):
            assert t[k * 256 + v] == E.polymod(v << (8 * k + 16)), (k, v)


def test_power_table(probe):
    """All 40 entries: p[k] = x^(8 * 2^k) mod P, here by single shifts with the exponent reduced by
    the order of x. A legal frame (at most 8 x 32 bits x 65,535 samples, about 2 MiB) reaches p[20];
    p[21..39] run on no stream a test could hold, so this is the only place they can be checked at all."""
    p = (ctypes.c_uint16 * 40)()
    probe.crc16_probe_pow(p)
    assert [p[k] for k in range(40)] == [E.pow_entry(k) for k in range(40)]
    assert p[0] == 0x100 and len({p[k] for k in range(15)}) == 15


def test_mulmod(probe):
    corners = (0, 1, 0x8000, 0xFFFF)
    rng = random.Random(16)
    pairs = [(a, b) for a in corners for b in corners] + [(rng.randrange(1 << 16), rng.randrange(1 << 16))
                                                          for _ in range(400)]
    for a, b in pairs:
        assert probe.crc16_probe_mulmod(a, b) == E.mulmod(a, b), (hex(a), hex(b))
    assert probe.crc16_probe_mulmod(0x8000, 2) == 0x8005  # x^15 * x = x^15 + x^2 + 1


# ---- CPU: the model and the cases -----------------------------------------------------------------
def _families():
    return {"alignment": E.alignment_cases(), "split": E.split_cases(), "shift": E.shift_cases(),
            "coverage": E.coverage_cases(), "trailer": (E.trailer_case(),)}


def _all_cases():
    return [c for fam in _families().values() for c in fam]


def test_model_reproduces_every_trailer():
    """Pieces, shifts and xor in Python give the bitwise CRC of the frame and the trailer craft
    wrote, for every frame of every family (the frames of 32 KiB and more: the byte-wise CRC)."""
    n = 0
    for c in _all_cases():
        for f, (a, e) in enumerate(c.st.frames):
            crc = crc16_ref if e - a < 4096 else E.crc16_fast
            want = int.from_bytes(c.st.data[e - 2:e], "big")
            assert E.crc_by_pieces(c.st.data, a, e, crc) == crc(c.st.data[a:e - 2]) == want, (c.name, f)
            n += 1
    st, _, _ = E.grid_streams()
    for a, e in st.frames:
        assert E.crc_by_pieces(st.data, a, e) == int.from_bytes(st.data[e - 2:e], "big")
    assert n > 200


def test_no_false_syncs_and_twins_differ_in_one_frame():
    for c in _all_cases():
        a, e = c.st.frames[c.frame]
        assert not E.false_syncs(c.st.data, c.st.frames), c.name
        clean = np.frombuffer(c.st.data, np.uint8)
        assert all(clean[lo:hi].max() < 0xFF for f in range(len(c.st.frames)) for lo, hi in c.st.samples[f]), c.name
        assert c.twins, c.name
        for name, data in c.twins.items():
            assert not E.false_syncs(data, c.st.frames), (c.name, name)
            assert len(data) == len(c.st.data)
            diff = np.flatnonzero(np.frombuffer(data, np.uint8) != clean)
            assert diff.size and a + 8 <= diff[0] and diff[-1] < e, (c.name, name)  # behind the frame's header
            assert diff.size == 1 or name in ("zero", "ones")
            # the twin's frame no longer carries its own CRC: FrameCrcMismatch is the right answer
            assert E.crc16_fast(data[a:e - 2]) != int.from_bytes(data[e - 2:e], "big"), (c.name, name)


def test_alignment_cases_sit_on_their_edges():
    seen = {"small": set(), "large": set()}
    for c in E.alignment_cases():
        s = c.split
        if c.name.startswith("align_smallest"):
            assert s.hi - s.lo == 9 and s.span == 3 and s.per == 1 and len(s.live) == 3
            assert c.st.shape == dict(bps=8, bs=16, verb=0, const=1, bs_field=8)
        elif c.name == "align_10_bytes_lo3":
            assert s.hi - s.lo == 10 and s.lo % 4 == 3 and s.span == 4
        else:
            tag = c.name.split("_")[1]
            assert c.name == f"align_{tag}_lo{s.lo % 4}_hi{s.hi % 4}"
            assert 6 <= s.span <= 8 and s.per == 1 if tag == "small" else s.span > 64 and s.per == 2
            seen[tag].add((s.lo % 4, s.hi % 4))
    assert all(len(v) == 16 for v in seen.values())
    assert {c.split.lo % 4 for c in E.alignment_cases() if c.name.startswith("align_smallest")} == {0, 1, 2, 3}


def test_split_cases_sit_on_their_edges():
    by_name = {c.name: c.split for c in E.split_cases()}
    for span in E.SPLIT_SPANS:
        w, r = by_name[f"split_{span}_whole"], by_name[f"split_{span}_ragged"]
        assert w.span == r.span == span and w.per == r.per == -(-span // 64)
        assert (w.lo % 4, w.hi % 4) == (0, 0) and (r.lo % 4, r.hi % 4) == (3, 1)
        assert r.pieces[0][1] - r.pieces[0][0] == 4 * r.per - 3  # lane 0 begins with the first dword's one byte
    assert {63: 1, 64: 1, 65: 2, 127: 2, 128: 2, 129: 3, 319: 5, 321: 6}.items() <= {s: by_name[f"split_{s}_whole"].per
                                                                                     for s in E.SPLIT_SPANS}.items()
    # the last lane that holds bytes holds exactly one: spans 63, 64 (per 1) and 65, 127 (a lone last dword)
    for span in (63, 64, 65, 127):
        assert by_name[f"split_{span}_ragged"].last_lane_bytes == 1, span
    assert by_name["split_129_ragged"].last_lane_bytes == 4 * 2 + 1  # against it: two dwords and a byte
    assert [len(by_name[f"split_{s}_whole"].live) for s in (63, 64, 65, 128, 129)] == [63, 64, 33, 64, 43]
    # a lane that starts exactly at d1 (an empty piece at the end): 63 = 63 x 1, 66 = 33 x 2, 126 = 63 x 2
    assert {s for s in E.SPLIT_SPANS if by_name[f"split_{s}_whole"].lane_at_d1} >= {63, 66, 126}
    assert not by_name["split_64_whole"].lane_at_d1 and not by_name["split_128_whole"].lane_at_d1


def test_shift_cases_use_exactly_p0_to_p20():
    used = set()
    for c, hashed in zip(E.shift_cases(), E.SHIFT_LENGTHS):
        s = c.split
        assert s.hi - s.lo == hashed
        used |= s.powers
    assert used == set(range(21))
    big = E.shift_cases()[-1]
    assert big.st.shape == dict(bps=32, bs=65535, verb=8, const=0, bs_field=16) and 20 in big.split.powers
    # what the rest of the suite reaches: frames under 32 KiB stop below p[15]
    assert max(max(c.split.powers) for c in E.alignment_cases() + E.split_cases() + E.coverage_cases()) < 15


def test_coverage_cases_sit_on_their_edges():
    pers = []
    for c in E.coverage_cases()[:-1]:
        s = c.split
        pers.append(s.per)
        assert (s.lo % 4, s.hi % 4) == (1, 3) and c.st.shape["const"] == 0
        pos = E.cover_positions(c.st, c.frame)
        assert {"first_body_byte", "last_hashed_byte", "last_live_lane_last"} <= set(pos)
        assert {f"lane{i}_{w}" for i in (31, 32) for w in ("first", "last")} <= set(pos)
        if len(s.live) == 64:
            assert {f"lane{i}_{w}" for i in (62, 63) for w in ("first", "last")} <= set(pos)
            assert pos["last_hashed_byte"] == pos["lane63_last"] == pos["last_live_lane_last"] == s.hi - 1
        else:
            assert s.live[-1] == 49 and pos["last_live_lane_last"] == s.hi - 1
        assert pos["first_body_byte"] == s.lo + c.st.shape["bs_field"] // 8 + 7
        for lane in E.COVER_LANES:
            if f"lane{lane}_last" in pos:
                assert lane == s.live[-1] or pos[f"lane{lane}_last"] + 1 == s.pieces[lane][1] == s.pieces[lane + 1][0]
    assert pers == [1, 2, 2, 3]
    c = E.coverage_cases()[-1]
    a, e = c.st.frames[c.frame]
    assert e - a - 2 == 7 + 1 + (12 * 17 + 4) // 8 and c.st.data[e - 3] & 0x0F == 0  # four padding bits, zero


def test_grid_class_is_past_the_largest_grid():
    st, copies, bad = E.grid_streams()
    assert len(st.frames) == E.GRID_FRAMES and all(e - a == 11 for a, e in st.frames)
    assert len(copies) * E.GRID_FRAMES > E.GRID_WAVES + 300 and len(bad) == 16
    assert {0, 2047, 2048, len(copies) - 1} <= set(bad) and bad[2047] == bad[len(copies) - 1] == 15
    assert (bad[0], bad[2048], E.grid_streams(1)[2][2048]) == (0, 0, 1)  # candidates 0, 32768 and 32769
    assert sum(len(c) for c in copies) < 512 * 1024
    for data in set(copies):
        assert not E.false_syncs(data, st.frames)
    assert [i for i, c in enumerate(copies) if c != st.data] == sorted(bad)


# ---- GPU -----------------------------------------------------------------------------------------
_ORACLE: dict = {}


def ref(data: bytes):
    if data not in _ORACLE:
        _ORACLE[data] = oracle.decode(data)
    return _ORACLE[data]


def results(b, n):
    """[(error name, samples or None)], samples also on InvalidChecksum (read without the MD5 check)."""
    from zflac_amd import errors

    out = []
    for i in range(n):
        rc, _ = b.info(i)
        if rc:
            out.append((errors.NAMES.get(rc, f"E{rc}"), None))
            continue
        v = b.read(i, verify_md5=False).samples.values
        try:
            b.read(i, verify_md5=True)
            out.append(("OK", v))
        except errors.ZflacError as e:
            out.append((type(e).__name__, v))
    return out


def run(streams, **kw):
    """One batch run: ([(error, samples)], (planned, used) fronts, sequential streams)."""
    import zflac_amd

    b = zflac_amd.Batch(streams, timing=True, **kw)
    try:
        b.run()
        return results(b, len(streams)), b.front(), b.timings().sequential_streams
    finally:
        b.close()


def same_as_oracle(streams, res):
    for i, (data, (err, v)) in enumerate(zip(streams, res)):
        r = ref(data)
        assert err == r.error, (i, err, r.error)
        assert (v is None) == (r.samples is None), (i, err)
        if v is not None:
            np.testing.assert_array_equal(v, r.samples, err_msg=str(i))


def check_pairs(cases, sequential=0, **kw):
    """The clean streams and the twins of `cases` in one batch, with and without the check."""
    streams, bad, names = [], [], []
    for c in cases:
        streams.append(c.st.data)
        bad.append(False)
        names.append(c.name)
        for name, data in c.twins.items():
            streams.append(data)
            bad.append(True)
            names.append(f"{c.name}/{name}")
    for data, is_bad in zip(streams, bad):
        assert is_bad or ref(data).error == "OK"
    off, _, seq_off = run(streams, **kw)
    same_as_oracle(streams, off)
    on, _, seq_on = run(streams, check_crc16=True, **kw)
    want = ["FrameCrcMismatch" if x else "OK" for x in bad]
    got = [err for err, _ in on]
    assert got == want, [(n, g) for n, g, w in zip(names, got, want) if g != w]
    same_as_oracle([s for s, x in zip(streams, bad) if not x], [r for r, x in zip(on, bad) if not x])
    n_seq = len(streams) if sequential == "all" else sequential
    assert seq_off == seq_on == n_seq, (seq_off, seq_on)
    return streams, want


@pytest.mark.gpu
def test_alignment(gpu_ready):
    """All 16 (lo % 4, hi % 4) at a few dwords and above 64, the smallest legal frame at every offset."""
    check_pairs(E.alignment_cases())


@pytest.mark.gpu
def test_split(gpu_ready):
    """Spans of 63 .. 321 dwords: per 1, 2, 3, 5, 6, a last lane of one byte, a lane exactly at d1."""
    check_pairs(E.split_cases())


@pytest.mark.gpu
def test_shift(gpu_ready):
    """Frames of 2^15 - 1 bytes to the largest there is: every power p[0..20]. A flipped bit in the
    first body byte is carried through the longest shift, one in the last hashed byte through none."""
    check_pairs(E.shift_cases())


@pytest.mark.gpu
def test_every_hashed_byte_counts(gpu_ready):
    """One flipped sample bit at the first body byte, at the first and last byte of the pieces of
    lanes 0, 1, 31, 32, 62 and 63, at the end of the last lane that holds bytes and in the last
    hashed byte, for per = 1, 2, 3; and a flipped padding bit behind an odd count of 12-bit samples.
    Without the check the sample flips are InvalidChecksum (the oracle says so)."""
    cases = E.coverage_cases()
    for c in cases[:-1]:
        assert {ref(t).error for t in c.twins.values()} == {"InvalidChecksum"}, c.name
    check_pairs(cases)


@pytest.mark.gpu
def test_trailer_bits(gpu_ready):
    """All 16 single-bit flips of one trailer, and the trailer replaced by 0 and by 0xFFFF: zflac
    never looks (OK without the check)."""
    c = E.trailer_case()
    assert {ref(t).error for t in c.twins.values()} == {"OK"}
    check_pairs([c])


@pytest.mark.gpu
@pytest.mark.parametrize("front", ["scan", "hop"])
def test_grid_stride(gpu_ready, front):
    """33,120 candidates in one class: more than the 32,768 waves of the largest grid, so the frames
    from 32,768 on are reached only by a wave's second trip. Bad trailers in candidates 0, 32767,
    32768 (hop: 32769), in the last frame of the last stream, where `end` is as close to the
    input's size as the layout allows, and in a dozen seeded others; every other stream is OK."""
    import zflac_amd
    from zflac_amd import _lib

    st, copies, bad = E.grid_streams(1 if front == "hop" else 0)
    assert ref(st.data).error == "OK" and all(ref(c).error == "OK" for c in set(copies))
    want = ["FrameCrcMismatch" if i in bad else "OK" for i in range(len(copies))]
    f = {"scan": _lib.FRONT_SCAN, "hop": _lib.FRONT_HOP}[front]
    for crc in (True, False):
        b = zflac_amd.Batch(copies, timing=True, check_crc16=crc, front=front)
        try:
            b.run()
            assert b.front() == (f, f) and b.timings().sequential_streams == 0
            assert b.timings().frames == len(copies) * E.GRID_FRAMES
            got = [b.error_name(i) for i in range(len(copies))]
            assert got == (want if crc else ["OK"] * len(copies)), [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
            for i in range(len(copies)):
                if got[i] == "OK":
                    np.testing.assert_array_equal(b.read(i).samples.values, ref(copies[i]).samples, err_msg=str(i))
        finally:
            b.close()


@pytest.mark.gpu
def test_sequential_path_same_verdicts(gpu_ready):
    """The alignment and split families through the sequential planner (force_slow: crc16_ok with
    n_frames_host, no stream table): the verdicts of the certified path."""
    check_pairs(E.alignment_cases() + E.split_cases(), sequential="all", force_slow=True)


@pytest.mark.gpu
def test_planted_sync_trailer_is_not_a_trailer(gpu_ready):
    """A CRC-8-valid header copy inside verbatim samples: the chain check rejects the stream, the
    planner decodes the true chain, and the bytes in front of the false candidate are no trailer:
    clean is OK with the check; one real trailer flipped is FrameCrcMismatch."""
    cases = edges.planted_sync_cases()
    data = cases["plant_mono16"][0]
    offs = edges.PLANT_FRAME_OFFSETS["plant_mono16"] + [len(data)]
    bad = E.flip(data, offs[3] - 1, 1)  # frame 2's trailer
    streams = [data, bad, cases["plant_lr16_unknown_total"][0]]
    off, _, seq = run(streams)
    same_as_oracle(streams, off)
    assert [e for e, _ in off] == ["OK"] * 3 and seq == 3
    on, _, seq = run(streams, check_crc16=True)
    assert [e for e, _ in on] == ["OK", "FrameCrcMismatch", "OK"] and seq == 3
    same_as_oracle([streams[0], streams[2]], [on[0], on[2]])


@pytest.mark.gpu
def test_earlier_decode_error_beats_later_bad_trailer(gpu_ready):
    """Frame 1's header broken, frame 3's trailer flipped: zflac stops at frame 1 and never reads
    frame 3, so the stream's error is the oracle's with the check too. The two swapped (the case of
    test_crc16_before_later_frame_error): the earlier mismatch is the error."""
    st = synth.generate(**STEREO)
    o = [int(x) for x in st.frame_offsets] + [len(st.flac)]
    first_err = E.flip(E.flip(st.flac, o[1] + 1, 7), o[4] - 1, 0)   # sync code 0xFFF8 -> 0xFF78
    first_crc = E.flip(E.flip(st.flac, o[2] - 1, 0), o[3] + 1, 7)
    streams = [first_err, first_crc]
    want = ref(first_err).error
    assert want not in ("OK", "InvalidChecksum") and ref(first_crc).error == want
    off, _, _ = run(streams)
    same_as_oracle(streams, off)
    on, _, _ = run(streams, check_crc16=True)
    assert [e for e, _ in on] == [want, "FrameCrcMismatch"]


@pytest.mark.gpu
def test_unknown_total(gpu_ready):
    """Crafted frames under an unknown total, one bad trailer, garbage behind the last frame: without
    the check the oracle's answer (3 bytes of garbage are never read, 8 are a broken header); with
    it the clean streams keep that answer and the earlier mismatch comes before the garbage's error."""
    cases = E.unknown_total_cases()
    names = sorted(cases)
    streams = [cases[n][0] for n in names]
    assert ref(cases["unknown_clean"][0]).error == ref(cases["unknown_clean_garbage3"][0]).error == "OK"
    assert ref(cases["unknown_clean_garbage8"][0]).error not in ("OK", "InvalidChecksum")
    off, _, _ = run(streams)
    same_as_oracle(streams, off)
    on, _, _ = run(streams, check_crc16=True)
    assert [e for e, _ in on] == ["FrameCrcMismatch" if cases[n][1] else ref(cases[n][0]).error for n in names]
    same_as_oracle([s for s, n in zip(streams, names) if not cases[n][1]],
                   [r for r, n in zip(on, names) if not cases[n][1]])


@pytest.mark.gpu
def test_two_flagged_batches_in_flight(gpu_ready):
    """Two batches with the check submitted before either is waited on give the verdicts they give alone."""
    import zflac_amd

    groups, wants = [], []
    for fam in (E.alignment_cases(), E.split_cases()):
        streams = [d for c in fam for d in [c.st.data] + list(c.twins.values())]
        groups.append(streams)
        wants.append([e for c in fam for e in ["OK"] + ["FrameCrcMismatch"] * len(c.twins)])
    alone = [[e for e, _ in run(g, check_crc16=True)[0]] for g in groups]
    assert alone == wants
    bs = [zflac_amd.Batch(g, check_crc16=True) for g in groups]
    try:
        for b in bs:
            b.submit()
        for b in bs:
            b.wait()
        for b, g, want in zip(bs, groups, wants):
            assert [b.error_name(i) for i in range(len(g))] == want
            for i, data in enumerate(g):
                if want[i] == "OK":
                    np.testing.assert_array_equal(b.read(i).samples.values, ref(data).samples)
    finally:
        for b in bs:
            b.close()
