"""The frame scan (k_scan, k_compact, candidate_ok: zflac_amd/csrc/scan.hip, frame_header.h) at every
window, lane, round, chunk and header-form edge.

A wrong scan cannot change a sample: the stream goes to the sequential planner and still equals the
oracle. What it changes is `timings().sequential_streams`, so that count is what the GPU half pins,
exactly, per family of crafted streams (tests/scan_edges.py).

CPU half: the scan's integer logic compiled for the host (tests/c/scan_probe.cpp, plain g++ against
frame_header.h: the SWAR sync masks over every byte pair, the parser with the register CRC-8 and
the candidate filter walked over every stream) against the Python restatement in scan_edges.py;
every case on the edge it names, by the layout model; the oracle's verdict on every stream; the
writer's defaults byte for byte.

GPU half: one batch per family under front="scan", run twice: every stream's error and samples equal
the oracle's, the front is (SCAN, SCAN) and `sequential_streams` equals the family's count of cases
that name a candidate the parallel pass cannot certify."""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import oracle

from . import craft
from . import crc16_edges as E16
from . import scan_edges as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zflac_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "scan_probe.cpp")
DEPS = [SRC, os.path.join(CSRC, "frame_header.h"), os.path.join(CSRC, "common.h")]
ALL_FILLINGS = 6 ** 6


def _stale(out: str) -> bool:
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


# ---- CPU: the probe ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    lib = os.path.join(ROOT, "tests", "c", "_build", "libscan_probe.so")
    if _stale(lib):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Werror", "-O3", "-shared", "-fPIC", "-pthread", "-I", CSRC,
                               SRC, "-o", lib])
    dll = ctypes.CDLL(lib)
    dll.scan_probe_masks.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    dll.scan_probe_masks.restype = ctypes.c_uint64
    dll.scan_probe_candidates.restype = ctypes.c_uint64
    dll.scan_probe_candidates.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64] + [ctypes.c_uint32] * 5 + [
        ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
        ctypes.c_uint64]
    dll.scan_probe_crc8_header_ok.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    return dll


def probe_candidates(dll, data: bytes, form: int) -> list:
    fb = E.frames_begin_of(data)
    first = E.parse_header(data, fb, len(data), E.si_rate_of(data))
    cap = len(data) // 2 + 1
    pos, bs, hl = (ctypes.c_uint64 * cap)(), (ctypes.c_uint32 * cap)(), (ctypes.c_uint32 * cap)()
    n = dll.scan_probe_candidates(data, len(data), fb, first.byte1, first.nch, first.dcode, first.rate, E.si_rate_of(data),
                                  form, pos, bs, hl, cap)
    assert n <= cap
    return [(int(pos[i]), int(bs[i]), int(hl[i])) for i in range(n)]


def all_cases():
    return [(fam, c) for fam, cases in E.families().items() for c in cases]


def test_constants(probe):
    out = (ctypes.c_uint64 * 4)()
    probe.scan_probe_constants(out)
    assert list(out) == [E.CHUNK_BYTES, E.SCAN_THREADS, E.SCAN_BYTES_PER_THREAD, E.CHUNK_CAP]
    assert E.ROUNDS * E.SCAN_THREADS * E.WINDOW == E.CHUNK_BYTES


def test_sync_masks_every_pair_position_and_filling(probe):
    """ff_mask, sync_mask, sync_any against a byte loop: all 65,536 (byte, next byte) pairs at each of
    the four positions of d (position 3: the next byte is byte 0 of dn), the six other bytes of d and
    dn every combination of 00 01 7F 80 F8 FF. sync_mask exact per byte, sync_any nonzero exactly
    where sync_mask is."""
    assert probe.scan_probe_masks(ALL_FILLINGS, min(8, os.cpu_count() or 1)) == 0


def test_fixed_length_crc8_on_crafted_headers(probe):
    """crc8_header_ok (k_hop's form) on the crafted headers of every length 6..16: right as written,
    wrong with any one bit of the CRC-8 byte flipped; whatever follows the header in the 16 bytes."""
    seen = set()
    for c in E.length_cases():
        for f, (a, _) in enumerate(c.st.frames):
            n = c.st.hdr_lens[f]
            seen.add(n)
            h = c.data[a:a + 16]
            assert E.crc8(h[:n - 1]) == h[n - 1]
            assert probe.scan_probe_crc8_header_ok(h, n) == 1, (c.name, f)
            bad = bytearray(h)
            bad[n - 1] ^= 1 << (f % 8)
            assert probe.scan_probe_crc8_header_ok(bytes(bad), n) == 0, (c.name, f)
    assert seen == set(range(6, 17))


def test_probe_sanitized(tmp_path):
    """The probe as a program of its own under the address and undefined-behaviour sanitizers: the
    masks over the fillings of 00 and FF, both walks over every stream."""
    exe = os.path.join(ROOT, "tests", "c", "_build", "scan_probe_san")
    if _stale(exe):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Werror", "-O1", "-g", "-pthread", "-DSCAN_PROBE_MAIN",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                               "-I", CSRC, SRC, "-o", exe])
    paths, want = [], []
    for i, (fam, c) in enumerate(all_cases()):
        if len(c.data) > 80000 and fam != "cap":
            continue
        p = tmp_path / f"{i}.flac"
        p.write_bytes(c.data)
        paths.append(str(p))
        want.append(len(E.expected_candidates(c.data)))
    r = subprocess.run([exe, "12"] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert lines[0] == "masks 0"
    assert [ln.split() for ln in lines[1:1 + len(paths)]] == [[str(n), str(n), "1", "0"] for n in want]


# ---- CPU: the writer -----------------------------------------------------------------------------
def test_craft_defaults_write_the_same_bytes():
    """Streams written without the new keyword arguments, against digests taken from the writer as it
    was before them (and through crc16_edges.padded, whose length field grew to 24 bits)."""
    c = craft
    rng = np.random.default_rng(1)
    out = [c.write(1, 8, 16, [[c.Sub(kind="const", samples=[0x21])] for _ in range(16)]),
           c.write(1, 16, 256, [[c.Sub(kind="verbatim", samples=rng.integers(-3000, 3000, 256))] for _ in range(3)]),
           c.write(2, 16, 4096, [[c.Sub(kind="fixed", order=2, params=(("k", 5),), samples=rng.integers(-200, 200, 4096))
                                  for _ in range(2)] for _ in range(2)], assignment="ms", rate=48000),
           c.write(1, 12, 17, [[c.Sub(kind="verbatim", samples=rng.integers(0, 1000, 17))] for _ in range(130)], bs_field=16)]
    got = [hashlib.sha256(x.flac).hexdigest()[:16] + ":" + str(len(x.flac)) for x in out]
    assert got == ["8cf8e507dae935c0:218", "3497d0f700193009:1608", "b54535ff52a20906:41407", "75c9025dfba20f86:4854"]
    flac = out[0].flac
    assert E16.padded(flac, 7) == flac[:4] + b"\x00" + flac[5:42] + bytes([0x81, 0, 0, 7]) + bytes(7) + flac[42:]
    assert E16.padded(flac, 300)[42:46] == bytes([0x81, 0, 1, 44]) and E.frames_begin_of(E16.padded(flac, 300)) == 346


def test_header_forms_reach_every_code_and_length():
    bs_codes, rate_codes, number_lens, byte1s, lens = set(), set(), set(), set(), set()
    for _, c in all_cases():
        for f, (a, _) in enumerate(c.st.frames):
            if a + 16 > len(c.data):
                continue
            d = c.data
            bs_codes.add(d[a + 2] >> 4)
            rate_codes.add(d[a + 2] & 15)
            byte1s.add(d[a + 1])
            first = d[a + 4]
            number_lens.add(1 if first < 0x80 else 8 - (first ^ 0xFF).bit_length())
            lens.add(c.st.hdr_lens[f])
    assert bs_codes == set(range(1, 16)) and rate_codes == set(range(15))
    assert number_lens == set(range(1, 8)) and byte1s == {0xF8, 0xF9} and lens == set(range(6, 17))
    st = E.LENGTH_FORMS[16]
    assert st["first_number"] >= 1 << 31 and st["blocking"] == "variable"
    assert any(c.data[c.st.frames[0][0] + 4] == 0xFE for c in E.length_cases() + E.form_cases())  # a 7-byte number


# ---- CPU: every case on its edge -------------------------------------------------------------------
def test_length_cases_meet_every_byte_on_interior_lanes():
    for c in E.length_cases():
        L = int(c.name[3:])
        assert set(c.st.hdr_lens) == {L}
        assert all((e - a) % 16 == 1 for a, e in c.st.frames)
        pl = [c.st.place(f) for f in c.at]
        assert {p.b for p in pl if p.source == "dpp"} == set(range(16)), c.name
        assert sum(p.source == "dpp" for p in pl) >= 17
        assert any(p.header_crosses for p in pl) and any(p.crc8_only_crosses for p in pl)
    assert [int(c.name[3:]) for c in E.length_cases()] == list(range(6, 17))


def test_source_cases_sit_on_their_windows():
    seen = set()
    for c in E.source_cases():
        name, b = c.name[len("source_"):c.name.rindex("_b")], int(c.name[c.name.rindex("_b") + 2:])
        chunk, rnd, thread, source = E.SOURCES[name]
        p = c.st.place(c.at[0])
        assert (p.chunk, p.round, p.thread, p.lane, p.b, p.hdr_len, p.source) == (chunk, rnd, thread, 63, b, E.SOURCE_L, source)
        assert p.header_crosses and p.sync_crosses == (b == 15) and p.crc8_only_crosses == (b == 17 - E.SOURCE_L)
        seen.add((name, b))
    assert len(seen) == len(E.SOURCES) * 3
    assert {(s[1], s[2]) for s in E.SOURCES.values()} >= {(0, 63), (0, 127), (0, 191), (0, 255), (6, 255), (7, 255)}


def test_chunk_edge_cases_sit_on_their_edges():
    by = {c.name[5:]: c for c in E.chunk_edge_cases()}
    for name, (chunk, off) in {"first_byte_of_chunk1": (1, 0), "last_byte_of_chunk0": (0, E.CHUNK_BYTES - 1),
                               "end_minus_hdr": (0, E.CHUNK_BYTES - 8), "end_minus_hdr_plus1": (0, E.CHUNK_BYTES - 7)}.items():
        c = by[name]
        p = c.st.place(c.at[0])
        a = c.st.frames[c.at[0]][0]
        assert p.chunk == chunk and a - E.grid_base(c.st.frames_begin) == chunk * E.CHUNK_BYTES + off and p.hdr_len == 8
        assert p.source == ("dpp" if chunk else "chunk_end") and p.header_crosses == (name in ("last_byte_of_chunk0",
                                                                                                "end_minus_hdr_plus1"))
    for name, n in (("exactly_one_chunk", 1), ("one_chunk_and_a_byte", 2)):
        c = by[name]
        ch = E.chunk_ranges(c.st.frames_begin, len(c.data))
        assert len(ch) == n and ch[-1][1] - E.grid_base(c.st.frames_begin) == E.CHUNK_BYTES + n - 1
    assert E.chunk_counts(by["exactly_one_chunk"].data)[-1] > 0 and E.chunk_counts(by["one_chunk_and_a_byte"].data)[-1] == 0
    assert E.chunk_counts(by["frame_over_two_chunks"].data) == [2, 0, 1]


def test_first_chunk_cases_cover_every_residue():
    plain = [c for c in E.first_chunk_cases() if not c.extra]
    assert [c.st.frames_begin % 16 for c in plain] == list(range(16))
    planted = [c for c in E.first_chunk_cases() if c.extra]
    assert [c.st.frames_begin % 16 for c in planted] == list(range(6, 16))
    for c in planted:
        fb, rate = c.st.frames_begin, E.si_rate_of(c.data)
        first = E.parse_header(c.data, fb, len(c.data), rate)
        for p in c.extra:  # a valid candidate in everything but its place
            assert E.grid_base(fb) <= p and p + 6 <= fb
            h = E.parse_header(c.data, p, len(c.data), rate)
            assert E.candidate_ok(h, first) and h.hdr_len == 6
        assert E.chunk_ranges(fb, len(c.data))[0][0] == fb
        assert oracle.decode(c.data).error == "OK"


def test_end_cases_sit_on_their_edges():
    cases = E.end_cases()
    assert [len(c.data) % 16 for c in cases[:4]] == [1, 8, 15, 0]
    assert all(c.st.frames[-1][1] == len(c.data) for c in cases[:4])
    cuts = cases[4:]
    assert [len(c.data) - c.st.frames[3][0] for c in cuts] == list(range(4, 16))
    assert all(c.st.hdr_lens[3] == 16 and c.seq == 1 and c.error == "EndOfStream" for c in cuts)


def test_neighbour_cases_sit_on_their_edges():
    by = {c.name: c for c in E.neighbour_cases()}
    c = by["crc16_low_byte_ff"]
    a = c.st.frames[1][0]
    assert c.data[a - 1:a + 2] == b"\xff\xff\xf8"
    for target in (0xFFF8, 0xFFF9):  # a sync code made of the trailer, the real one right behind it
        c = by[f"trailer_{target:04x}"]
        a = c.st.frames[2][0]
        assert c.data[a - 2:a + 2] == target.to_bytes(2, "big") + b"\xff\xf8"
        assert a - 2 in E.sync_codes(c.data, c.st.frames_begin)
        assert E.crc16_fast(c.data[c.st.frames[1][0]:a - 2]) == target
    c = by["bs_field_ff"]
    assert len({c.st.place(f).b for f in c.at}) == 8  # (266-byte frames: every other byte of a window)
    assert len([c for c in by if c.startswith("near_miss")]) == len(E.NEAR_MISSES)
    for (x, y) in E.NEAR_MISSES:
        c = by[f"near_miss_{x:02x}_{y:02x}"]
        fb = c.st.frames_begin
        firsts = [p for p in c.at if c.data[p] == x and c.data[p + 1] == y and p + 1 in c.at]
        assert {p % 16 for p in firsts} == {3, 7, 11, 15}
        ends = [E.place(p, 8, fb, len(c.data)) for p in firsts if p % 16 == 15]
        assert {pl.source for pl in ends} == {"dpp", "lane", "round", "chunk_end"}
        assert not [p for p in E.sync_codes(c.data, fb) if p in c.at]  # near misses, not sync codes


FILTER_TERM = {"control": [], "crc8": ["crc8"], "zero_bit": ["zero_bit"], "byte1": ["byte1"], "channels": ["channels"],
               "depth": ["depth"], "rate": ["rate"]}


def test_filter_cases_fail_exactly_one_term():
    seen = set()
    for c in E.filter_cases():
        name = c.name[len("filter_"):]
        f9 = name.endswith("_f9")
        name = name[:-3] if f9 else name
        where = next(w for w in E.FILTER_PLACES if name.endswith("_" + w))
        term = name[:-len(where) - 1]
        fb, rate = c.st.frames_begin, E.si_rate_of(c.data)
        first = E.parse_header(c.data, fb, len(c.data), rate)
        assert first.byte1 == (0xF9 if f9 else 0xF8)
        at = c.at[0]
        assert c.data[at] == 0xFF and c.data[at + 1] & 0xFE == 0xF8 and any(a <= at and at + 8 <= b for a, b in c.st.samples)
        h = E.parse_header(c.data, at, len(c.data), rate)
        assert E.rejected_by(h, first) == FILTER_TERM.get(term, ["parse"]), (c.name, E.rejected_by(h, first))
        if term.startswith("parse"):
            assert h.err in ("InvalidFrameHeader", "InvalidCodedNumber")
        else:
            assert E.crc8(c.data[at:at + h.hdr_len - 1]) == c.data[at + h.hdr_len - 1] ^ (0x10 if term == "crc8" else 0)
        pl = E.place(at, h.hdr_len or 8, fb, len(c.data))
        chunk, rnd, thread, b = E.FILTER_PLACES[where]
        assert (pl.chunk, pl.round, pl.thread, pl.b) == (chunk, rnd, thread, b)
        assert pl.source == ("lane" if where == "b15_lane63" else "dpp")
        assert c.seq == int(term == "control")
        seen.add((term, where, f9))
    terms = {t for t, _, f9 in seen if not f9}
    assert terms == {"control", "crc8", "zero_bit", "byte1", "channels", "depth", "rate", "parse_bs_code0", "parse_rate_code15",
                     "parse_number_ff", "parse_number_10xxxxxx", "parse_bs_ffff"}
    assert {t for t, _, f9 in seen if f9} == {"control", "byte1"} and len(seen) == 2 * (len(terms) + 2)


def test_cap_cases_hold_the_counts_they_name():
    by = {c.name: c for c in E.cap_cases()}
    for c in E.cap_cases():
        assert c.st.frames_begin % 16 == 0
        if c.note != "smallest":
            assert E.chunk_counts(c.data) == [int(x) for x in c.note.split(",")], c.name
    assert {E.chunk_counts(by[n].data)[0] for n in ("cap_63", "cap_64", "cap_65")} == {E.CHUNK_CAP - 1, E.CHUNK_CAP, E.CHUNK_CAP + 1}
    c = by["cap_65th_in_last_window"]
    pl = c.st.place(64)
    assert (pl.chunk, pl.round, pl.thread, pl.source) == (0, E.ROUNDS - 1, E.SCAN_THREADS - 1, "chunk_end")
    counts = E.chunk_counts(by["cap_four_overflowed_in_a_row"].data)
    assert [n > E.CHUNK_CAP for n in counts] == [False, True, True, True, True, False, False]  # two share a group of four
    c = by["cap_smallest_frames"]
    counts = E.chunk_counts(c.data)
    assert c.st.frames[0][1] - c.st.frames[0][0] == 11 and len(counts) == 2
    # (11 bytes while the frame number takes one byte, 12 up to number 2,047, 13 after: 2,688, not 32768 / 11)
    assert 40 * E.CHUNK_CAP < counts[0] < E.CHUNK_BYTES // 11 and {e - a for a, e in c.st.frames} == {11, 12, 13}
    beside = [E.chunk_counts(c.data) for c in E.cap_beside_cases()]
    assert beside == [[20], [200], [9], [64]]


def test_unknown_total_cases():
    cases = E.unknown_total_cases()
    assert all(E.si_total_of(c.data) == 0 for c in cases)
    assert [len(c.data) - cases[0].st.frames[-1][1] for c in cases] == [0, 1, 2, 3, 4]
    assert [c.seq for c in cases] == [0, 0, 0, 0, 1]


# ---- CPU: the candidates of every stream ------------------------------------------------------------
def test_expected_candidates_python_probe_and_frames(probe):
    n_seq = 0
    for fam, c in all_cases():
        want = E.expected_candidates(c.data)
        for form in (2, 1):
            assert probe_candidates(probe, c.data, form) == want, (c.name, form)
        pos = [p for p, _, _ in want]
        starts = [a for a, e in c.st.frames if a + 1 < len(c.data)]
        whole = [a for a, e in c.st.frames if e <= len(c.data)]
        if c.seq == 0:
            assert pos == starts == whole, c.name  # the true frame starts and nothing else
            assert [h for _, _, h in want] == c.st.hdr_lens, c.name
        else:
            n_seq += 1
            if fam == "filter":
                assert sorted(set(pos) - set(starts)) == list(c.extra) and set(starts) <= set(pos), c.name
            else:
                assert c.name.startswith(("end_cut", "unknown_garbage4")) and pos == whole, c.name
    assert n_seq == 4 + 12 + 1


def test_oracle_decodes_every_case():
    for _, c in all_cases():
        r = oracle.decode(c.data)
        assert r.error == c.error, (c.name, r.error)
        if c.error == "OK":
            np.testing.assert_array_equal(r.samples, c.st.pcm, err_msg=c.name)
        assert len(c.data) < 210_000


# ---- GPU ---------------------------------------------------------------------------------------------
_ORACLE: dict = {}


def ref(data: bytes):
    if data not in _ORACLE:
        _ORACLE[data] = oracle.decode(data)
    return _ORACLE[data]


def run(streams, front="scan", runs=2, **kw):
    """Per run of one batch: ([(error, samples)], (planned, used) fronts, sequential streams)."""
    import zflac_amd

    from .test_hop_front import gpu_result

    b = zflac_amd.Batch(streams, timing=True, front=front, **kw)
    out = []
    try:
        for _ in range(runs):
            b.run()
            out.append(([gpu_result(b, i) for i in range(len(streams))], b.front(), b.timings().sequential_streams))
    finally:
        b.close()
    return out


def same_as_oracle(streams, res):
    for i, (data, (err, v)) in enumerate(zip(streams, res)):
        r = ref(data)
        assert err == r.error, (i, err, r.error)
        if r.samples is not None and v is not None:
            np.testing.assert_array_equal(v, r.samples, err_msg=str(i))
        assert (v is None) == (r.samples is None or err not in ("OK", "InvalidChecksum")), (i, err)


def check_scan(cases, **kw):
    from zflac_amd import _lib

    streams = [c.data for c in cases]
    want = sum(c.seq for c in cases)
    for res, fronts, seq in run(streams, **kw):
        same_as_oracle(streams, res)
        assert fronts == (_lib.FRONT_SCAN, _lib.FRONT_SCAN)
        assert seq == want, (seq, want)


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(E.families()))
def test_family(gpu_ready, family):
    """One batch of the family's streams under the scan front, run twice (the second run has the
    planned buckets): the oracle's errors and samples, and exactly the family's seq = 1 cases finished
    by the planner."""
    check_scan(E.families()[family])


@pytest.mark.gpu
def test_each_control_alone(gpu_ready):
    """Every case the planner must finish, in a batch of its own: 1 each."""
    controls = [c for _, c in all_cases() if c.seq]
    assert len(controls) == 17
    for c in controls:
        check_scan([c])


@pytest.mark.gpu
def test_all_certified_families_in_one_batch(gpu_ready):
    cases = [c for _, c in all_cases() if c.seq == 0]
    assert len(cases) > 64
    check_scan(cases, runs=1)


@pytest.mark.gpu
def test_with_the_crc16_check(gpu_ready):
    """The same with ZFLAC_FLAG_CHECK_CRC16: every frame's trailer is right (patched frames too), so
    everything the oracle calls OK stays OK."""
    cases = [c for _, c in all_cases() if c.error == "OK"]
    check_scan(cases, runs=1, check_crc16=True)


@pytest.mark.gpu
def test_hop_front_same_results(gpu_ready):
    """The fixed-blocking, known-total families forced to the hop front: the oracle's results,
    whatever front the batch ends up using."""
    for fam in E.HOP_FAMILIES:
        streams = [c.data for c in E.families()[fam]]
        for res, _, _ in run(streams, front="hop", runs=1):
            same_as_oracle(streams, res)
