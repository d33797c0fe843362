"""The host side of the hop front (k_hop, zflac_amd/csrc/hop.hip), without a GPU: the value of a
frame header's coded number (frame_header.h: coded_number_value), the header fields the parser
has always returned, and the choice of front with its per-stream descriptors (stream_plan.cpp:
plan_hop). Built with plain g++, like tests/test_stream_plan.py."""
from __future__ import annotations

import ctypes
import os
import subprocess

import pytest

import synth

from .util import GOLDEN, load_fixture_manifest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zflac_amd", "csrc")
SCAN, HOP = 1, 2
AUTO, FORCE_SCAN, FORCE_HOP = 0, 1, 2


class Hdr(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint) for n in ("bs", "rate", "hdr_len", "chan_code", "dcode", "byte1", "zero_bit",
                                             "bs_code")] + \
               [(n, ctypes.c_int) for n in ("err", "crc_eof", "crc_ok", "num_ok")] + [("number", ctypes.c_ulonglong)]


class Desc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint) for n in ("n_frames", "f0", "units", "guess")]


@pytest.fixture(scope="module")
def probe():
    srcs = [os.path.join(ROOT, "tests", "c", "hop_probe.cpp"), os.path.join(CSRC, "stream_plan.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("stream_plan.h", "frame_header.h", "common.h")]
    lib = os.path.join(ROOT, "tests", "c", "_build", "libhop_probe.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Werror", "-O2", "-shared", "-fPIC", "-I", CSRC,
                               *srcs, "-o", lib])
    dll = ctypes.CDLL(lib)
    dll.hop_probe_header.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, ctypes.POINTER(Hdr)]
    dll.hop_probe_header.restype = None
    dll.hop_probe_plan.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                                   ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(Desc),
                                   ctypes.POINTER(ctypes.c_ulonglong)]
    dll.hop_probe_plan.restype = ctypes.c_int
    dll.hop_probe_default_max_frames.restype = ctypes.c_uint
    dll.hop_probe_default_min_streams.restype = ctypes.c_uint
    return dll


def header(dll, data: bytes, avail=None, si_rate=44100) -> Hdr:
    h = Hdr()
    dll.hop_probe_header(data, len(data) if avail is None else avail, si_rate, ctypes.byref(h))
    return h


def plan(dll, streams, mode=AUTO, max_frames=1 << 20, min_streams=1):
    n = len(streams)
    arr = (ctypes.c_char_p * n)(*streams)
    lens = (ctypes.c_size_t * n)(*[len(s) for s in streams])
    out = (Desc * max(n, 1))()
    total = ctypes.c_ulonglong()
    f = dll.hop_probe_plan(arr, lens, n, mode, max_frames, min_streams, out, ctypes.byref(total))
    return f, [(d.n_frames, d.f0, d.units, d.guess) for d in out[:n]], total.value


# ---------------------------------------------------------------- the test's own header model
def crc8(b: bytes) -> int:
    c = 0
    for x in b:
        c ^= x
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def coded(n: int) -> bytes:
    """The UTF-8-style coded number of RFC 9639 section 9.1.5, 1 to 7 bytes."""
    if n < 0x80:
        return bytes([n])
    for k, bits in ((2, 11), (3, 16), (4, 21), (5, 26), (6, 31), (7, 36)):
        if n < 1 << bits:
            cont = [(0x80 | ((n >> (6 * i)) & 0x3F)) for i in range(k - 1)][::-1]
            lead = ((0xFF << (8 - k)) & 0xFF) | (n >> (6 * (k - 1)))
            return bytes([lead] + cont)
    raise ValueError(n)


def make_header(number: int) -> bytes:
    """Fixed blocking, 4,096 samples (code 12), 44.1 kHz (code 9), stereo L/R, 16 bits."""
    h = bytes([0xFF, 0xF8, 0xC9, 0x18]) + coded(number)
    return h + bytes([crc8(h)])


RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000,
         11: 96000}


def model(d: bytes, off: int, si_rate: int):
    """(bs, rate, hdr_len, chan_code, dcode, byte1, zero_bit, bs_code, number) of a well-formed header."""
    b1, b2, b3, first = d[off + 1], d[off + 2], d[off + 3], d[off + 4]
    ones = 0
    while ones < 8 and first & (0x80 >> ones):
        ones += 1
    nbytes = 1 if ones == 0 else ones
    num = first if ones == 0 else first & (0x7F >> ones)
    for k in range(1, nbytes):
        num = (num << 6) | (d[off + 4 + k] & 0x3F)
    idx = off + 4 + nbytes
    bc, rc = b2 >> 4, b2 & 15
    if bc == 6:
        bs, idx = d[idx] + 1, idx + 1
    elif bc == 7:
        bs, idx = ((d[idx] << 8) | d[idx + 1]) + 1, idx + 2
    else:
        bs = 192 if bc == 1 else (144 << bc if bc <= 5 else 1 << bc)
    if rc == 0:
        rate = si_rate
    elif rc == 12:
        rate, idx = d[idx], idx + 1
    elif rc in (13, 14):
        rate, idx = ((d[idx] << 8) | d[idx + 1]) * (10 if rc == 14 else 1), idx + 2
    else:
        rate = RATES[rc]
    assert d[idx] == crc8(d[off:idx])
    return (bs, rate, idx + 1 - off, b3 >> 4, (b3 >> 1) & 7, b1, b3 & 1, bc, num)


def fields(h: Hdr):
    return (h.bs, h.rate, h.hdr_len, h.chan_code, h.dcode, h.byte1, h.zero_bit, h.bs_code, h.number)


# ---------------------------------------------------------------------------------- tests
NUMBERS = [0, 1, 0x7F, 0x80, 0x7FF, 0x800, 2099, 0xFFFF, 0x10000, 0x1FFFFF, 0x200000, 0x3FFFFFF, 0x4000000,
           0x7FFFFFFF, 0x80000000, 0xFFFFFFFFF]


def test_coded_number_values(probe):
    """1- to 6-byte encodings (and the 7-byte one of sample numbers) give the number written; the
    rest of the header reads as before."""
    sizes = set()
    for n in NUMBERS:
        hdr = make_header(n)
        sizes.add(len(coded(n)))
        h = header(probe, hdr + bytes(8))
        assert (h.err, h.crc_eof, h.crc_ok, h.num_ok) == (0, 0, 1, 1), hex(n)
        assert fields(h) == (4096, 44100, len(hdr), 1, 4, 0xF8, 0, 12, n), hex(n)
        assert fields(h) == model(hdr + bytes(8), 0, 44100), hex(n)
    assert sizes == {1, 2, 3, 4, 5, 6, 7}


def test_coded_number_rejects_what_zflac_rejects(probe):
    base = bytes([0xFF, 0xF8, 0xC9, 0x18])
    for first in (0xFF, 0x80, 0xBF):  # src/zflac.zig:206
        h = header(probe, base + bytes([first]) + bytes(12))
        assert h.num_ok == 0 and h.err == 8, hex(first)
    hdr = make_header(0x2345)  # 3 bytes
    for avail in (4, 5, 6):  # the number's bytes are cut off
        assert header(probe, hdr, avail=avail).num_ok == 0, avail
    h = header(probe, hdr, avail=7)  # the number is whole, the CRC-8 byte is not there
    assert (h.num_ok, h.number, h.crc_eof) == (1, 0x2345, 1)


def test_existing_fields_unchanged_on_golden_headers(probe):
    """Every frame header of the committed fixtures: the fields the parser has always returned
    equal the test's own reading of the header, and the number is the frame's index (fixed
    blocking) or its first sample (variable blocking)."""
    seen = 0
    for fx in load_fixture_manifest()["fixtures"]:
        with open(os.path.join(GOLDEN, fx["file"]), "rb") as f:
            data = f.read()
        st = synth.generate(**fx["config"])
        assert st.flac == data, fx["file"]  # the writer reproduces the fixture: its frame offsets hold
        si_rate = (data[18] << 12) | (data[19] << 4) | (data[20] >> 4)
        first_sample = 0
        for i, off in enumerate(int(x) for x in st.frame_offsets):
            h = header(probe, data[off:off + 32], avail=len(data) - off, si_rate=si_rate)
            assert (h.err, h.crc_eof, h.crc_ok, h.num_ok) == (0, 0, 1, 1), (fx["file"], i)
            assert fields(h) == model(data, off, si_rate), (fx["file"], i)
            assert h.number == (first_sample if fx["config"].get("variable_blocking") else i), (fx["file"], i)
            first_sample += h.bs
            seen += 1
    assert seen >= 20


MONO = dict(channels=1, bps=16, predictor=2, order=2, block_size=256)
STEREO = dict(channels=2, bps=16, block_size=1024, order=8)


def _gen(n_samples, seed, **kw):
    return synth.generate(**dict(kw, n_samples=n_samples, seed=seed))


def test_eligibility_one_case_per_way_out(probe):
    ok = [_gen(256 * 4, 1, **MONO).flac, _gen(256 * 3 + 5, 2, **MONO).flac, _gen(256 * 2, 3, **MONO).flac]
    assert plan(probe, ok)[0] == HOP  # totals, fixed blocking, within both limits
    variable = _gen(256 * 4, 4, **dict(MONO, variable_blocking=1)).flac
    assert plan(probe, ok + [variable])[0] == SCAN
    assert plan(probe, ok + [variable], mode=FORCE_HOP)[0] == SCAN  # forcing does not lift it
    unknown = _gen(256 * 4, 5, **dict(MONO, write_total=0)).flac
    assert plan(probe, ok + [unknown])[0] == SCAN
    assert plan(probe, ok + [unknown], mode=FORCE_HOP)[0] == SCAN
    assert plan(probe, ok, max_frames=4)[0] == HOP  # the longest has 4 frames
    assert plan(probe, ok, max_frames=3)[0] == SCAN
    assert plan(probe, ok, max_frames=3, mode=FORCE_HOP)[0] == SCAN
    assert plan(probe, ok, min_streams=3)[0] == HOP
    assert plan(probe, ok, min_streams=4)[0] == SCAN
    assert plan(probe, ok, min_streams=4, mode=FORCE_HOP)[0] == HOP  # forcing lifts only this one
    assert plan(probe, ok, mode=FORCE_SCAN)[0] == SCAN
    assert plan(probe, [])[0] == SCAN
    broken = b"fLaX" + ok[0][4:]  # a stream the host already rejects
    assert plan(probe, ok + [broken])[0] == SCAN


def test_defaults_are_the_documented_ones(probe):
    text = open(os.path.join(ROOT, "include", "zflac_hip.h")).read()
    text = " ".join(text.replace("\n *", " ").split())  # the comment as prose, however it is wrapped
    assert f"no stream has more than {probe.hop_probe_default_max_frames()} frames" in text
    assert f"at least {probe.hop_probe_default_min_streams()} streams" in text


def test_descriptor_arithmetic(probe):
    """f0 is the running frame count, n_frames = ceil(total / block) (a short last frame and a
    one-frame stream among them), units = block x channels, guess = frame bytes / frames."""
    sts = [_gen(1024 * 5, 11, **STEREO), _gen(1024 * 3 + 17, 12, **STEREO), _gen(9, 13, **STEREO),
           _gen(1024, 14, **STEREO), _gen(1024 * 2 + 1023, 15, **STEREO)]
    front, descs, total = plan(probe, [s.flac for s in sts])
    assert front == HOP
    f0 = 0
    for s, (n, first, units, guess) in zip(sts, descs):
        assert n == len(s.frame_offsets)
        assert (first, units) == (f0, 1024 * 2)
        assert guess == (len(s.flac) - s.frames_begin) // n
        f0 += n
    assert [d[0] for d in descs] == [5, 4, 1, 1, 3]
    assert total == f0 == 14
