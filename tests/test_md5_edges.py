"""The device MD5 (md5.hip) at every block, unit and tail edge of its message, on the streams of
tests/md5_edges.py, with zflac_hip_batch_md5_source / _md5_stats showing that the digest under
test is the hash kernel's own: a left-justified stream whose device digest is wrong is decoded
again and hashed on the host (md5_before_justify), after which zflac_hip_batch_md5 returns
STREAMINFO's digest whatever the kernel computed; only the source and the recheck count tell.

CPU tests: the oracle decodes every stream; hashlib over the writer's message bytes is the
STREAMINFO digest and the digest of the oracle's samples before the left-justify shift; L, r and
nu are what each case's name says, from the stream's shape alone; no stream meant to be certified
holds a false frame start; every (form x tail residue x unit count) cell that has a length at all
holds a stream; the batches have the wave shapes they are built for.

`gpu` tests run each wave shape as one batch with the device MD5, once with run() and once with
submit() / wait() beside a second batch in flight (one hub launch over both): every digest equals
hashlib over the oracle's samples and STREAMINFO, comes from the pipelined launch (from the
synchronous one for exactly the streams the sequential planner decoded), never from a recheck, and
the launch was the kernel the shape is built for. One stream per batch has a flipped STREAMINFO
MD5 byte: InvalidChecksum, and the one recheck it costs when its depth is left-justified."""
import functools
import hashlib
import re

import numpy as np
import pytest

import oracle
import zflac_amd
from zflac_amd import _lib, errors

from . import craft, malformed, md5_edges
from .test_gpu import _md5_pre_justify

DEPTHS = [bps for _, bps in md5_edges.DEPTHS]
COOP, MULTI, LANE = _lib.MD5_K_COOP, _lib.MD5_K_MULTI, _lib.MD5_K_LANE
NONE, PIPELINED, SYNC, HOST_RECHECK = (_lib.MD5_SRC_NONE, _lib.MD5_SRC_PIPELINED, _lib.MD5_SRC_SYNC,
                                       _lib.MD5_SRC_HOST_RECHECK)


@functools.lru_cache(maxsize=None)
def _ref(data: bytes):
    return oracle.decode(data)


def _message(cr) -> bytes:
    """The bytes zflac hashes, from the writer's PCM: (bps + 7) / 8 little-endian bytes a sample."""
    w = (cr.bps + 7) // 8
    return np.ascontiguousarray(cr.pcm_array.astype("<i8").view(np.uint8).reshape(-1, 8)[:, :w]).tobytes()


def _everything():
    return md5_edges.all_cases() + md5_edges.planted()


# ---------------------------------------------------------------------------- CPU
def test_abi_symbols_and_constants():
    """The two calls are declared, exported and bound; the header's ZFLAC_MD5_SRC_* / ZFLAC_MD5_K_*
    are the values the binding carries; a NULL batch or pointer is an argument error."""
    import ctypes
    import os

    L = _lib.load()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zflac_hip.h")).read()
    src = {n: int(v) for n, v in re.findall(r"#define ZFLAC_MD5_SRC_(\w+) (\d+)\n", text)}
    assert src == {"NONE": 0, "PIPELINED": 1, "SYNC": 2, "HOST_RECHECK": 3}
    assert src == {n: getattr(_lib, "MD5_SRC_" + n) for n in src}
    ks = {n: int(v) for n, v in re.findall(r"#define ZFLAC_MD5_K_(\w+) (\d+)u", text)}
    assert ks == {"COOP": 1, "MULTI": 2, "LANE": 4} == {n: getattr(_lib, "MD5_K_" + n) for n in ks}
    assert re.search(r"Added without a bump.*zflac_hip_batch_md5_source.*zflac_hip_batch_md5_stats", text, re.S)
    s, k, r = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint64()
    assert L.zflac_hip_batch_md5_source(None, 0, ctypes.byref(s)) == 14
    assert L.zflac_hip_batch_md5_stats(None, ctypes.byref(k), ctypes.byref(r)) == 14
    assert L.zflac_hip_batch_md5_stats(None, None, None) == 14


@pytest.mark.parametrize("bps", DEPTHS + ["planted"])
def test_oracle_and_hashlib_agree(bps):
    """The oracle decodes every stream to the writer's PCM; hashlib over the writer's message bytes
    is STREAMINFO's digest and the digest of the oracle's samples before the shift."""
    for c in (md5_edges.planted() if bps == "planted" else md5_edges.cases(bps)):
        r = _ref(c.data)
        assert r.error == "OK", (c.name, r.error)
        assert (r.channels, r.bits_per_sample) == (1, c.bps), c.name
        np.testing.assert_array_equal(r.samples, c.cr.justified(), err_msg=c.name)
        msg = _message(c.cr)
        assert len(msg) == c.L, c.name
        dig = hashlib.md5(msg).digest()
        assert dig == c.cr.md5 == c.data[26:42], c.name
        assert dig == _md5_pre_justify(r.samples, r.bits_per_sample), c.name


def test_geometry_is_what_the_name_says():
    """L, r and nu from channels, block size, frames and depth, against the case's name; and the
    form is the one md5_job (md5_host.cpp) gives the depth."""
    names = set()
    for c in _everything():
        cr = c.cr
        w = (cr.bps + 7) // 8
        U = 192 if w == 3 else 256
        L = cr.channels * cr.bs * len(cr.layout) * w
        m = re.fullmatch(r"(\w+?)_(\d+)_(tail|unit|small|planted)_L(\d+)_r(\d+)_nu(\d+)", c.name)
        assert m, c.name
        assert (int(m[2]), int(m[4]), int(m[5]), int(m[6])) == (cr.bps, L, L % 64, L // U), c.name
        assert (L, L % 64, L // U) == md5_edges.geometry(cr.channels, cr.bs, len(cr.layout), cr.bps) == (c.L, c.r, c.nu)
        js = md5_edges.justify_of(cr.bps)
        form = ({1: "raw8", 2: "s16" if js else "raw16", 3: "s24" if js == 8 else "s24js", 4: "s32" if js else "raw32"})[w]
        assert m[1] == form == c.form and (js > 0) == (form[0] == "s"), c.name
        assert cr.channels == 1 and cr.bs >= 16 and L <= 4 * 256 + 256, c.name
        names.add(c.name)
    assert len(names) == len(_everything())
    # every (mode, js) form of md5_job, RAW at each of its widths, with shifts by whole bytes and not
    assert {f: d[0] for f, d in md5_edges.FORMS.items()} == {"raw8": (8,), "raw16": (16,), "raw32": (32,), "s16": (9, 15),
                                                            "s32": (25, 31), "s24": (24,), "s24js": (17, 20)}


def test_no_false_frame_start_in_certified_streams():
    """No byte-aligned sync pattern off the frame starts (the frame search would take it for a
    candidate); a planted stream holds exactly its one copy of a header, CRC-8 valid."""
    for c in md5_edges.all_cases():
        assert craft.sync_frames(c.cr) == [], c.name
    for c in md5_edges.planted():
        f = 0
        assert len(c.cr.layout) == 2 and craft.sync_frames(c.cr) == [f], c.name
        (at,) = craft.sync_positions(c.cr, f)
        off = c.cr.frame_offsets[f]
        hdr = c.data[off:off + 7]
        assert c.data[off + at:off + at + 7] == hdr, c.name
        assert int(craft._crc_rows(np.frombuffer(hdr, np.uint8), [0], [6], craft._CRC8, 8)[0]) == hdr[6], c.name


def test_samples_span_the_depth():
    """Every stream holds the depth's minimum, maximum, -1 and 0 at both ends; in a 16-bit
    container a negative low half beside a positive high half of one dword, and the reverse. Over a
    depth's streams the samples reach the top and bottom sixteenth of the range (uniform, seeded)."""
    for bps in DEPTHS:
        lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
        seen = []
        for c in md5_edges.cases(bps):
            p = c.cr.pcm_array
            n = p.size
            for part in (p[:8], p[n - 9:]):
                assert {lo, hi, -1, 0} <= set(part.tolist()), c.name
            assert p.min() == lo and p.max() == hi
            if craft.widths(bps)[0] == 16:
                for part, base in ((p[:8], 0), (p[n - 8:], n - 8)):
                    pairs = [(int(part[i]), int(part[i + 1])) for i in range(len(part) - 1) if (base + i) % 2 == 0]
                    assert any(a < 0 < b for a, b in pairs) and any(a > 0 > b for a, b in pairs), c.name
            seen.append(p[8:n - 9])
        mid = np.concatenate(seen)
        assert (mid > hi - (hi >> 3)).any() and (mid < lo - (lo >> 3)).any(), bps
        assert len(set(mid.tolist())) > min(mid.size, 1 << bps) // 3, bps


def test_coverage_table():
    """Every (form x tail residue x nu 0..4) cell holds a stream, for every depth of the form. The
    only cells without one have no length at all: three-byte samples, nu = 0, r = 0 (L < 192,
    a multiple of 64 and of 3: L = 0)."""
    empty = []
    for form, (depths, w, U) in md5_edges.FORMS.items():
        for bps in depths:
            cells = {(c.r, c.nu) for c in md5_edges.cases(bps)}
            for r in md5_edges.TAILS[w]:
                for nu in md5_edges.NUS:
                    if (r, nu) in cells:
                        continue
                    assert not [L for L in range(nu * U, (nu + 1) * U) if L % 64 == r and L % w == 0 and L >= 16 * w], \
                        (form, bps, r, nu)
                    empty.append((form, r, nu))
    assert sorted(set(empty)) == [("s24", 0, 0), ("s24js", 0, 0)]
    # the residues are the ones nearest the edges that the width allows
    for w, tails in md5_edges.TAILS.items():
        reach = [r for r in range(64) if any((r + 64 * j) % w == 0 for j in range(3))] if w != 3 else list(range(64))
        assert max(r for r in reach if r <= 55) in tails and min(r for r in reach if r >= 56) in tails
        assert max(reach) in tails and 0 in tails
    assert md5_edges.TAILS[1] == (55, 56, 63, 0) and md5_edges.TAILS[2] == (54, 56, 62, 0) and md5_edges.TAILS[4] == (52, 56, 60, 0)
    assert {54, 57, 63, 0} <= set(md5_edges.TAILS[3])


def test_unit_edges():
    """L = kU - w, kU, kU + w for k = 1..4 and one L < U, for every depth."""
    for form, (depths, w, U) in md5_edges.FORMS.items():
        for bps in depths:
            Ls = {c.L for c in md5_edges.cases(bps)}
            for k in (1, 2, 3, 4):
                assert {k * U - w, k * U, k * U + w} <= Ls, (bps, k)
            assert any(c.kind == "small" and c.L < U for c in md5_edges.cases(bps))
            assert {c.nu for c in md5_edges.cases(bps)} == {0, 1, 2, 3, 4}


def test_wave_shapes():
    """The batches have the shapes they are built for, by the host's job order (longest first)."""
    for bps in DEPTHS:
        a = md5_edges.shape_a(bps)
        waves = md5_edges.job_waves([c.L for c in a])
        assert len(a) >= 70 and len(waves) == 2 and len(waves[-1]) < 64
        nus = {a[i].nu for i in waves[0]}
        assert {0, 4} <= nus and nus == {0, 1, 2, 3, 4}, (bps, nus)  # lanes leave the unit loop at every unit
        assert {c.name for c in a} == {c.name for c in md5_edges.cases(bps)}
    for form, (depths, _, _) in md5_edges.FORMS.items():
        b = md5_edges.shape_b(depths[0])
        waves = md5_edges.job_waves([c.L for c in b])
        assert len(b) > 64 * md5_edges.MD5_WG_WAVES and len(waves) == md5_edges.MD5_WG_WAVES + 1 and len(waves[-1]) < 64
        assert all(b[i].nu == 0 for i in waves[-1])
    c = md5_edges.shape_c()
    assert sum(x.planted for x in c) == len(md5_edges.planted()) >= 2
    assert {x.form for x in c} == {"raw16"}
    seen = []
    for pair in md5_edges.D_PAIRS:
        d = md5_edges.shape_d(pair)
        assert len({md5_edges.MODE_OF[x.form] for x in d}) == 2 and len(d) == sum(len(md5_edges.cases(b)) for b in pair)
        seen += pair
    assert sorted(seen) == sorted(DEPTHS)


# ---------------------------------------------------------------------------- GPU
_COOP_GOT = set()  # what the single-mode launches of this session were: all k_md5_coop, or all its fallback


def _flip(data: bytes) -> bytes:
    b = bytearray(data)
    b[30] ^= 0x01  # a STREAMINFO MD5 byte
    return bytes(b)


def _kernels_ok(shape: str, k: int):
    if shape in ("a", "b", "c"):
        # the pipelined launch: k_md5_coop, or k_md5_multi where the device refuses its LDS (then
        # every such launch of the session); (c)'s synchronous launch over the planner's streams
        # may add a kernel of its own (k_md5_coop again, or k_md5 when a stream lies unaligned)
        pipe = k & (COOP | MULTI)
        print(f"shape {shape}: kernels {k:#x}:", "k_md5_coop" if pipe == COOP else "the k_md5_multi fallback")
        assert pipe in (COOP, MULTI), k
        _COOP_GOT.add(pipe)
        assert len(_COOP_GOT) == 1, _COOP_GOT
        assert k == pipe or (shape == "c" and k & ~pipe == LANE), k
    elif shape in ("d", "e_hub"):
        assert k == MULTI, k
    else:
        assert shape == "e" and k == LANE, k


def _run_shape(shape: str, items, extra=(), second=None):
    """items: the Cases of the batch; extra: (bytes, error name) of streams that are no Case.
    One stream's STREAMINFO MD5 byte is flipped. Two passes: run(), then submit() / wait() with
    `second` (Cases; by default the first ten of the batch) in flight as well."""
    flips = [i for i, c in enumerate(items) if not c.planted and c.nu >= 1 and c.L % 64]
    flip = flips[len(flips) // 2]
    datas = [_flip(c.data) if i == flip else c.data for i, c in enumerate(items)] + [d for d, _ in extra]
    want_err = ["InvalidChecksum" if i == flip else "OK" for i in range(len(items))] + [e for _, e in extra]
    for (d, e) in extra:
        assert _ref(d).error == e != "OK"
    planner = sum(c.planted for c in items) + len(extra)
    justified_flip = 1 if md5_edges.justify_of(items[flip].bps) else 0
    second = list(second if second is not None else [c for c in items if not c.planted][:10])

    def check(b, cs, errs, flipped, rechecks):
        for i, e in enumerate(errs):
            rc, _ = b.info(i)
            assert errors.NAMES.get(rc) == e, (shape, i, rc, e)
            if e != "OK":
                assert b.md5_source(i) == NONE, (shape, i)
                continue
            c, r = cs[i], _ref(cs[i].data)
            dig = b.md5(i)
            src = b.md5_source(i)
            assert src != HOST_RECHECK, (shape, c.name, "the device digest was not STREAMINFO's: only the recheck saved it")
            assert dig == _md5_pre_justify(r.samples, r.bits_per_sample), (shape, c.name)
            assert dig == c.data[26:42], (shape, c.name)
            assert src == (SYNC if c.planted else PIPELINED), (shape, c.name, src)
        k, n = b.md5_stats()
        assert n == rechecks, (shape, n, rechecks)  # the flipped stream's, if its depth is justified
        assert b.timings().sequential_streams == sum(c.planted for c in cs) + (len(errs) - len(cs)), shape
        return k

    b = zflac_amd.Batch(datas, device_md5=True, timing=True)
    b2 = zflac_amd.Batch([c.data for c in second], device_md5=True, timing=True)
    try:
        b.run()
        _kernels_ok(shape, check(b, items, want_err, flip, justified_flip))
        b.submit()
        b2.submit()
        b.wait()
        b2.wait()
        _kernels_ok(shape, check(b, items, want_err, flip, 2 * justified_flip))
        _kernels_ok("a" if shape == "c" else shape, check(b2, second, ["OK"] * len(second), None, 0))
        assert planner == b.timings().sequential_streams
        # a read with verify_md5: the device verdict stands, nothing is decoded again
        for i in sorted({0, len(items) - 1, (flip + 1) % len(items)}):
            got = b.read(i, verify_md5=True).samples.values
            np.testing.assert_array_equal(got, _ref(items[i].data).samples, err_msg=items[i].name)
        with pytest.raises(errors.InvalidChecksum):
            b.read(flip, verify_md5=True)
        assert b.md5_stats().rechecks == 2 * justified_flip, shape
    finally:
        b.close()
        b2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bps", DEPTHS)
def test_shape_a_one_class_mixed_unit_counts(gpu_ready, bps):
    """(a) One class, 70 jobs or more; the first wave holds lanes of every unit count 0..4."""
    _run_shape("a", md5_edges.shape_a(bps))


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(md5_edges.FORMS))
def test_shape_b_second_workgroup(gpu_ready, form):
    """(b) More tiny jobs than a k_md5_coop workgroup has lanes: a second workgroup, a partial last wave."""
    _run_shape("b", md5_edges.shape_b(md5_edges.FORMS[form][0][0]))


@pytest.mark.gpu
def test_shape_c_planner_streams_hashed_afterwards(gpu_ready):
    """(c) A cooperative batch in which a malformed stream and the planted ones go to the sequential
    planner: their lanes only help load, and the synchronous launch hashes the planted ones."""
    bad = malformed.cases()["bad_sync_frame2"]
    _run_shape("c", md5_edges.shape_c(), extra=[(bad[0], bad[1])], second=md5_edges.cases(16)[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("pair", md5_edges.D_PAIRS, ids=lambda p: f"{p[0]}+{p[1]}")
def test_shape_d_two_modes(gpu_ready, pair):
    """(d) Two forms in one batch: k_md5_multi, each lane its own loads."""
    _run_shape("d", md5_edges.shape_d(pair))


@pytest.mark.gpu
@pytest.mark.parametrize("bps", DEPTHS)
def test_shape_e_lane_loads(gpu_ready, monkeypatch, bps):
    """(e) ZFLAC_MD5_LANE_LOADS=1 on the run stream (ZFLAC_MD5_NOHUB=1: a hub launch is always
    k_md5_multi or k_md5_coop): k_md5."""
    monkeypatch.setenv("ZFLAC_MD5_LANE_LOADS", "1")
    monkeypatch.setenv("ZFLAC_MD5_NOHUB", "1")
    _run_shape("e", md5_edges.shape_e(bps))


@pytest.mark.gpu
@pytest.mark.parametrize("bps", [9, 20, 31])
def test_shape_e_lane_loads_through_the_hub(gpu_ready, monkeypatch, bps):
    """ZFLAC_MD5_LANE_LOADS=1 alone: the hub's launch is k_md5_multi."""
    monkeypatch.setenv("ZFLAC_MD5_LANE_LOADS", "1")
    _run_shape("e_hub", md5_edges.shape_e(bps))


@pytest.mark.gpu
@pytest.mark.parametrize("bps", DEPTHS)
def test_host_hash_needs_no_recheck(gpu_ready, bps):
    """Without the device MD5, _read hashes on the host (SampleHasher, its shifted branches for the
    justified depths): every stream verifies with no recheck, no stream has a device digest, and a
    flipped STREAMINFO MD5 is InvalidChecksum, after one recheck where the depth is justified."""
    cs = md5_edges.cases(bps)
    b = zflac_amd.Batch([c.data for c in cs] + [_flip(cs[len(cs) // 2].data)])
    try:
        with pytest.raises(errors.InvalidArgument):
            b.md5_stats()  # before the first run
        with pytest.raises(errors.InvalidArgument):
            b.md5_source(0)
        b.submit()
        with pytest.raises(errors.InvalidArgument):
            b.md5_stats()  # between submit and wait
        b.wait()
        for i, c in enumerate(cs):
            np.testing.assert_array_equal(b.read(i, verify_md5=True).samples.values, _ref(c.data).samples, err_msg=c.name)
            assert b.md5_source(i) == NONE and b.md5(i) is None
        assert b.md5_stats() == (0, 0)
        with pytest.raises(errors.InvalidChecksum):
            b.read(len(cs), verify_md5=True)
        assert b.md5_stats() == (0, 1 if md5_edges.justify_of(bps) else 0)
        with pytest.raises(errors.InvalidArgument):
            b.md5_source(len(cs) + 1)
    finally:
        b.close()
