"""The exact value-range edges of the predictor and the stereo decorrelation
(tests/value_edges.py), on streams written from chosen samples by tests/craft.py: the SampleType
of a predicted sample, the InterType of every LPC product and partial sum in zflac's order, the
decorrelation's overflow per output channel, the raw reads, and which error wins.

CPU tests hold every case to an exact-integer model of zflac's checks (the first trap sits where
the case aims, or nowhere), to the oracle (the stated error name, the writer's PCM for OK
streams) and to craft's chunk model (the edge sample's chunk takes the fast, warm or generic
path the case names, in the wave the batch gives it). `gpu` tests decode one batch per family,
OK and trapping streams side by side in the same waves, twice: error names equal the case's and
the oracle's, OK streams are bit-exact with the device digest equal to STREAMINFO's, and exactly
the refused streams went to the sequential planner."""
import functools

import numpy as np
import pytest

import oracle
import zflac_amd
from zflac_amd import _lib, errors

from . import craft, value_edges

FAMILIES = value_edges.FAMILIES
WALKS = [(n, None) for n in FAMILIES] + [("S", "wave"), ("D", "wave")]


@functools.lru_cache(maxsize=None)
def _refs(name: str) -> tuple:
    """The oracle's verdict on every stream of a family's batch, computed once."""
    return tuple(oracle.decode(c.data) for c in value_edges.batch(name))


# ---------------------------------------------------------------------------- CPU
def test_model_arithmetic():
    """The model's own pieces, against values worked by hand."""
    assert value_edges.fits(127, 8) and not value_edges.fits(128, 8) and value_edges.fits(-128, 8)
    assert not value_edges.fits(-129, 8) and value_edges.fits(-(1 << 31), 32) and not value_edges.fits(1 << 31, 32)
    assert value_edges.wrap(40000, 16) == -25536 and value_edges.wrap(-32769, 16) == 32767
    assert value_edges.ms_side(0, 32760, 32767, 0) == 14 and value_edges.ms_side(1, 32760, 32768, 1) == -15
    assert value_edges.choose_k([-(1 << 30)]) == (30, 32)
    # 8-bit, order 3, history -128, -128, 127: the partial sums in zflac's order, oldest first
    sub = craft.Sub(kind="lpc", order=3, coefs=(-200, -200, -200), precision=9, shift=15, samples=[127, -128, -128, 127, 5])
    trap, _ = value_edges.model([[sub]], 1, 8, 5)
    assert trap == (0, 0, 4, "partial")
    sub = craft.Sub(kind="lpc", order=3, coefs=(-200, -200, -200), precision=9, shift=15, samples=[127, -128, -128, 5])
    assert value_edges.model([[sub]], 1, 8, 4)[0] is None


def test_families_are_complete():
    names = [c.name for n in FAMILIES for c in value_edges.family(n)]
    assert len(names) == len(set(names))
    for n in FAMILIES:
        cs = value_edges.family(n)
        assert all(c.name.startswith(n + "_") for c in cs)
        errs = {c.error for c in cs}
        assert "OK" in errs and "OutOfDomain" in errs, (n, errs)  # no family is all-OK or all-error
        for c in cs:
            assert len(c.cr.layout) == 3 and c.cr.bs in (32, 48, 64), c.name
            assert (c.error == "OK") == (c.aim is None and c.flac is None), c.name
        # every edge as a pair: the admissible stream beside the inadmissible one
        traps = [c.name[:-5] for c in cs if c.name.endswith("_trap")]
        oks = {c.name[:-3] for c in cs if c.name.endswith("_ok") and c.error == "OK"}
        assert traps and set(traps) <= oks, (n, set(traps) - oks)
    assert {c.error for c in value_edges.family("P")} == {"OK", "OutOfDomain", "EndOfStream", "InvalidSubframeHeader"}


@pytest.mark.parametrize("name", FAMILIES)
def test_model_puts_the_first_trap_where_the_case_aims(name):
    """From the Subs alone: the first trap in zflac's read order is the case's, or there is none;
    and where nothing traps the model's PCM is the writer's."""
    for c in value_edges.family(name):
        cr = c.cr
        trap, pcm = value_edges.model(c.frames, cr.channels, cr.bps, cr.bs, cr.assignment)
        assert trap == c.aim, (c.name, trap, c.aim)
        if trap is None:
            SB = craft.widths(cr.bps)[0]
            assert pcm == [value_edges.wrap(v, SB) for v in cr.pcm], c.name
            assert len(pcm) == 3 * cr.bs * cr.channels, c.name


@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_agrees(name):
    """The oracle's error name is the case's; the samples of an OK stream are the writer's PCM,
    left-justified as zflac does (a value outside the depth wraps there)."""
    for c, r in zip(value_edges.batch(name), _refs(name)):
        assert r.error == c.error, (c.name, r.error, c.error)
        if c.error == "OK":
            want = c.cr.justified()
            assert (r.channels, r.bits_per_sample) == (c.cr.channels, c.cr.bps), c.name
            assert r.samples.dtype == want.dtype and r.samples.size == want.size, c.name
            np.testing.assert_array_equal(r.samples, want, err_msg=c.name)


@pytest.mark.parametrize("name", FAMILIES)
def test_cases_take_the_path_they_name(name):
    """From craft's chunk model: the edge sample's chunk is fast, warm or generic as the case says,
    and no other lane of its wave sends a fast or warm chunk back to the generic path. No frame
    holds a byte-aligned sync pattern (the frame scan would count a lane more)."""
    cases = value_edges.batch(name)
    seen = value_edges.assert_paths(cases)
    want = {"S": {"fast", "warm", "generic"}, "I": {"fast", "generic"}, "J": {"fast", "generic"},
            "D": {"fast", "generic"}, "R": {"fast", "warm", "generic"}, "P": {"fast"}}[name]
    assert set(seen) == want, (name, seen)
    for c in cases:
        assert craft.sync_frames(c.cr) == [], c.name
    by_class = {}
    for (i, f), wave in value_edges.waves(cases).items():
        by_class.setdefault(value_edges.class_of(cases[i]), set()).add(len(wave))
    assert all(sizes == {64 // k[1]} for k, sizes in by_class.items()), by_class  # whole waves only


def test_unsafe_lanes_are_the_ones_the_kernels_send_to_the_generic_path():
    """craft's `unsafe` restates safe_lpc_bound (decode/subframe.h): the J pair straddles it."""
    by = {c.name: c for c in value_edges.family("J")}
    assert not by["J_sum_safe_ok"].cr.layout[1][0].unsafe and by["J_sum_unsafe_ok"].cr.layout[1][0].unsafe
    assert by["J_sum_safe_ok"].cr.pcm[64:128] == by["J_sum_unsafe_ok"].cr.pcm[64:128]  # the edge frame's samples
    by = {c.name: c for c in value_edges.family("I")}
    assert not by["I_sum255_shift0_ok"].cr.layout[1][0].unsafe and by["I_sum256_neg_ok"].cr.layout[1][0].unsafe
    orders = {c.cr.layout[1][0].order for c in by.values() if c.cr.layout[1][0].unsafe}
    assert {2, 3, 8, 12, 16, 32} <= orders  # every history bucket of decode/config.h's kernels


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


def _needs_recheck(c) -> bool:
    """The device digest of this stream cannot be STREAMINFO's: a left-justified depth, and either
    a stream that really fails its checksum, or an OK stream with a sample beyond its depth, of
    which the shift has pushed out bits that zflac hashed: the hashed bytes ((bps + 7) / 8 of
    them) of the sample and of the sample shifted left and back differ. A 24-bit sample never
    does that (its three hashed bytes survive the shift by eight). md5_before_justify decodes
    exactly these streams again."""
    bps = c.cr.bps
    js = 16 - bps if 9 <= bps <= 15 else 32 - bps if 17 <= bps <= 31 else 0
    if not js:
        return False
    if c.error != "OK":
        return c.error == "InvalidChecksum"
    kept, hashed = craft.widths(bps)[0] - js, 8 * ((bps + 7) // 8)
    return any((value_edges.wrap(v, kept) ^ v) & ((1 << hashed) - 1) for v in c.cr.pcm)


def _verdicts(name, walk, device_md5):
    """Decode the family's batch twice; every disagreement of both runs, as printable rows."""
    cases, refs = value_edges.batch(name), _refs(name)
    refused = sum(c.error != "OK" for c in cases)
    rechecked = sum(_needs_recheck(c) for c in cases)
    b = zflac_amd.Batch([c.data for c in cases], timing=True, device_md5=device_md5, walk=walk)
    bad = []
    try:
        for run in range(2):
            b.run()
            for i, (c, r) in enumerate(zip(cases, refs)):
                if device_md5:
                    err, got, md5 = _read(b, i)
                else:
                    rc, _ = b.info(i)
                    err = errors.NAMES.get(rc, f"E{rc}") if rc else "OK"
                    got, md5 = (b.read(i, verify_md5=False).samples.values if not rc else None), c.cr.md5
                if err != c.error or r.error != c.error:
                    bad.append((run, c.name, "error", err, r.error, c.error))
                elif err != "OK":
                    continue
                elif got.dtype != r.samples.dtype or not np.array_equal(got, r.samples):
                    bad.append((run, c.name, "differs from the oracle"))
                elif not np.array_equal(got, c.cr.justified()):
                    bad.append((run, c.name, "differs from the writer's PCM"))
                elif md5 != c.cr.md5:
                    bad.append((run, c.name, "device digest"))
                elif device_md5:
                    # the digest is the hash kernel's own, but for the streams beyond their depth
                    src = b.md5_source(i)
                    want = (_lib.MD5_SRC_HOST_RECHECK,) if _needs_recheck(c) else (_lib.MD5_SRC_PIPELINED, _lib.MD5_SRC_SYNC)
                    if src not in want:
                        bad.append((run, c.name, "digest source", src, want))
            if device_md5 and b.md5_stats().rechecks != (run + 1) * rechecked:
                bad.append((run, "rechecks", b.md5_stats().rechecks, "expected", (run + 1) * rechecked))
            if not device_md5 and b.md5_stats() != (0, 0):
                bad.append((run, "md5 stats without the device MD5", b.md5_stats()))
            if b.timings().sequential_streams != refused:
                bad.append((run, "sequential streams", b.timings().sequential_streams, "refused streams", refused))
    finally:
        b.close()
    for row in bad:
        print(name, walk, *row)
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("name,walk", WALKS, ids=[f"{n}-{w or 'auto'}" for n, w in WALKS])
def test_family_verdicts(gpu_ready, name, walk):
    """One batch per family, run twice: every stream's error name is the case's and the oracle's,
    OK streams are bit-exact against the oracle and the writer with the device digest equal to
    STREAMINFO's, and the sequential planner saw exactly the refused streams: the parallel pass
    certified every OK edge stream itself.

    The twelve OK streams of depth 12 and 20 in family S whose edge sample lies beyond the depth
    but inside the container are the ones whose digest cannot be taken from the left-justified
    samples (a 12-bit sample of 32767 has lost its top four bits there): md5_before_justify
    (md5_host.cpp) answers for them. zflac_hip_batch_md5_source says HOST_RECHECK for exactly the
    streams of that kind (_needs_recheck, from the family list) and the pipelined or synchronous
    hash launch for every other OK stream; zflac_hip_batch_md5_stats counts one recheck per such
    stream and run, and none else."""
    s12 = [c for c in value_edges.batch("S") if _needs_recheck(c)]
    assert len(s12) == 12 and all(c.cr.bps in (12, 20) and c.error == "OK" for c in s12)
    bad = _verdicts(name, walk, device_md5=True)
    assert not bad, (walk, bad[:8], len(bad))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_family_pcm(gpu_ready, name):
    """The same batch without the digests: the value verdicts and the PCM alone."""
    bad = _verdicts(name, None, device_md5=False)
    assert not bad, (bad[:8], len(bad))


@pytest.mark.gpu
def test_beyond_depth_streams_alone(gpu_ready):
    """decode() of a 12- or 20-bit stream with a sample beyond its depth: zflac hashes before it
    left-justifies, so the host's checksum verdict is OK too, and the PCM is the writer's."""
    cases = [c for c in value_edges.family("S") if c.error == "OK" and c.cr.bps in (12, 20)]
    assert len(cases) == 12
    for c in cases:
        got = zflac_amd.decode(c.data).samples.values
        np.testing.assert_array_equal(got, c.cr.justified(), err_msg=c.name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_refused_streams_alone(gpu_ready, name):
    """Each refused stream once on its own, through the planner path of a single stream."""
    for c in value_edges.family(name):
        if c.error != "OK":
            try:
                zflac_amd.decode(c.data)
                got = "OK"
            except errors.ZflacError as e:
                got = type(e).__name__
            assert got == c.error, c.name
