"""Every k_decode instantiation decodes work of its own: the 63 cells of tests/decode_matrix.py
(container x layout x history bucket x MIX), each checked bit for bit against the oracle and
the writer's source PCM, with zflac_hip_batch_decode_buckets showing that the cell's kernel,
not the `rest` launch, decoded it; sweeps over what the cells hold fixed; and one stream per
(container, layout) whose frame groups go through all seven launches. The CPU tests keep the
table honest where there is no GPU: the writer falls back to fixed order 2 or VERBATIM without
a word, and a cell whose streams no longer carry its orders would test another kernel."""
import numpy as np
import pytest

import zflac_amd
from zflac_amd import _lib

from . import decode_matrix as dm
from .util import container_dtype, justified

BATCHES = dm.batch_ids()
BATCH_IDS = [dm.batch_name(key, j) for key, j in BATCHES]
KIND_LAYOUT = [(k, lay) for k in dm.KINDS for lay in dm.LAYOUTS]


def _expected(d, bps):
    return justified(d.pcm, bps).astype(container_dtype(bps))


def _check_reference(d, what):
    """The oracle decodes the stream and reproduces the writer's source PCM."""
    assert d.ref.error == "OK", what
    bps = d.ref.bits_per_sample
    assert d.ref.samples.dtype == container_dtype(bps), what
    np.testing.assert_array_equal(d.ref.samples, _expected(d, bps), err_msg=str(what))


# ---- CPU: the table is what it says ------------------------------------------------------------
def test_cell_table_shape():
    cells = dm.cells()
    assert len(cells) == 63 and len(BATCHES) == 84
    assert sorted({(k, lay) for k, lay, _, _ in cells}) == sorted(KIND_LAYOUT)
    for (kind, lay, mb, mix), batches in cells.items():
        assert [b[0]["channels"] for b in batches] == list(dm.LAYOUTS[lay])
        for cfgs in batches:
            assert len(cfgs) == len(dm.FLAVOURS)
            assert {(c["bps"] + 7) // 8 for c in cfgs} <= ({1}, {2}, {3, 4})[kind]
            assert len({c["channels"] for c in cfgs}) == 1  # one class: same container, same channel count
            assert all(c["block_size"] == 200 and c["n_samples"] == 805 for c in cfgs)
    # over a container's cells every depth and, in stereo, every mode is used
    for kind in dm.KINDS:
        used = {c["bps"] for key, b in cells.items() if key[0] == kind for cfgs in b for c in cfgs}
        assert used == set(dm.DEPTHS[kind])
        modes = {c["stereo_mode"] for key, b in cells.items() if key[:2] == (kind, "stereo") for c in b[0]}
        assert modes == set(dm.STEREO_MODES)
    assert any(c["bps"] == 32 and c["stereo_mode"] == 10 for key, b in cells.items() if key[:2] == (2, "stereo")
               for c in b[0])


@pytest.mark.parametrize("key,j", BATCHES, ids=BATCH_IDS)
def test_cell_streams_are_what_the_table_says(key, j):
    kind, lay, mb, mix = key
    streams = dm.cell_streams(key, j)
    nch = dm.LAYOUTS[lay][j]
    per_stream = []
    for i, d in enumerate(streams):
        _check_reference(d, (key, j, i))
        assert d.ref.channels == nch and d.ref.samples.dtype == (np.int8, np.int16, np.int32)[kind]
        per_stream.append(dm.ch0_types(d.st))
    orders = [[dm.order_of_type(t) for t in ts] for ts in per_stream]
    cv = [t <= 1 for ts in per_stream for t in ts]
    top, bottom = (dm.MIX_ORDER[mb],) * 2 if mix else dm.ORDERS[mb]
    assert top in orders[0][:4], f"the top-order stream fell back: {per_stream[0]}"
    assert bottom in orders[1][:4], f"the bottom-order stream fell back: {per_stream[1]}"
    assert max(max(o) for o in orders) <= top
    if mix:
        assert any(cv)
        # both kinds of lane: CONSTANT (digital silence) and VERBATIM
        assert {0, 1} <= {t for ts in per_stream for t in ts}
    else:
        assert not any(cv)
        # every full frame's order lies in the bucket, so no frame group classifies lower
        for o in orders:
            assert all(dm.bucket_of_order(x) == mb for x in o[:4]), o
        # and no coded channel of any frame is a constant block, which the writer codes CONSTANT
        # (never a side channel: const_side is off)
        for d in streams:
            x = d.st.pcm.reshape(-1, nch).astype(np.int64)
            if nch == 2:
                L, R = x[:, 0], x[:, 1]
                x = {1: (L, R), 8: (L,), 9: (R,), 10: ((L + R) >> 1,)}[d.st.config["stereo_mode"]]
                x = np.stack(x, axis=1)
            for f in range(0, x.shape[0], dm.BS):
                blk = x[f:f + dm.BS]
                assert not (blk == blk[0]).all(axis=0).any(), (key, j, d.st.config, f)


@pytest.mark.parametrize("kind", dm.KINDS)
@pytest.mark.parametrize("name", ["order", "depth", "rice", "block_order"])
def test_sweep_streams_on_the_oracle(name, kind):
    streams = dm.sweep_streams(name, kind)
    cfgs = [d.st.config for d in streams]
    for i, d in enumerate(streams):
        _check_reference(d, (name, kind, i, cfgs[i]))
    types = [dm.ch0_types(d.st) for d in streams]
    if name == "order":  # every order is really written
        got = {(c["channels"], t) for c, ts in zip(cfgs, types) for t in ts[:4]}
        for nch in (1, 2):
            assert {t for n, t in got if n == nch} == set(range(32, 64)) | set(range(8, 13))
    if name == "depth":
        assert sorted(d.ref.bits_per_sample for d in streams) == sorted(2 * list(range(*((4, 9), (9, 17), (17, 33))[kind])))
    if name == "rice":
        ks = {c["rice_k"] for c in cfgs}
        assert set(range(15)) <= ks and (kind == 0 or set(range(15, 31)) <= ks)
    if name == "block_order":
        for c, ts in zip(cfgs, types):
            assert all(t == 31 + c["order"] for t in ts), (c, ts)
            assert len(ts) == 70


@pytest.mark.parametrize("kind,layout", KIND_LAYOUT)
def test_every_bucket_stream_on_the_oracle(kind, layout):
    d = dm.every_bucket_stream(kind, layout)
    _check_reference(d, (kind, layout))


# ---- GPU ---------------------------------------------------------------------------------------
def _assert_batch_equals(b, streams, what, md5=None):
    for i, d in enumerate(streams):
        assert b.error_name(i) == d.ref.error == "OK", (what, i)
        got = b.read(i).samples.values
        assert got.dtype == d.ref.samples.dtype and got.size == d.ref.samples.size, (what, i)
        np.testing.assert_array_equal(got, d.ref.samples, err_msg=f"{what} stream {i}: differs from the oracle")
        np.testing.assert_array_equal(got, _expected(d, d.ref.bits_per_sample),
                                      err_msg=f"{what} stream {i}: differs from the source PCM")
        if md5 == "streaminfo":
            assert b.md5(i) == d.flac[26:42], (what, i)
        elif md5 == "hashlib":
            assert b.md5(i) == d.flac[26:42] == dm.md5_pre_justify(d.ref.samples, d.ref.bits_per_sample), (what, i)


@pytest.mark.gpu
@pytest.mark.parametrize("key,j", BATCHES, ids=BATCH_IDS)
def test_cell_decodes_in_its_own_kernel(gpu_ready, key, j):
    """One k_decode<kind, layout, MB, MIX> instantiation: its cell, decoded twice, equals the
    oracle and the source PCM bit for bit with the device digest equal to STREAMINFO's; on the
    second run no `rest` launch ran and every bucket used had a launch of its own, and the
    classification found the cell's bucket (pure: nothing else; MIX: nothing of the other
    order class). With 2+ channels the second run is repeated under each subframe walk."""
    kind, lay, mb, mix = key
    streams = dm.cell_streams(key, j)
    datas = [d.flac for d in streams]
    bit = dm.bucket_bit(mb, mix)
    if mix:
        low = _lib.BUCKET_4 | _lib.BUCKET_8 | _lib.BUCKET_MIX_8
        other = (_lib.BUCKET_ALL & ~low) if mb == 8 else low
    else:
        other = _lib.BUCKET_ALL & ~bit
    nch = dm.LAYOUTS[lay][j]
    for walk in (None,) if nch == 1 else (None, "lane", "wave"):
        b = zflac_amd.Batch(datas, timing=True, device_md5=True, check_crc16=True, walk=walk)
        try:
            with pytest.raises(zflac_amd.errors.InvalidArgument):
                b.decode_buckets()  # before the first run
            for run in range(2):
                b.run()
                _assert_batch_equals(b, streams, (key, j, walk, run), md5="streaminfo")
            used, planned = b.decode_buckets()
            assert b.timings().rest_launches == 0, (walk, used, planned)
            assert used & ~planned == 0, (walk, used, planned)
            assert used & bit, (walk, used, planned)
            assert used & other == 0, (walk, used, planned)
        finally:
            b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", dm.KINDS)
@pytest.mark.parametrize("name", ["order", "depth", "rice", "block_order"])
def test_sweeps(gpu_ready, name, kind):
    """order: LPC 1..32 and fixed 0..4; depth: every depth of the container, device digest equal
    to hashlib over the oracle's pre-justify bytes; rice: forced parameters 0..30; block_order:
    block sizes at or just above the order, 70 frames. Mono and stereo (block_order: and 3
    channels) in one batch per container, two runs, bit-exact. (A frame group spans several
    streams here, so most orders are decoded by the kernel of a larger bucket: its coefficient
    padding. The cells are where each kernel meets its own orders.)"""
    streams = dm.sweep_streams(name, kind)
    b = zflac_amd.Batch([d.flac for d in streams], timing=True, device_md5=True, check_crc16=True)
    try:
        for run in range(2):
            b.run()
            _assert_batch_equals(b, streams, (name, kind, run), md5="hashlib" if name == "depth" else "streaminfo")
        assert b.timings().rest_launches == 0
        used, planned = b.decode_buckets()
        assert used & ~planned == 0
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,layout", KIND_LAYOUT)
def test_every_bucket_stream(gpu_ready, kind, layout):
    """group_mb routing: one stream whose frame groups lie in all seven buckets. The plan holds
    bucket 8 alone at first, so run 1 decodes six groups in the `rest` launch; run 2 gives each
    its own launch. Both runs are bit-exact (a group decoded twice, or by no launch, is not),
    and both classify the same seven buckets."""
    d = dm.every_bucket_stream(kind, layout)
    b = zflac_amd.Batch([d.flac], timing=True, device_md5=True, check_crc16=True)
    try:
        b.run()
        used, planned = b.decode_buckets()
        assert (b.timings().rest_launches, used, planned) == (1, _lib.BUCKET_ALL, _lib.BUCKET_8)
        _assert_batch_equals(b, [d], (kind, layout, 0), md5="streaminfo")
        b.run()
        used, planned = b.decode_buckets()
        assert (b.timings().rest_launches, used, planned) == (0, _lib.BUCKET_ALL, _lib.BUCKET_ALL)
        _assert_batch_equals(b, [d], (kind, layout, 1), md5="streaminfo")
    finally:
        b.close()


@pytest.mark.gpu
def test_decode_buckets_usage_errors(gpu_ready):
    """InvalidArgument for a null pointer, before the first run and between submit and wait."""
    import ctypes

    d = dm.every_bucket_stream(1, "stereo")
    b = zflac_amd.Batch([d.flac])
    u, p = ctypes.c_uint32(), ctypes.c_uint32()
    L = _lib.load()
    try:
        assert L.zflac_hip_batch_decode_buckets(b._h, ctypes.byref(u), ctypes.byref(p)) == 14
        b.submit()
        assert L.zflac_hip_batch_decode_buckets(b._h, ctypes.byref(u), ctypes.byref(p)) == 14
        b.wait()
        assert L.zflac_hip_batch_decode_buckets(b._h, None, ctypes.byref(p)) == 14
        assert L.zflac_hip_batch_decode_buckets(b._h, ctypes.byref(u), None) == 14
        assert L.zflac_hip_batch_decode_buckets(b._h, ctypes.byref(u), ctypes.byref(p)) == 0
        assert (u.value, p.value) == (_lib.BUCKET_ALL, _lib.BUCKET_8)
        assert b.decode_buckets() == (_lib.BUCKET_ALL, _lib.BUCKET_8)
    finally:
        b.close()
