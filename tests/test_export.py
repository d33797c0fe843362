"""GPU tests of the dense device export (zflac_hip_batch_export / k_export, zflac_amd.tensor):
every dtype and layout, windows, channel fitting, coverage and bounds of the destination,
state errors, caller streams, the sequential planner's output and 64-bit indexing. Expected
values come from the oracle through tests/export_ref.py; every comparison is on bit patterns."""
import ctypes

import torch  # before zflac_amd loads its library: one HIP runtime per process (zflac_amd/tensor.py)

import numpy as np
import pytest

import oracle
import synth
import zflac_amd
from zflac_amd import _lib, errors, tensor

from . import malformed
from .export_ref import BIT_VIEW, expected_row
from .util import PARITY_CONFIGS

pytestmark = pytest.mark.gpu

MIXED = ["mono8_lpc3", "c3_ms16_lpc8", "stereo12_ms", "ch3_16", "ch8_16_fixed", "c4_24bit_lpc32_wasted", "stereo32",
         "blocksize16"]
BAD = ["wrong_md5", "bad_sync_frame2"]
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16, "int32": torch.int32}
LAYOUTS = ["planar", "interleaved"]


class Mixed:
    """The shared batch: its streams, the oracle's verdict on each, and one completed run."""

    def __init__(self, **batch_kw):
        cases = malformed.cases()
        self.datas = [synth.generate(**dict(PARITY_CONFIGS[n], seed=3000 + i)).flac for i, n in enumerate(MIXED)]
        self.datas += [cases[c][0] for c in BAD]
        self.ref = []  # (samples or None, channels, error name)
        self.oracle = [oracle.decode(d) for d in self.datas]
        for r in self.oracle:
            ok = r.error == "OK"
            self.ref.append((np.ascontiguousarray(r.samples) if ok else None, int(r.channels) if ok else 0, r.error))
        self.frames = [s.size // c if s is not None else 0 for s, c, _ in self.ref]
        # device MD5, so that a wrong STREAMINFO MD5 is the stream's result as it is the oracle's
        self.batch = zflac_amd.Batch(self.datas, device_md5=True, **batch_kw)
        self.batch.run()

    def expect(self, C, T, starts, dtype, layout):
        rows, valid = [], []
        for i, (s, c, _) in enumerate(self.ref):
            row, v = expected_row(s, c, C, T, starts[i] if starts is not None else 0, dtype, layout)
            rows.append(row)
            valid.append(v)
        return np.stack(rows), valid


@pytest.fixture(scope="module")
def mixed(gpu_ready):
    m = Mixed()
    yield m
    m.batch.close()


def bits_of(t: torch.Tensor, dtype: str) -> np.ndarray:
    view = torch.int32 if t.element_size() == 4 else torch.int16
    return t.view(view).cpu().numpy().view(BIT_VIEW[dtype])


def check(m, C, T, starts, dtype, layout, **kw):
    x, lengths = tensor.export(m.batch, frames=T, channels=C, starts=starts, dtype=DTYPES[dtype], layout=layout, **kw)
    want, valid = m.expect(C, T, starts, dtype, layout)
    assert x.dtype == DTYPES[dtype] and x.device.type == "cuda" and tuple(x.shape) == want.shape
    got = bits_of(x, dtype)
    for i in range(len(m.datas)):  # row by row, so that a failure names the stream
        np.testing.assert_array_equal(got[i], want[i], err_msg=f"row {i} ({(MIXED + BAD)[i]}) {dtype} {layout}")
    assert lengths.dtype == torch.int64 and lengths.device == x.device
    assert lengths.cpu().tolist() == valid
    return x


def test_statuses_match_the_oracle(mixed):
    for i, (_, _, err) in enumerate(mixed.ref):
        assert errors.NAMES.get(mixed.batch.info(i)[0]) == err, i
    assert [e for _, _, e in mixed.ref[-2:]] == ["InvalidChecksum", "InvalidFrameHeader"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_full_parity(mixed, dtype, layout):
    """C = 8, T = the longest stream: every row equals the reference, error rows are zero with
    length 0, lengths are the frame counts."""
    T = max(mixed.frames)
    x = check(mixed, 8, T, None, dtype, layout)
    for i, (s, _, _) in enumerate(mixed.ref):
        if s is None:
            assert not x[i].view(torch.int32 if x.element_size() == 4 else torch.int16).any().item()


def test_defaults_are_longest_and_widest(mixed):
    x, lengths = tensor.export(mixed.batch)
    assert x.dtype == torch.float32 and tuple(x.shape) == (len(mixed.datas), 8, max(mixed.frames))
    assert lengths.cpu().tolist() == mixed.frames
    want, _ = mixed.expect(8, max(mixed.frames), None, "float32", "planar")
    np.testing.assert_array_equal(bits_of(x, "float32"), want)


def _window_starts(m, shift):
    out = []
    for i, n in enumerate(m.frames):
        cand = [0, 1, 3, 63, 64, 65, 4095, 4097, max(n - 1, 0), n, n + 5]
        out.append(cand[(i + shift) % len(cand)])
    return out


@pytest.mark.parametrize("T", [1, 7, 64, 1000, 4099])
@pytest.mark.parametrize("dtype,layout", [("float32", "planar"), ("float16", "planar"), ("bfloat16", "interleaved"),
                                          ("int32", "interleaved")])
def test_windows(mixed, T, dtype, layout):
    """Per-row starts from {0, 1, 3, 63, 64, 65, 4095, 4097, n-1, n, n+5}, every row taking every
    start in turn: unaligned heads, windows straddling the end and wholly past it, valid_frames."""
    for shift in range(11):
        check(mixed, 2, T, _window_starts(mixed, shift), dtype, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", [1, 3])
def test_channel_fit(mixed, C, layout):
    """C = 1 keeps channel 0 of the stereo and 8-channel streams; C = 3 leaves zero planes for
    mono and cuts 8 channels to 3."""
    T = 4096 + 64
    for dtype in ("float32", "float16", "int32"):
        check(mixed, C, T, None, dtype, layout)


def _c_export(batch, dtype, layout, C, T, dst_ptr, dst_bytes, starts=None, stream=None, size=None):
    n = len(batch)
    h_starts = (ctypes.c_uint64 * n)(*starts) if starts is not None else None
    d = _lib.zflac_export_desc(ctypes.sizeof(_lib.zflac_export_desc) if size is None else size, dtype, layout, C, T,
                               h_starts)
    valid = (ctypes.c_uint64 * n)()
    rc = batch._L.zflac_hip_batch_export(batch._h, ctypes.byref(d), dst_ptr, dst_bytes, valid, stream)
    return rc, list(valid)


@pytest.mark.parametrize("offset", [64, 68])  # a 16-byte aligned destination and one that is not
@pytest.mark.parametrize("layout", LAYOUTS)
def test_coverage_and_bounds(mixed, layout, offset):
    """The destination is a slice of a larger buffer of 0x7F bytes: every element inside is
    written, nothing outside is, and a dst_bytes one element short writes nothing at all."""
    C, T, B = 3, 4100, len(mixed.datas)
    need = B * C * T * 4
    buf = torch.full((offset + need + 256,), 0x7F, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lay = _lib.LAYOUT_PLANAR if layout == "planar" else _lib.LAYOUT_INTERLEAVED
    rc, valid = _c_export(mixed.batch, _lib.EXPORT_F32, lay, C, T, buf.data_ptr() + offset, need - 4)
    assert rc == 14
    assert bool((buf == 0x7F).all().item()), "a refused export wrote to the destination"
    rc, valid = _c_export(mixed.batch, _lib.EXPORT_F32, lay, C, T, buf.data_ptr() + offset, need)
    assert rc == 0
    host = buf.cpu().numpy()
    assert (host[:offset] == 0x7F).all() and (host[offset + need:] == 0x7F).all()
    inside = host[offset:offset + need].copy().view(np.uint32)
    assert not (inside == 0x7F7F7F7F).any(), "elements of the destination were left unwritten"
    want, want_valid = mixed.expect(C, T, None, "float32", layout)
    np.testing.assert_array_equal(inside.reshape(want.shape), want)
    assert valid == want_valid


def test_state_errors(mixed):
    """Before the first run, between submit and wait, and a bad dtype, layout or size: 14."""
    dst = torch.empty((len(mixed.datas), 2, 64), dtype=torch.float32, device="cuda")
    args = (2, 64, dst.data_ptr(), dst.numel() * 4)
    b = zflac_amd.Batch(mixed.datas[:3])
    try:
        assert _c_export(b, _lib.EXPORT_F32, _lib.LAYOUT_PLANAR, *args)[0] == 14
        with pytest.raises(errors.InvalidArgument):
            tensor.export(b)
        b.submit()
        assert _c_export(b, _lib.EXPORT_F32, _lib.LAYOUT_PLANAR, *args)[0] == 14
        b.wait()
        assert _c_export(b, _lib.EXPORT_F32, _lib.LAYOUT_PLANAR, *args)[0] == 0
        assert _c_export(b, 4, _lib.LAYOUT_PLANAR, *args)[0] == 14
        assert _c_export(b, _lib.EXPORT_F32, 2, *args)[0] == 14
        assert _c_export(b, _lib.EXPORT_F32, _lib.LAYOUT_PLANAR, *args, size=16)[0] == 14
        assert _c_export(b, _lib.EXPORT_F32, _lib.LAYOUT_PLANAR, 0, 64, args[2], args[3])[0] == 14
        assert _c_export(b, _lib.EXPORT_F32, _lib.LAYOUT_PLANAR, 2, 0, args[2], args[3])[0] == 14
        assert _c_export(b, _lib.EXPORT_F32, _lib.LAYOUT_PLANAR, 2, 64, None, args[3])[0] == 14
        ms = ctypes.c_double()
        assert b._L.zflac_hip_batch_export_ms(b._h, ctypes.byref(ms)) == 14  # not a timing batch
    finally:
        b.close()
    with pytest.raises(TypeError):
        tensor.export(mixed.batch, dtype=torch.float64)
    with pytest.raises(ValueError):
        tensor.export(mixed.batch, layout="frames")


def test_caller_stream(gpu_ready):
    """Two back-to-back exports with different starts on a torch side stream, a torch op
    behind them, one synchronise: both tensors are right. The same after another run, and
    with stream = NULL through the C call. (A timing batch: the synchronous export reports
    its device time.)"""
    m = Mixed(timing=True)
    try:
        C, T = 2, 4096 + 512
        s1, s2 = _window_starts(m, 1), _window_starts(m, 5)
        side = torch.cuda.Stream()
        for _ in range(2):
            with torch.cuda.stream(side):
                a, la = tensor.export(m.batch, frames=T, channels=C, starts=s1, stream=side)
                b, lb = tensor.export(m.batch, frames=T, channels=C, starts=s2, stream=side)
                total = a.sum() + b.sum()  # a consumer on the same stream, ordered after both
            side.synchronize()
            for x, ln, st in ((a, la, s1), (b, lb, s2)):
                want, valid = m.expect(C, T, st, "float32", "planar")
                np.testing.assert_array_equal(bits_of(x, "float32"), want)
                assert ln.cpu().tolist() == valid
            assert np.isfinite(total.item())
            m.batch.run()  # waits for nothing on the host; the run's streams wait for the exports
        dst = torch.empty((len(m.datas), C, T), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rc, valid = _c_export(m.batch, _lib.EXPORT_F32, _lib.LAYOUT_PLANAR, C, T, dst.data_ptr(), dst.numel() * 4,
                              starts=s1)
        assert rc == 0
        want, want_valid = m.expect(C, T, s1, "float32", "planar")
        np.testing.assert_array_equal(bits_of(dst, "float32"), want)
        assert valid == want_valid
        ms = ctypes.c_double(-1.0)
        assert m.batch._L.zflac_hip_batch_export_ms(m.batch._h, ctypes.byref(ms)) == 0 and ms.value > 0
        # an export left pending on the side stream when the batch is destroyed: destroy waits
        with torch.cuda.stream(side):
            a, _ = tensor.export(m.batch, frames=T, channels=C, starts=s2, stream=side)
    finally:
        m.batch.close()
    side.synchronize()
    np.testing.assert_array_equal(bits_of(a, "float32"), m.expect(C, T, s2, "float32", "planar")[0])


def test_sequential_planner_output(gpu_ready):
    """force_slow: every stream goes through the sequential planner (its own output storage
    where the stream outgrows its region); the export reads the same values."""
    m = Mixed(force_slow=True)
    try:
        for dtype, layout in (("float32", "planar"), ("int32", "interleaved")):
            check(m, 8, max(m.frames), None, dtype, layout)
    finally:
        m.batch.close()


def test_decode_to_tensor(mixed):
    datas = [mixed.datas[1], mixed.datas[0], mixed.datas[-1]]  # stereo 16, mono 8, InvalidFrameHeader
    x, lengths, infos = tensor.decode_to_tensor(datas, dtype=torch.float16)
    n1, n0 = mixed.frames[1], mixed.frames[0]
    assert tuple(x.shape) == (3, 2, max(n0, n1)) and x.dtype == torch.float16 and x.device == torch.device("cuda", 0)
    assert lengths.dtype == torch.int64 and lengths.cpu().tolist() == [n1, n0, 0]
    for k, i in enumerate((1, 0)):
        r = mixed.oracle[i]
        assert infos[k] == ("OK", r.channels, r.sample_rate, r.bits_per_sample)
    assert (infos[0][1], infos[0][3], infos[1][1], infos[1][3]) == (2, 16, 1, 8)
    assert infos[2][0] == "InvalidFrameHeader"
    got = bits_of(x, "float16")
    for row, i in enumerate((1, 0, len(mixed.datas) - 1)):
        s, c, _ = mixed.ref[i]
        np.testing.assert_array_equal(got[row], expected_row(s, c, 2, max(n0, n1), 0, "float16", "planar")[0])
    # out= is checked: dtype, contiguity, shape, device
    b = mixed.batch
    B = len(mixed.datas)
    good = torch.empty((B, 2, 128), dtype=torch.float32, device="cuda")
    y, _ = tensor.export(b, frames=128, channels=2, out=good)
    assert y is good
    with pytest.raises(TypeError):
        tensor.export(b, frames=128, channels=2, out=torch.empty((B, 2, 128), dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        tensor.export(b, frames=128, channels=2, out=torch.empty((B, 2, 256), device="cuda")[:, :, ::2])
    with pytest.raises(ValueError):
        tensor.export(b, frames=128, channels=2, out=torch.empty((B, 2, 127), device="cuda"))
    with pytest.raises(ValueError):
        tensor.export(b, frames=128, channels=2, out=torch.empty((B, 2, 128)))


def test_64bit_indexing(gpu_ready):
    """One mono 16-bit stream, C = 1, f16, T = 2^32 + 4096 (8 GiB, nearly all zero fill):
    element offsets past 2^32."""
    st = synth.generate(**dict(PARITY_CONFIGS["c2_mono16_fixed2_k4"], seed=3100))
    r = oracle.decode(st.flac)
    assert r.error == "OK" and r.channels == 1
    n = r.samples.size
    T = 2 ** 32 + 4096
    try:
        out = torch.empty((1, 1, T), dtype=torch.float16, device="cuda")
    except torch.cuda.OutOfMemoryError:
        pytest.skip("no room for the 8 GiB destination")
    b = zflac_amd.Batch([st.flac])
    try:
        b.run()
        x, lengths = tensor.export(b, frames=T, channels=1, dtype=torch.float16, out=out)
        torch.cuda.synchronize()
        assert lengths.cpu().tolist() == [n]
        want, _ = expected_row(np.ascontiguousarray(r.samples), 1, 1, n, 0, "float16", "planar")
        np.testing.assert_array_equal(bits_of(x[..., :n], "float16")[0], want)
        assert not x[..., n:].view(torch.int16).any().item()
        # and a window far in: the last tile of the row starts past element 2^32
        tail = x[0, 0, T - 4096:].view(torch.int16).cpu().numpy()
        assert not tail.any()
    finally:
        b.close()
        del out
