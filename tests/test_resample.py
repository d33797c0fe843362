"""GPU tests of the resampled dense export (zflac_hip_batch_export_resampled / k_resample,
zflac_amd.tensor.export(sample_rate=...)): one mixed-rate batch to 16 kHz and 48 kHz against the
float64 reference (tests/resample_ref.py) within its f32 error bound, same-rate rows against the
plain export bit for bit, windows against the full export bit for bit, the rounding to f16 and
bf16, tiles, table placement, coverage and bounds of the destination, state and argument errors,
caller streams and the Python layer."""
import ctypes

import torch  # before zflac_amd loads its library: one HIP runtime per process (zflac_amd/tensor.py)

import numpy as np
import pytest

import oracle
import synth
import zflac_amd
from zflac_amd import _lib, errors, tensor

from . import malformed
from . import resample_ref as ref
from .export_ref import BIT_VIEW
from .test_export import bits_of
from .test_resample_plan import probe  # noqa: F401  (the tile rule, from the library's own planner)

pytestmark = pytest.mark.gpu

TARGETS = (16000, 48000)
LAYOUTS = ("planar", "interleaved")
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
C_FULL = 3  # the 3-channel stream whole, stereo and mono with zero planes

# name -> flacgen overrides; a few blocks each. rate_code_mode: 0 the table code, 1 the 16-bit Hz
# field; 768 kHz fits neither and is read from STREAMINFO.
STREAMS = {
    "mono8_8000": dict(channels=1, bps=8, order=3, precision=7, block_size=576, n_samples=3 * 576 + 77, sample_rate=8000),
    "mono16_22050": dict(channels=1, bps=16, order=6, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=22050),
    "stereo16_44100": dict(channels=2, bps=16, stereo_mode=10, order=8, block_size=1024, n_samples=3 * 1024 + 77,
                           sample_rate=44100),
    "stereo16_48000": dict(channels=2, bps=16, stereo_mode=1, order=8, block_size=1024, n_samples=3 * 1024 + 77,
                           sample_rate=48000),
    "ch3_16_37800": dict(channels=3, bps=16, order=6, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=37800,
                         rate_code_mode=1),
    "stereo24_96000": dict(channels=2, bps=24, stereo_mode=1, order=8, precision=14, block_size=2048,
                           n_samples=3 * 2048 + 77, sample_rate=96000),
    "stereo32_768000": dict(channels=2, bps=32, stereo_mode=1, order=8, precision=15, block_size=4096,
                            n_samples=3 * 4096 + 77, tone_amp=0.2, noise_lsb=1e6, sample_rate=768000),
    "stereo16_11025": dict(channels=2, bps=16, stereo_mode=10, order=8, block_size=576, n_samples=3 * 576 + 77,
                           sample_rate=11025, rate_code_mode=1),
    "stereo16_16000": dict(channels=2, bps=16, stereo_mode=10, order=8, block_size=576, n_samples=3 * 576 + 77,
                           sample_rate=16000),
    # shorter than the filter's half width at either target
    "five_frames_44100": dict(channels=2, bps=16, predictor=0, stereo_mode=1, block_size=16, n_samples=5,
                              sample_rate=44100),
    "one_frame_44100": dict(channels=2, bps=16, predictor=0, stereo_mode=1, block_size=16, n_samples=1,
                            sample_rate=44100),
}
BAD = ["wrong_md5", "bad_sync_frame2"]


def _desc(dtype, layout, C, T, starts, rate, zeros=16, rolloff=ref.ROLLOFF, beta=ref.BETA, reserved=0, size=None):
    return _lib.zflac_resample_desc(ctypes.sizeof(_lib.zflac_resample_desc) if size is None else size, dtype, layout, C,
                                    T, starts, rate, zeros, reserved, rolloff, beta)


def c_export(batch, dtype, layout, C, T, dst_ptr, dst_bytes, rate, starts=None, stream=None, **kw):
    n = len(batch)
    h_starts = (ctypes.c_uint64 * n)(*starts) if starts is not None else None
    valid = (ctypes.c_uint64 * n)()
    d = _desc(dtype, layout, C, T, h_starts, rate, **kw)
    rc = batch._L.zflac_hip_batch_export_resampled(batch._h, ctypes.byref(d), dst_ptr, dst_bytes, valid, stream)
    return rc, list(valid)


def tables_built(batch):
    built, held = ctypes.c_uint64(), ctypes.c_uint64()
    assert batch._L.zflac_hip_batch_resample_tables(batch._h, ctypes.byref(built), ctypes.byref(held)) == 0
    return built.value, held.value


class Mixed:
    """The shared batch, the oracle's verdict on each stream, one completed run, and per target
    the float64 reference of every stream resampled whole (computed once, never modified)."""

    def __init__(self, configs=STREAMS, bad=BAD, **batch_kw):
        cases = malformed.cases()
        self.names = list(configs) + list(bad)
        self.datas = [synth.generate(**dict(cfg, seed=5000 + i)).flac for i, cfg in enumerate(configs.values())]
        self.datas += [cases[c][0] for c in bad]
        self.oracle = [oracle.decode(d) for d in self.datas]
        for cfg, r in zip(configs.values(), self.oracle):  # the streams are what the list says
            assert r.error == "OK" and r.sample_rate == cfg["sample_rate"] and r.channels == cfg["channels"], cfg
            assert r.samples.size == cfg["n_samples"] * cfg["channels"]
        self.samples = [np.ascontiguousarray(r.samples) if r.error == "OK" else None for r in self.oracle]
        self.nch = [int(r.channels) if r.error == "OK" else 0 for r in self.oracle]
        self.rate = [int(r.sample_rate) if r.error == "OK" else 0 for r in self.oracle]
        self.n_in = [s.size // c if s is not None else 0 for s, c in zip(self.samples, self.nch)]
        self.batch = zflac_amd.Batch(self.datas, device_md5=True, **batch_kw)
        self.batch.run()
        self.whole, self.tol, self.n_out = {}, {}, {}
        for fout in TARGETS:
            rows, tols = [], []
            for s, c, fin in zip(self.samples, self.nch, self.rate):
                if s is None:
                    rows.append(None)
                    tols.append(0.0)
                elif fin == fout:  # not filtered: the plain export's f32, exactly
                    rows.append(ref.to_f32(s).reshape(-1, c))
                    tols.append(0.0)
                else:
                    table = ref.taps(fin, fout)
                    rows.append(ref.resample(s, c, fin, fout, table=table))
                    tols.append(ref.tol(table[4]))
            for r in rows:
                if r is not None:
                    r.setflags(write=False)
            self.whole[fout], self.tol[fout] = rows, tols
            self.n_out[fout] = [r.shape[0] if r is not None else 0 for r in rows]
        self._full = {}

    def expect(self, fout, C, T, starts, layout):
        rows, valid = [], []
        for i, w in enumerate(self.whole[fout]):
            row, v = ref.expected_row(w, C, T, starts[i] if starts is not None else 0, layout)
            rows.append(row)
            valid.append(v)
        return np.stack(rows), valid

    def full(self, fout, layout):
        """The whole batch at `fout`, f32, C_FULL channels, T = the longest row + 5: (host f32
        array, valid lengths). Exported once per (target, layout)."""
        key = (fout, layout)
        if key not in self._full:
            T = max(self.n_out[fout]) + 5
            x, lengths = tensor.export(self.batch, frames=T, channels=C_FULL, layout=layout, sample_rate=fout)
            torch.cuda.synchronize()
            self._full[key] = (x.cpu().numpy(), lengths.cpu().tolist())
            self._full[key][0].setflags(write=False)
        return self._full[key]


@pytest.fixture(scope="module")
def mixed(gpu_ready):
    m = Mixed()
    yield m
    m.batch.close()


def test_streams_are_what_the_list_says(mixed):
    for i, r in enumerate(mixed.oracle):
        assert errors.NAMES.get(mixed.batch.info(i)[0]) == r.error, mixed.names[i]
        if r.error == "OK":
            assert mixed.batch.info(i)[1].sample_rate == r.sample_rate
    assert [r.error for r in mixed.oracle[-2:]] == ["InvalidChecksum", "InvalidFrameHeader"]
    assert sorted(set(mixed.rate)) == [0, 8000, 11025, 16000, 22050, 37800, 44100, 48000, 96000, 768000]
    # the two short streams lie inside the filter's half width at either target
    for fout in TARGETS:
        assert ref.ratio(44100, fout)[2] > 5


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fout", TARGETS)
def test_parity(mixed, fout, layout):
    """Every element of every row within tol of the float64 reference; valid lengths equal; error
    rows all zero with length 0; rows that are not filtered exact."""
    got, lengths = mixed.full(fout, layout)
    T = got.shape[2] if layout == "planar" else got.shape[1]
    want, valid = mixed.expect(fout, C_FULL, T, None, layout)
    assert got.shape == want.shape and got.dtype == np.float32
    assert lengths == valid == [min(n, T) for n in mixed.n_out[fout]]
    for i, name in enumerate(mixed.names):
        err = float(np.abs(got[i].astype(np.float64) - want[i]).max())
        print(f"{fout} {layout} {name}: max |error| {err:.3e}, tol {mixed.tol[fout][i]:.3e}")
        assert err <= mixed.tol[fout][i], (name, fout, layout, err, mixed.tol[fout][i])
        if mixed.samples[i] is None:
            assert lengths[i] == 0 and not got[i].view(np.uint32).any()
    for i, n in enumerate(mixed.n_in):
        if mixed.samples[i] is not None:
            assert mixed.n_out[fout][i] == ref.out_frames(n, mixed.rate[i], fout)


def test_reference_tolerances():
    """tol at the default parameters: the figures the bound was argued with."""
    assert ref.tol(ref.taps(44100, 16000)[4]) == pytest.approx(1.2e-5, rel=0.1)
    assert ref.tol(ref.taps(8000, 16000)[4]) == pytest.approx(5e-6, rel=0.1)
    assert ref.tol(ref.taps(768000, 16000)[4]) == pytest.approx(2.0e-4, rel=0.1)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fout", TARGETS)
def test_same_rate_rows_are_the_plain_exports(mixed, fout, layout):
    i = mixed.rate.index(fout)
    got, _ = mixed.full(fout, layout)
    T = got.shape[2] if layout == "planar" else got.shape[1]
    plain, lengths = tensor.export(mixed.batch, frames=T, channels=C_FULL, layout=layout)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got[i].view(np.uint32), bits_of(plain, "float32")[i])
    assert lengths.cpu().tolist()[i] == mixed.n_in[i]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_half_dtypes_round_the_f32_result(mixed, dtype, layout):
    """The f16 / bf16 output is the f32 output of the same export rounded as the plain export
    rounds (export_ref.convert_bits): bit for bit."""
    for fout in TARGETS:
        f32, lengths32 = mixed.full(fout, layout)
        T = f32.shape[2] if layout == "planar" else f32.shape[1]
        x, lengths = tensor.export(mixed.batch, frames=T, channels=C_FULL, layout=layout, sample_rate=fout,
                                   dtype=DTYPES[dtype])
        torch.cuda.synchronize()
        assert x.dtype == DTYPES[dtype] and lengths.cpu().tolist() == lengths32
        np.testing.assert_array_equal(bits_of(x, dtype), ref.round_bits(f32, dtype).reshape(f32.shape))
        assert BIT_VIEW[dtype] is np.uint16


def _starts(m, fout, shift):
    out = []
    for i, n in enumerate(m.n_out[fout]):
        cand = [0, 1, 63, 64, 65, max(n - 1, 0), n, n + 5, 2 ** 40]
        out.append(cand[(i + shift) % len(cand)])
    return out


@pytest.mark.parametrize("T", [1, 7, 64, 1000])
def test_windows(mixed, T):
    """Per-row starts from {0, 1, 63, 64, 65, N-1, N, N+5, 2^40} (N the row's resampled length),
    every row taking every start in turn: each window is bit-identical to that slice of the
    full export, zero after the stream's end, and valid_frames is clamp(N - start, 0, T)."""
    for fout in TARGETS:
        for shift in range(9):
            layout = LAYOUTS[shift % 2]
            full, _ = mixed.full(fout, layout)
            full = full if layout == "planar" else full.transpose(0, 2, 1)  # [B, C, frames]
            starts = _starts(mixed, fout, shift)
            x, lengths = tensor.export(mixed.batch, frames=T, channels=C_FULL, starts=starts, layout=layout,
                                       sample_rate=fout)
            torch.cuda.synchronize()
            got = x.cpu().numpy()
            got = got if layout == "planar" else got.transpose(0, 2, 1)
            want_valid = [min(max(n - s, 0), T) for n, s in zip(mixed.n_out[fout], starts)]
            assert lengths.cpu().tolist() == want_valid
            for i, (s, v) in enumerate(zip(starts, want_valid)):
                want = np.zeros((C_FULL, T), dtype=np.float32)
                want[:, :v] = full[i][:, s:s + v]
                np.testing.assert_array_equal(got[i].view(np.uint32), want.view(np.uint32),
                                              err_msg=f"{fout} {layout} {mixed.names[i]} start {s} T {T}")


def test_tiles(gpu_ready, probe):  # noqa: F811
    """The tile rule (resample_tile in resample_plan.cpp): a workgroup takes `tile` output frames
    of a row, the largest multiple of its 512 lanes (at most 2,048; of 64 below 512) whose input
    span, ceil((tile - 1) M / L) + K frames for each of the channels staged together, fits the
    80 KiB of LDS beside the table.
    For stereo 44.1 k -> 16 k that is 512, for mono 22.05 k -> 48 k 2,048. Both streams cross three
    tiles; the first ends one frame past a tile boundary (1,025 frames). A second window starts
    inside a tile, so the same frames fall into other tiles: same bits."""
    tile, cg, tab, lds = (ctypes.c_uint() for _ in range(4))
    probe.resample_probe_tile(44100, 16000, 16, ref.ROLLOFF, 2, tile, cg, tab, lds)
    assert (tile.value, cg.value, lds.value) == (512, 2, 20480)
    probe.resample_probe_tile(22050, 48000, 16, ref.ROLLOFF, 1, tile, cg, tab, lds)
    assert (tile.value, cg.value) == (2048, 1)
    cfgs = {"down": dict(channels=2, bps=16, stereo_mode=10, order=8, block_size=1024, n_samples=2823, sample_rate=44100),
            "up": dict(channels=1, bps=16, order=6, block_size=1024, n_samples=1883, sample_rate=22050)}
    datas = [synth.generate(**dict(c, seed=5100 + i)).flac for i, c in enumerate(cfgs.values())]
    refs = [oracle.decode(d) for d in datas]
    assert [r.error for r in refs] == ["OK", "OK"]
    assert ref.out_frames(2823, 44100, 16000) == 2 * 512 + 1 and ref.out_frames(1883, 22050, 48000) == 4100 > 2 * 2048
    b = zflac_amd.Batch(datas)
    try:
        b.run()
        for i, (r, fout) in enumerate(zip(refs, TARGETS)):
            table = ref.taps(r.sample_rate, fout)
            want = ref.resample(np.ascontiguousarray(r.samples), r.channels, r.sample_rate, fout, table=table)
            x, lengths = tensor.export(b, channels=2, sample_rate=fout)
            y, _ = tensor.export(b, channels=2, sample_rate=fout, starts=[37, 37], frames=x.shape[2])
            torch.cuda.synchronize()
            got = x.cpu().numpy()[i].T  # [frames, 2]
            assert lengths.cpu().tolist()[i] == want.shape[0]
            err = float(np.abs(got[:want.shape[0], :r.channels].astype(np.float64) - want).max())
            print(f"tiles {r.sample_rate} -> {fout}: max |error| {err:.3e}, tol {ref.tol(table[4]):.3e}")
            assert err <= ref.tol(table[4])
            assert not got[want.shape[0]:].any() and not got[:, r.channels:].any()
            np.testing.assert_array_equal(y.cpu().numpy()[i][:, :want.shape[0] - 37].view(np.uint32),
                                          x.cpu().numpy()[i][:, 37:want.shape[0]].view(np.uint32))
    finally:
        b.close()


def test_table_placement(mixed, probe):  # noqa: F811
    """48 k -> 16 k keeps its 115-float table in LDS, 11.025 k -> 16 k reads its 24,960 floats from
    global memory (more than the 16,896 floats of LDS a table may take); both rows are in the
    mixed batch and pass test_parity. 44.1 k -> 16 k (16,800 floats) is in LDS as well."""
    tile, cg, tab, lds = (ctypes.c_uint() for _ in range(4))
    for fin, want in ((48000, 1), (44100, 1), (11025, 0)):
        probe.resample_probe_tile(fin, 16000, 16, ref.ROLLOFF, 2, tile, cg, tab, lds)
        assert tab.value == want, fin
        assert fin in mixed.rate
    got, _ = mixed.full(16000, "planar")
    for fin in (48000, 11025):
        i = mixed.rate.index(fin)
        want, _ = ref.expected_row(mixed.whole[16000][i], C_FULL, got.shape[2], 0, "planar")
        assert np.abs(got[i] - want).max() <= mixed.tol[16000][i]


@pytest.mark.parametrize("offset", [64, 68])  # a 16-byte aligned destination and one at base + 4
@pytest.mark.parametrize("layout", LAYOUTS)
def test_coverage_and_bounds(mixed, layout, offset):
    """The destination is a slice of a larger buffer of 0xFF bytes (a NaN pattern as f32): every
    element inside is written, nothing outside is, a dst_bytes one element short writes nothing,
    and the values do not depend on the destination's alignment."""
    fout = 16000
    full, full_valid = mixed.full(fout, layout)
    C, B = C_FULL, len(mixed.datas)
    T = full.shape[2] if layout == "planar" else full.shape[1]
    need = B * C * T * 4
    buf = torch.full((offset + need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lay = _lib.LAYOUT_PLANAR if layout == "planar" else _lib.LAYOUT_INTERLEAVED
    rc, _ = c_export(mixed.batch, _lib.EXPORT_F32, lay, C, T, buf.data_ptr() + offset, need - 4, fout)
    assert rc == 14
    assert bool((buf == 0xFF).all().item()), "a refused export wrote to the destination"
    rc, valid = c_export(mixed.batch, _lib.EXPORT_F32, lay, C, T, buf.data_ptr() + offset, need, fout)
    assert rc == 0
    host = buf.cpu().numpy()
    assert (host[:offset] == 0xFF).all() and (host[offset + need:] == 0xFF).all()
    inside = host[offset:offset + need].copy().view(np.uint32)
    assert not (inside == 0xFFFFFFFF).any(), "elements of the destination were left unwritten"
    np.testing.assert_array_equal(inside.reshape(full.shape), full.view(np.uint32))
    assert valid == full_valid


def test_state_and_arguments(mixed):
    """14 before the first run, between submit and wait, and for I32, rate 0, zeros 0, a reserved
    field, rolloff or beta out of range, a rate above 2^20 - 1 and a K above 4,096 taps; none of
    them writes."""
    B = len(mixed.datas)
    dst = torch.full((B, 2, 64), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    args = (2, 64, dst.data_ptr(), dst.numel() * 4)
    F32, PL = _lib.EXPORT_F32, _lib.LAYOUT_PLANAR
    b = zflac_amd.Batch(mixed.datas[:3])
    try:
        assert c_export(b, F32, PL, *args, 16000)[0] == 14
        with pytest.raises(errors.InvalidArgument):
            tensor.export(b, sample_rate=16000)
        b.submit()
        assert c_export(b, F32, PL, *args, 16000)[0] == 14
        b.wait()
    finally:
        b.close()
    m = mixed.batch
    assert c_export(m, _lib.EXPORT_I32, PL, *args, 16000)[0] == 14
    assert c_export(m, 4, PL, *args, 16000)[0] == 14
    assert c_export(m, F32, 2, *args, 16000)[0] == 14
    assert c_export(m, F32, PL, *args, 0)[0] == 14
    assert c_export(m, F32, PL, *args, 1048576)[0] == 14
    assert c_export(m, F32, PL, *args, 16000, zeros=0)[0] == 14
    assert c_export(m, F32, PL, *args, 16000, reserved=1)[0] == 14
    assert c_export(m, F32, PL, *args, 16000, rolloff=0.0)[0] == 14
    assert c_export(m, F32, PL, *args, 16000, rolloff=1.5)[0] == 14
    assert c_export(m, F32, PL, *args, 16000, beta=-1.0)[0] == 14
    assert c_export(m, F32, PL, *args, 16000, size=24)[0] == 14
    assert c_export(m, F32, PL, 0, 64, args[2], args[3], 16000)[0] == 14
    assert c_export(m, F32, PL, 2, 0, args[2], args[3], 16000)[0] == 14
    assert c_export(m, F32, PL, 2, 64, None, args[3], 16000)[0] == 14
    # the 768 kHz stream at zeros = 64: W = ceil(64 * 48 / 0.85) = 3,615, K = 7,231 > 4,096
    assert ref.ratio(768000, 16000, 64)[3] == 7231
    assert c_export(m, F32, PL, *args, 16000, zeros=64)[0] == 14
    # 1,048,575 shares 25 or 75 with the batch's rates: nine tables of 13,981 or 41,943 phases x 39
    # taps, 7.1 M floats together, past the call's 4 Mi
    assert c_export(m, F32, PL, *args, 1048575)[0] == 14
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all().item()), "a refused export wrote to the destination"
    assert c_export(m, F32, PL, *args, 16000)[0] == 0
    with pytest.raises(TypeError):
        tensor.export(m, sample_rate=16000, dtype=torch.int32)
    with pytest.raises(ValueError):
        tensor.export(m, sample_rate=0)


def test_caller_stream_tables_and_the_next_run(gpu_ready):
    """On a torch side stream a torch op behind the export sees the complete tensor; the batch's
    next run() still decodes bit-exactly; a second export with the same parameters builds no
    table (observed through zflac_hip_batch_resample_tables' count of tables built, not through
    timing); a synchronous export of a timing batch reports its device time."""
    cfgs = {k: STREAMS[k] for k in ("stereo16_44100", "mono8_8000", "stereo16_16000", "stereo24_96000")}
    m = Mixed(cfgs, bad=[], timing=True)
    try:
        assert tables_built(m.batch) == (0, 0)
        fout, T = 16000, max(m.n_out[16000]) + 3
        want, valid = m.expect(fout, 2, T, None, "planar")
        side = torch.cuda.Stream()
        for rep in range(2):
            with torch.cuda.stream(side):
                x, lengths = tensor.export(m.batch, frames=T, channels=2, sample_rate=fout, stream=side)
                total = x.abs().sum(dim=(1, 2))  # a consumer on the same stream, ordered after the export
            side.synchronize()
            got = x.cpu().numpy()
            for i in range(len(m.datas)):
                assert np.abs(got[i] - want[i]).max() <= m.tol[fout][i]
            assert lengths.cpu().tolist() == valid
            np.testing.assert_allclose(total.cpu().numpy(), np.abs(got).sum(axis=(1, 2), dtype=np.float64), rtol=1e-4)
            # three streams are filtered (44.1 k, 8 k, 96 k), one is not: three tables, built once
            built, held = tables_built(m.batch)
            assert built == 3 and held == sum(ref.ratio(f, fout)[0] * ref.ratio(f, fout)[3] for f in (44100, 8000, 96000))
            m.batch.run()  # waits for nothing on the host; the run's streams wait for the export
            for i, r in enumerate(m.oracle):
                assert np.array_equal(m.batch.read(i).samples.values, r.samples), i
        # other parameters are another set of tables; the first set stays
        x2, _ = tensor.export(m.batch, frames=T, channels=2, sample_rate=fout, resample_zeros=8)
        torch.cuda.synchronize()
        assert tables_built(m.batch)[0] == 6
        tensor.export(m.batch, frames=T, channels=2, sample_rate=fout)
        assert tables_built(m.batch)[0] == 6
        # stream = NULL through the C call: complete on return, and timed
        dst = torch.empty((len(m.datas), 2, T), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rc, c_valid = c_export(m.batch, _lib.EXPORT_F32, _lib.LAYOUT_PLANAR, 2, T, dst.data_ptr(), dst.numel() * 4, fout)
        assert rc == 0 and c_valid == valid
        np.testing.assert_array_equal(bits_of(dst, "float32"), got.view(np.uint32))
        ms = ctypes.c_double(-1.0)
        assert m.batch._L.zflac_hip_batch_export_ms(m.batch._h, ctypes.byref(ms)) == 0 and ms.value > 0
        # an export left pending on the side stream when the batch is destroyed: destroy waits
        with torch.cuda.stream(side):
            a, _ = tensor.export(m.batch, frames=T, channels=2, sample_rate=fout, stream=side)
    finally:
        m.batch.close()
    side.synchronize()
    np.testing.assert_array_equal(bits_of(a, "float32"), got.view(np.uint32))


def test_python_layer(mixed):
    x, lengths = tensor.export(mixed.batch, sample_rate=16000)
    longest = max(mixed.n_out[16000])
    assert tuple(x.shape) == (len(mixed.datas), 3, longest) and x.dtype == torch.float32
    assert lengths.cpu().tolist() == mixed.n_out[16000]
    full, _ = mixed.full(16000, "planar")
    np.testing.assert_array_equal(bits_of(x, "float32"), full[:, :, :longest].view(np.uint32))
    # starts move the default length with them
    starts = [10] * len(mixed.datas)
    y, ly = tensor.export(mixed.batch, sample_rate=16000, starts=starts)
    assert y.shape[2] == longest - 10 and ly.cpu().tolist() == [max(n - 10, 0) for n in mixed.n_out[16000]]
    # decode_to_tensor: rows of one rate, whatever the streams' own
    pick = [mixed.names.index(n) for n in ("stereo16_44100", "mono8_8000", "stereo16_16000", "bad_sync_frame2")]
    x, lengths, infos = tensor.decode_to_tensor([mixed.datas[i] for i in pick], sample_rate=16000)
    want_n = [mixed.n_out[16000][i] for i in pick]
    assert tuple(x.shape) == (4, 2, max(want_n)) and lengths.cpu().tolist() == want_n
    assert [inf[2] for inf in infos[:3]] == [44100, 8000, 16000] and infos[3][0] == "InvalidFrameHeader"
    got = x.cpu().numpy()
    for row, i in enumerate(pick):
        want, _ = ref.expected_row(mixed.whole[16000][i], 2, max(want_n), 0, "planar")
        assert np.abs(got[row] - want).max() <= mixed.tol[16000][i], mixed.names[i]
    with pytest.raises(TypeError):
        tensor.decode_to_tensor([mixed.datas[0]], sample_rate=16000, dtype=torch.int32)
