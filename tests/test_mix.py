"""GPU tests of the mixed exports (zflac_hip_batch_export_mixed / k_export_mixed,
zflac_hip_batch_export_resampled_mixed / k_resample_mixed, zflac_amd.tensor.export(mix=...)): one
batch of mono .. 8-channel streams of mixed rates and containers against tests/mix_ref.py: bit
for bit where the arithmetic is exact, within the derived f32 bounds elsewhere; rows without a
matrix against the unmixed exports bit for bit; identities, windows, coverage and bounds of the
destination, arguments, the matrices' lifetime, ordering with the next run, the Python layer."""
import ctypes

import torch  # before zflac_amd loads its library: one HIP runtime per process (zflac_amd/tensor.py)

import numpy as np
import pytest

import oracle
import synth
import zflac_amd
from zflac_amd import _lib, tensor

from . import malformed
from . import mix_ref
from . import resample_ref as ref
from .test_export import bits_of
from .test_resample import STREAMS
from .test_resample_plan import probe  # noqa: F401  (the tile rule, from the library's own planner)
from .util import PARITY_CONFIGS

pytestmark = pytest.mark.gpu

LAYOUTS = ("planar", "interleaved")
LAY = {"planar": _lib.LAYOUT_PLANAR, "interleaved": _lib.LAYOUT_INTERLEAVED}
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
CODE = {"float32": _lib.EXPORT_F32, "float16": _lib.EXPORT_F16, "bfloat16": _lib.EXPORT_BF16, "int32": _lib.EXPORT_I32}
TARGETS = (16000, 48000)
LONG = 2 * 4096 + 77  # crosses two EXPORT_TILE boundaries and ends inside a 16-byte unit

CONFIGS = {
    "mono8": STREAMS["mono8_8000"],
    "mono16": dict(channels=1, bps=16, order=6, block_size=1024, n_samples=3 * 1024 + 77, sample_rate=32000),
    "stereo8": dict(channels=2, bps=8, stereo_mode=10, order=4, precision=7, block_size=1024, n_samples=3 * 1024 + 5,
                    noise_lsb=1.0, tone_amp=0.3, sample_rate=44100),
    "stereo16_44100": STREAMS["stereo16_44100"],
    "stereo24": STREAMS["stereo24_96000"],
    "ch3_16": STREAMS["ch3_16_37800"],
    "ch4_16": PARITY_CONFIGS["ch4_16_lpc12"],
    "ch6_16": dict(channels=6, bps=16, order=6, block_size=1024, n_samples=2 * 1024 + 1),
    "ch6_24": PARITY_CONFIGS["ch6_24_wasted"],
    "ch8_16": PARITY_CONFIGS["ch8_16_fixed"],
    "stereo32_768000": STREAMS["stereo32_768000"],
    "stereo16_48000": STREAMS["stereo16_48000"],
    "mono16_22050": STREAMS["mono16_22050"],
    "stereo16_16000": STREAMS["stereo16_16000"],
    "stereo16_11025": STREAMS["stereo16_11025"],
    "long16": dict(channels=2, bps=16, stereo_mode=10, order=8, block_size=4096, n_samples=LONG, sample_rate=44100),
    "one_frame_44100": STREAMS["one_frame_44100"],
}
BAD = ["wrong_md5"]


def random_mats(C, seed):
    """{n: [C, n] float32}, seeded, coefficients in [-1, 1] (none below 2^-64 in magnitude)."""
    rng = np.random.default_rng(seed)
    out = {n: rng.uniform(-1.0, 1.0, size=(C, n)).astype(np.float32) for n in range(1, 9)}
    assert all((np.abs(m) >= 2.0 ** -64).all() for m in out.values())
    return out


def preset(name):
    return {n: np.asarray(m, dtype=np.float32) for n, m in tensor.mix_preset(name).items()}


def c_mix(batch, mats, dtype, layout, C, T, dst_ptr, dst_bytes, rate=None, starts=None, stream=None, size=None,
          reserved=0, mix_null=False):
    """The C call: mats {n: float32 [C, n] (any shape: the library reads C * n floats)} or None for
    an all-NULL descriptor; mix_null: mix == NULL. -> (rc, valid, the arrays the descriptor points to)."""
    n = len(batch)
    h_starts = (ctypes.c_uint64 * n)(*starts) if starts is not None else None
    valid = (ctypes.c_uint64 * n)()
    mix = _lib.zflac_mix_desc(ctypes.sizeof(_lib.zflac_mix_desc) if size is None else size, reserved)
    keep = []
    for k, m in (mats or {}).items():
        keep.append(np.array(m, dtype=np.float32, order="C"))  # (a copy: a test may overwrite it)
        mix.matrix[k - 1] = keep[-1].ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    pm = None if mix_null else ctypes.byref(mix)
    if rate is None:
        d = _lib.zflac_export_desc(ctypes.sizeof(_lib.zflac_export_desc), CODE[dtype], LAY[layout], C, T, h_starts)
        rc = batch._L.zflac_hip_batch_export_mixed(batch._h, ctypes.byref(d), pm, dst_ptr, dst_bytes, valid, stream)
    else:
        d = _lib.zflac_resample_desc(ctypes.sizeof(_lib.zflac_resample_desc), CODE[dtype], LAY[layout], C, T, h_starts,
                                     rate, 16, 0, ref.ROLLOFF, ref.BETA)
        rc = batch._L.zflac_hip_batch_export_resampled_mixed(batch._h, ctypes.byref(d), pm, dst_ptr, dst_bytes, valid,
                                                             stream)
    return rc, list(valid), keep


def as_bct(x, layout):
    """[B, C, T] view of an exported host array."""
    return x if layout == "planar" else x.transpose(0, 2, 1)


class Mixed:
    """The shared batch, the oracle's verdict on each stream and one completed run. Every
    expectation comes from the oracle's samples; the float64 references are computed once."""

    def __init__(self):
        self.names = list(CONFIGS) + BAD
        self.datas = [synth.generate(**dict(cfg, seed=7000 + i)).flac for i, cfg in enumerate(CONFIGS.values())]
        self.datas += [malformed.cases()[c][0] for c in BAD]
        self.oracle = [oracle.decode(d) for d in self.datas]
        for cfg, r in zip(CONFIGS.values(), self.oracle):
            assert r.error == "OK" and r.channels == cfg["channels"] and r.samples.size == cfg["n_samples"] * cfg["channels"]
        assert self.oracle[-1].error == "InvalidChecksum"
        self.samples = [np.ascontiguousarray(r.samples) if r.error == "OK" else None for r in self.oracle]
        self.nch = [int(r.channels) if r.error == "OK" else 0 for r in self.oracle]
        self.rate = [int(r.sample_rate) if r.error == "OK" else 0 for r in self.oracle]
        self.frames = [s.size // c if s is not None else 0 for s, c in zip(self.samples, self.nch)]
        self.T = max(self.frames) + 3
        self.batch = zflac_amd.Batch(self.datas, device_md5=True)
        self.batch.run()
        self._taps, self._plain = {}, {}

    def i(self, name):
        return self.names.index(name)

    def taps(self, fin, fout):
        if (fin, fout) not in self._taps:
            self._taps[fin, fout] = ref.taps(fin, fout)
        return self._taps[fin, fout]

    def mixed64(self, i, mats, C):
        """[frames, C] float64 of stream i: mixed when mats has its channel count, else the fit rule."""
        s, n = self.samples[i], self.nch[i]
        if n in mats:
            return mix_ref.mix64(s, n, mats[n])
        out = np.zeros((self.frames[i], C))
        out[:, :min(n, C)] = ref.to_f32(s).reshape(-1, n)[:, :C]
        return out

    def plain(self, C, dtype, layout, rate=None):
        """The unmixed export of the whole batch: bits [B, C, T'] (exported once per key)."""
        key = (C, dtype, layout, rate)
        if key not in self._plain:
            T = self.T if rate is None else self.T_at(rate)
            x, lengths = tensor.export(self.batch, frames=T, channels=C, dtype=DTYPES.get(dtype, torch.int32),
                                       layout=layout, sample_rate=rate)
            torch.cuda.synchronize()
            self._plain[key] = (as_bct(bits_of(x, dtype), layout), lengths.cpu().tolist())
        return self._plain[key]

    def T_at(self, rate):
        return max(ref.out_frames(n, f, rate) for n, f in zip(self.frames, self.rate)) + 3

    def export(self, mats, C, dtype="float32", layout="planar", T=None, starts=None, rate=None):
        """tensor.export(mix=mats) -> (host bits [B, C, T], lengths)."""
        T = T or (self.T if rate is None else self.T_at(rate))
        x, lengths = tensor.export(self.batch, frames=T, channels=C, dtype=DTYPES[dtype], layout=layout, starts=starts,
                                   sample_rate=rate, mix=mats)
        torch.cuda.synchronize()
        return as_bct(bits_of(x, dtype), layout), lengths.cpu().tolist()


@pytest.fixture(scope="module")
def mixed(gpu_ready):
    m = Mixed()
    yield m
    m.batch.close()


# ---- 1. exact ------------------------------------------------------------------------------
EXACT = {
    "C1_from_2": (1, {2: [[0.5, 0.5]]}),
    "C2_from_1": (2, {1: [[1.0], [-0.5]]}),
    "C2_from_6": (2, {6: [[1.0, 0.0, 0.5, 0.25, -0.5, 0.0], [0.0, -1.0, 0.5, 0.25, 0.0, 0.5]]}),
    "C3_from_8": (3, {8: [[1, 0, 0.5, 0, -0.5, 0, 0.25, 0], [0, 1, 0.5, 0, 0, -0.5, 0, 0.25], [0.25, -1, 0, 0.5, 0, 0, 1, -0.5]]}),
}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("case", sorted(EXACT))
def test_exact(mixed, case, dtype, layout):
    """8- and 16-bit containers, coefficients from {0, +-1, +-0.5, 0.25}: every product and sum is
    exact in f32, so the rows equal the integer reference bit for bit in every dtype."""
    C, mats = EXACT[case]
    mats = {n: np.asarray(m, dtype=np.float32) for n, m in mats.items()}
    got, lengths = mixed.export(mats, C, dtype, layout)
    (n,) = mats
    hit = [i for i, (c, s) in enumerate(zip(mixed.nch, mixed.samples)) if c == n and s.dtype.itemsize <= 2]
    assert hit, case
    for i in hit:
        want = mix_ref.mix_exact_bits(mixed.samples[i], n, mats[n], dtype).T  # [C, frames]
        N = mixed.frames[i]
        assert lengths[i] == N
        np.testing.assert_array_equal(got[i][:, :N], want, err_msg=f"{case} {mixed.names[i]} {dtype} {layout}")
        assert not got[i][:, N:].any()


# ---- 2. tolerance ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("which", ["random1", "random2", "random3", "random8", "mono", "stereo"])
def test_tolerance(mixed, which, layout):
    """Every stream (24- and 32-bit ones too): |got - float64 reference| <= (n + 1) 2^-24 sum_j |m|.
    The float64 reference rounded to f32 sits inside that bound of itself (the bound is not vacuous:
    it admits the correctly rounded result, and only a few roundings more)."""
    if which.startswith("random"):
        C = int(which[6:])
        mats = random_mats(C, 100 + C)
    else:
        mats, C = preset(which), {"mono": 1, "stereo": 2}[which]
    got, lengths = mixed.export(mats, C, "float32", layout)
    got = got.view(np.float32)
    for i, name in enumerate(mixed.names):
        if mixed.samples[i] is None:
            assert lengths[i] == 0 and not got[i].view(np.uint32).any()
            continue
        n, N = mixed.nch[i], mixed.frames[i]
        want = mixed.mixed64(i, mats, C).T  # [C, N]
        tol = np.array([mix_ref.mix_tol(mats[n][c], n) if n in mats else 0.0 for c in range(C)])[:, None]
        err = np.abs(got[i][:, :N].astype(np.float64) - want)
        print(f"{which} {layout} {name}: max |error| {err.max():.3e}, tol {tol.max():.3e}")
        assert (err <= tol).all(), (which, name, float(err.max()), float(tol.max()))
        assert (np.abs(want.astype(np.float32).astype(np.float64) - want) <= tol).all()
        assert lengths[i] == N and not got[i][:, N:].view(np.uint32).any()


# ---- 3. pass-through ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16", "int32"])
def test_null_mix_is_the_plain_export(mixed, dtype):
    """mix == NULL and an all-NULL mix: the plain export's bits for every dtype, i32 included; with
    only matrix[1] set, every non-stereo row has the plain export's bits."""
    B, C, T = len(mixed.datas), 3, mixed.T
    esz = 4 if dtype in ("float32", "int32") else 2
    for layout in LAYOUTS:
        want, valid = mixed.plain(C, dtype, layout)
        for null in (True, False):
            dst = torch.full((B * C * T * esz,), 0xFF, dtype=torch.uint8, device="cuda")
            rc, v, _ = c_mix(mixed.batch, None, dtype, layout, C, T, dst.data_ptr(), dst.numel(), mix_null=null)
            assert rc == 0 and v == valid
            shape = (B, C, T) if layout == "planar" else (B, T, C)
            got = as_bct(dst.cpu().numpy().view(want.dtype).reshape(shape), layout)
            np.testing.assert_array_equal(got, want)
        if dtype != "int32":
            got, v = mixed.export({2: np.asarray([[0.5, 0.5], [1, 0], [0, 1]], dtype=np.float32)}, C, dtype, layout)
            assert v == valid
            for i, n in enumerate(mixed.nch):
                if n != 2:
                    np.testing.assert_array_equal(got[i], want[i], err_msg=mixed.names[i])
                elif dtype == "float32":  # the identity rows of that matrix are the stream's own channels
                    np.testing.assert_array_equal(got[i][1:], want[i][:2], err_msg=mixed.names[i])


# ---- 4. identities --------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_identities(mixed, layout):
    """The n x n identity at C = n is the plain export's row; the swap matrix exchanges a stereo
    row's planes; an all-zero matrix row is 0x00000000 everywhere (never 0x80000000)."""
    for n in (1, 2, 3, 4, 6, 8):
        want, _ = mixed.plain(n, "float32", layout)
        got, _ = mixed.export({n: np.eye(n, dtype=np.float32)}, n, "float32", layout)
        for i, c in enumerate(mixed.nch):
            np.testing.assert_array_equal(got[i], want[i], err_msg=f"identity {n} {mixed.names[i]}")
    want, _ = mixed.plain(2, "float32", layout)
    got, _ = mixed.export({2: np.asarray([[0, 1], [1, 0]], dtype=np.float32)}, 2, "float32", layout)
    zero, _ = mixed.export({2: np.asarray([[0, 0], [-1, 0]], dtype=np.float32), 6: np.zeros((2, 6), dtype=np.float32)}, 2,
                           "float32", layout)
    for i, c in enumerate(mixed.nch):
        if c == 2:
            np.testing.assert_array_equal(got[i], want[i][::-1], err_msg=mixed.names[i])
            assert not zero[i][0].any(), mixed.names[i]  # +0 in every frame
            assert (zero[i][1] != 0x80000000).all()  # -1 * (+0 sample) is summed onto +0: +0
        if c == 6:
            assert (mixed.samples[i] < 0).any() and not zero[i].any()
    assert (mixed.samples[mixed.i("long16")] < 0).any()


# ---- 5. windows -----------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4095, 4096, 4097, 2 * 4096 + 80])
def test_windows(mixed, T):
    """Odd starts (unaligned loads), windows that end one frame before, at and after a tile
    boundary and past the stream's end: each equals the slice of the full mixed export bit for bit,
    zero after the end; valid_frames is the plain export's."""
    mats = random_mats(2, 55)
    for shift, layout in enumerate(LAYOUTS):
        full, _ = mixed.export(mats, 2, "float32", layout)
        starts = [(1, 3, 63, 65, 4097, max(n - 1, 0), n + 5)[(i + shift) % 7] for i, n in enumerate(mixed.frames)]
        got, lengths = mixed.export(mats, 2, "float32", layout, T=T, starts=starts)
        _, plain_valid = tensor.export(mixed.batch, frames=T, channels=2, starts=starts)
        assert lengths == plain_valid.cpu().tolist() == [min(max(n - s, 0), T) for n, s in zip(mixed.frames, starts)]
        for i, (s, v) in enumerate(zip(starts, lengths)):
            want = np.zeros((2, T), dtype=np.uint32)
            want[:, :v] = full[i][:, s:s + v]
            np.testing.assert_array_equal(got[i], want, err_msg=f"{layout} {mixed.names[i]} start {s} T {T}")


# ---- 6. coverage and bounds -----------------------------------------------------------------
@pytest.mark.parametrize("offset", [64, 68])  # a 16-byte aligned base and one at base + 4 (vec == 0)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_coverage_and_bounds(mixed, layout, offset):
    """The destination is a slice of a larger buffer of 0xFF bytes (a NaN pattern): every element
    inside is written, no guard byte is touched, and the values do not depend on the alignment."""
    mats, C, B, T = random_mats(2, 56), 2, len(mixed.datas), mixed.T  # (a multiple of 4: vec at offset 64)
    assert T % 4 == 0
    full, valid = mixed.export(mats, C, "float32", layout, T=T)
    need = B * C * T * 4
    buf = torch.full((offset + need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, v, _ = c_mix(mixed.batch, mats, "float32", layout, C, T, buf.data_ptr() + offset, need)
    assert rc == 0 and v == valid
    host = buf.cpu().numpy()
    assert (host[:offset] == 0xFF).all() and (host[offset + need:] == 0xFF).all()
    inside = host[offset:offset + need].copy().view(np.uint32)
    assert not (inside == 0xFFFFFFFF).any(), "elements of the destination were left unwritten"
    shape = (B, C, T) if layout == "planar" else (B, T, C)
    np.testing.assert_array_equal(as_bct(inside.reshape(shape), layout), full)


# ---- 7. resampled, mixed --------------------------------------------------------------------
@pytest.mark.parametrize("fout", TARGETS)
@pytest.mark.parametrize("which", ["random2", "mono"])
def test_resampled(mixed, which, fout):
    """Mix, then filter: against resample_ref.resample over the float64 mixed frames within
    (K + n + 5) 2^-24 max_r sum_k |h| max(1, sum_j |m|). Rows already at the target rate have the
    mixed plain export's bits; rows with a NULL matrix the unmixed resampled export's."""
    mats, C = (random_mats(2, 77), 2) if which == "random2" else (preset("mono"), 1)
    got, lengths = mixed.export(mats, C, "float32", "planar", rate=fout)
    same, _ = mixed.export(mats, C, "float32", "planar")
    unmixed, valid = mixed.plain(C, "float32", "planar", rate=fout)
    assert lengths == valid
    for i, name in enumerate(mixed.names):
        n, fin = mixed.nch[i], mixed.rate[i]
        if mixed.samples[i] is None:
            assert not got[i].any()
        elif n not in mats:
            np.testing.assert_array_equal(got[i], unmixed[i], err_msg=name)
        elif fin == fout:
            N = mixed.frames[i]
            np.testing.assert_array_equal(got[i][:, :N], same[i][:, :N], err_msg=name)
            assert not got[i][:, N:].any()
        else:
            table = mixed.taps(fin, fout)
            want = ref.resample(mix_ref.mix64(mixed.samples[i], n, mats[n]), C, fin, fout, table=table).T
            N = want.shape[1]
            assert lengths[i] == N
            tol = np.array([mix_ref.resample_mix_tol(table[4], mats[n][c], n) for c in range(C)])[:, None]
            err = np.abs(got[i].view(np.float32)[:, :N].astype(np.float64) - want)
            print(f"{which} -> {fout} {name}: max |error| {err.max():.3e}, tol {tol.min():.3e}")
            assert (err <= tol).all(), (name, float(err.max()), float(tol.min()))
            assert not got[i][:, N:].any()


@pytest.mark.parametrize("name,staged_tab", [("stereo16_44100", 1), ("stereo16_11025", 0)])
def test_resampled_windows(mixed, probe, name, staged_tab):  # noqa: F811
    """Stereo -> mono stages one channel: the planner's tile for (ratio, 1 staged channel), and a
    window that starts inside that tile, so that its frames fall into other tiles: same bits. Once
    with the table in LDS (44.1 k -> 16 k), once with the taps read from global memory (11.025 k)."""
    fout, i = 16000, mixed.i(name)
    tile, cg, tab, lds = (ctypes.c_uint() for _ in range(4))
    probe.resample_probe_tile(mixed.rate[i], fout, 16, ref.ROLLOFF, 1, tile, cg, tab, lds)
    assert cg.value == 1 and tab.value == staged_tab
    two = ctypes.c_uint()
    probe.resample_probe_tile(mixed.rate[i], fout, 16, ref.ROLLOFF, 2, two, cg, tab, lds)
    assert tile.value >= two.value  # half the span: the tile is no smaller than the stereo row's
    mats = preset("mono")
    full, lengths = mixed.export(mats, 1, "float32", "planar", rate=fout)
    N = lengths[i]
    assert N > tile.value + 40, "the row crosses the planner's tile"
    start = tile.value - 37
    starts = [start if k == i else 0 for k in range(len(mixed.datas))]
    T = 101  # the window straddles the edge of the full export's first tile
    got, v = mixed.export(mats, 1, "float32", "planar", T=T, starts=starts, rate=fout)
    assert v[i] == T
    np.testing.assert_array_equal(got[i], full[i][:, start:start + T])


def test_resampled_upmix_of_mono(mixed):
    """A mono stream to C = 2 with weights (1, 1): both planes are the unmixed mono resample's bits."""
    i = mixed.i("mono16_22050")
    got, _ = mixed.export({1: np.ones((2, 1), dtype=np.float32)}, 2, "float32", "interleaved", rate=16000)
    unmixed, _ = mixed.plain(2, "float32", "interleaved", rate=16000)
    assert unmixed[i][0].any()
    np.testing.assert_array_equal(got[i][0], unmixed[i][0])
    np.testing.assert_array_equal(got[i][1], unmixed[i][0])


# ---- 8. arguments ---------------------------------------------------------------------------
def test_arguments(mixed):
    """Each rejected call returns 14 and leaves the NaN-prefilled destination untouched."""
    B = len(mixed.datas)
    dst = torch.full((B * 9 * 64 * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    m, ok = mixed.batch, {2: np.asarray([[0.5, 0.5]] * 9, dtype=np.float32)}

    def call(mats, dtype="float32", C=1, batch=m, **kw):
        return [c_mix(batch, mats, dtype, "planar", C, 64, dst.data_ptr(), dst.numel(), rate=r, **kw)[0]
                for r in (None, 16000)]

    def with_coef(v, n=2):
        a = np.full((1, n), 0.5, dtype=np.float32)
        a[0, n - 1] = v
        return {n: a}

    assert call(ok, size=64) == [14, 14]
    assert call(ok, reserved=1) == [14, 14]
    assert call(ok, dtype="int32") == [14, 14]
    assert call(ok, C=9) == [14, 14]
    assert call(with_coef(np.nan)) == [14, 14]
    assert call(with_coef(np.inf)) == [14, 14]
    assert 7 not in mixed.nch
    assert call(with_coef(2.0 ** -65, n=7)) == [14, 14]
    assert call(with_coef(2.0 ** 65, n=7)) == [14, 14]
    b = zflac_amd.Batch(mixed.datas[:3])
    try:
        assert call(ok, batch=b) == [14, 14]  # before the first run
        b.submit()
        assert call(ok, batch=b) == [14, 14]  # between submit and wait
        b.wait()
    finally:
        b.close()
    torch.cuda.synchronize()
    assert bool((dst == 0xFF).all().item()), "a refused export wrote to the destination"
    # accepted: C = 9 with an all-NULL mix (the i32 dtype too, in the plain call), the range's ends
    assert call(None, C=9) == [0, 0]
    assert c_mix(m, None, "int32", "planar", 9, 64, dst.data_ptr(), dst.numel())[0] == 0
    assert call(with_coef(2.0 ** -64)) == [0, 0]
    assert call(with_coef(-(2.0 ** 64))) == [0, 0]
    assert call(with_coef(-0.0)) == [0, 0]
    torch.cuda.synchronize()


# ---- 9, 10. matrix lifetime, ordering -------------------------------------------------------
def test_matrix_lifetime_and_ordering(gpu_ready):
    """On a caller's stream the host matrix is overwritten right after the call returns: the result
    is still the reference. A mixed export on a side stream, the batch's next run, a second mixed
    export: both tensors are right; the batch is destroyed with an export pending."""
    cfgs = [CONFIGS[k] for k in ("stereo16_44100", "mono16", "ch3_16")]
    datas = [synth.generate(**dict(c, seed=7100 + i)).flac for i, c in enumerate(cfgs)]
    refs = [oracle.decode(d) for d in datas]
    mats = {2: np.asarray([[0.5, 0.25]], dtype=np.float32), 3: np.asarray([[1.0, -0.5, 0.25]], dtype=np.float32)}
    T = max(r.samples.size // r.channels for r in refs)
    want = np.zeros((3, 1, T), dtype=np.uint32)
    for i, r in enumerate(refs):
        s = np.ascontiguousarray(r.samples)
        row = (mix_ref.mix_exact_bits(s, r.channels, mats[r.channels], "float32") if r.channels in mats
               else ref.round_bits(ref.to_f32(s).astype(np.float32), "float32").reshape(-1, 1))
        want[i, 0, :row.shape[0]] = row[:, 0]
    b = zflac_amd.Batch(datas)
    side = torch.cuda.Stream()
    try:
        b.run()
        outs = []
        for rep in range(2):
            with torch.cuda.stream(side):
                dst = torch.empty((3, 1, T), dtype=torch.float32, device="cuda")
                rc, _, keep = c_mix(b, mats, "float32", "planar", 1, T, dst.data_ptr(), dst.numel() * 4,
                                    stream=side.cuda_stream)
                for a in keep:
                    a.fill(np.nan)  # the library has read them
                assert rc == 0
            outs.append(dst)
            b.run()  # waits for nothing on the host; the run's streams wait for the export
            for i, r in enumerate(refs):
                assert np.array_equal(b.read(i).samples.values, r.samples), i
        side.synchronize()
        for dst in outs:
            np.testing.assert_array_equal(bits_of(dst, "float32"), want)
        with torch.cuda.stream(side):
            last, _ = tensor.export(b, frames=T, channels=1, mix=mats, stream=side, sample_rate=16000)
    finally:
        b.close()  # with the export pending
    side.synchronize()
    assert bool(torch.isfinite(last).all().item())


# ---- 11. the Python layer -------------------------------------------------------------------
def test_python_layer(mixed):
    x, lengths = tensor.export(mixed.batch, sample_rate=16000, mix="mono")
    want_n = [ref.out_frames(n, f, 16000) for n, f in zip(mixed.frames, mixed.rate)]
    assert tuple(x.shape) == (len(mixed.datas), 1, max(want_n)) and lengths.cpu().tolist() == want_n
    full, _ = mixed.export(preset("mono"), 1, "float32", "planar", rate=16000)  # test_resampled checks its values
    np.testing.assert_array_equal(bits_of(x, "float32"), full[:, :, :max(want_n)])
    y, _ = tensor.export(mixed.batch, mix="stereo", layout="interleaved")
    assert tuple(y.shape) == (len(mixed.datas), max(mixed.frames), 2)
    want, _ = mixed.export(preset("stereo"), 2, "float32", "interleaved", T=max(mixed.frames))
    np.testing.assert_array_equal(as_bct(bits_of(y, "float32"), "interleaved"), want)
    z, _ = tensor.export(mixed.batch, channels=1, mix={2: [[0.5, 0.5]], 3: torch.tensor([[0.25, 0.25, 0.5]])},
                         dtype=torch.float16)
    assert z.dtype == torch.float16 and z.shape[1] == 1
    out, _, _ = tensor.decode_to_tensor([mixed.datas[mixed.i("stereo16_44100")], mixed.datas[0]], mix="mono",
                                        sample_rate=16000)
    assert out.shape[:2] == (2, 1)
    with pytest.raises(TypeError):
        tensor.export(mixed.batch, mix="mono", dtype=torch.int32)
    with pytest.raises(ValueError):
        tensor.export(mixed.batch, channels=2, mix={2: [[0.5, 0.5]]})  # not [channels, n]
    with pytest.raises(ValueError):
        tensor.export(mixed.batch, channels=1, mix={9: [[0.5] * 9]})
    with pytest.raises(ValueError):
        tensor.export(mixed.batch, channels=1, mix={0: [[]]})
    with pytest.raises(ValueError):
        tensor.export(mixed.batch, channels=9, mix={2: [[0.5, 0.5]] * 9})
    with pytest.raises(ValueError):
        tensor.export(mixed.batch, mix="quad")
    with pytest.raises(ValueError):
        tensor.export(mixed.batch, mix="mono", channels=2)
    with pytest.raises(ValueError):
        tensor.export(mixed.batch, mix="stereo", channels=1)
