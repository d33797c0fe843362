"""CPU tests of the feature calls' boundary (zflac_hip_mel_*): the header's names in the library
and the binding, zflac_mel_desc as ctypes and as a strict C11 compiler see it, the argument checks
that need no device, and zflac_amd.tensor.mel_filters against the formulas written here."""
import ctypes
import os
import re
import subprocess

import torch  # noqa: F401  before zflac_amd loads its library (zflac_amd/tensor.py)

import numpy as np
import pytest

import zflac_amd
from zflac_amd import _lib, tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zflac_hip_mel_create", "zflac_hip_mel_run", "zflac_hip_mel_frames", "zflac_hip_mel_destroy")
FIELDS = ["size", "dtype", "layout", "scale", "center", "n_fft", "hop", "n_bins", "reserved", "floor", "window", "filters"]


def desc(n_fft=400, hop=160, n_bins=80, dtype=_lib.EXPORT_F32, layout=0, scale=_lib.MEL_LOG10, center=1, floor=1e-10,
         reserved=0, size=None, window=True, filters=True):
    w = np.hanning(n_fft + 1)[:-1].astype(np.float32) if n_fft else np.zeros(1, np.float32)
    f = np.ones((max(n_bins, 1), n_fft // 2 + 1), np.float32)
    d = _lib.zflac_mel_desc(ctypes.sizeof(_lib.zflac_mel_desc) if size is None else size, dtype, layout, scale, center,
                            n_fft, hop, n_bins, reserved, floor,
                            w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if window else None,
                            f.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if filters else None)
    return d, (w, f)


def test_header_names_and_the_unchanged_abi():
    L = _lib.load()
    text = open(os.path.join(ROOT, "include", "zflac_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", text) and hasattr(L, name), name
        assert re.search(rf"Added without a bump.*\b{name}\b", text, re.S), name
    assert len(_lib.SIGNATURES["zflac_hip_mel_run"][1]) == 10 and len(_lib.SIGNATURES["zflac_hip_mel_create"][1]) == 3
    hdr = {n: int(v) for n, v in re.findall(r"#define ZFLAC_MEL_(\w+)\s+(\d+)", text)}
    assert hdr == {"POWER": 0, "LOG10": 1, "LN": 2, "BINS_FIRST": 0, "FRAMES_FIRST": 1}
    assert hdr == {n: getattr(_lib, "MEL_" + n) for n in hdr}
    assert "no reflect" in text.lower()
    assert int(re.search(r"#define ZFLAC_HIP_ABI_VERSION (\d+)", text).group(1)) == 5 and L.zflac_hip_abi_version() == 5


def test_desc_layout_matches_header(tmp_path):
    D = _lib.zflac_mel_desc
    assert [n for n, _ in D._fields_] == FIELDS
    want = [40, 0, 4, 5, 6, 7, 8, 10, 12, 14, 16, 24, 32]
    assert [ctypes.sizeof(D)] + [getattr(D, n).offset for n in FIELDS] == want
    offs = ", ".join(f"offsetof(zflac_mel_desc, {f})" for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zflac_hip.h"\n'
                   "int main(void) {\n"
                   f"    size_t v[] = {{sizeof(zflac_mel_desc), {offs}}};\n"
                   "    for (size_t i = 0; i < sizeof v / sizeof v[0]; i++) printf(\"%zu \", v[i]);\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_arguments_are_checked_before_the_device():
    """A bad descriptor is InvalidArgument (14) whether or not a GPU is there; without one a good
    descriptor is DeviceError (13)."""
    L = _lib.load()
    h = ctypes.c_void_p()
    bad = [dict(size=39), dict(dtype=_lib.EXPORT_I32), dict(layout=2), dict(scale=3), dict(center=2), dict(n_fft=401),
           dict(n_fft=2050), dict(n_fft=0), dict(hop=0), dict(hop=401), dict(n_bins=0), dict(n_bins=257), dict(reserved=1),
           dict(floor=0.0), dict(floor=float("inf")), dict(scale=_lib.MEL_POWER, floor=1e-10), dict(window=False),
           dict(filters=False)]
    for kw in bad:
        d, keep = desc(**kw)
        assert L.zflac_hip_mel_create(ctypes.byref(d), 0, ctypes.byref(h)) == 14, kw
    d, keep = desc()
    assert L.zflac_hip_mel_create(None, 0, ctypes.byref(h)) == 14
    assert L.zflac_hip_mel_create(ctypes.byref(d), 0, None) == 14
    keep[0][7] = np.nan
    assert L.zflac_hip_mel_create(ctypes.byref(d), 0, ctypes.byref(h)) == 14
    if zflac_amd.device_count() == 0:
        d, keep = desc()
        assert L.zflac_hip_mel_create(ctypes.byref(d), 0, ctypes.byref(h)) == 13
        assert not h.value


def test_run_and_destroy_without_a_plan():
    L = _lib.load()
    assert L.zflac_hip_mel_run(None, 0x1000, 1, 10, 10, 0, 1, 0x2000, 1 << 20, None) == 14
    assert L.zflac_hip_mel_run(None, None, 0, 0, 0, 0, 0, None, 0, None) == 14
    L.zflac_hip_mel_destroy(None)


def test_mel_frames():
    L = _lib.load()
    for n_fft, hop in ((400, 160), (16, 3)):
        for n in (0, 1, n_fft - 1, n_fft, 10 * hop - 1, 10 * hop, 10 * hop + 1):
            assert L.zflac_hip_mel_frames(n, n_fft, hop, 1) == (n // hop + 1 if n else 0)
            assert L.zflac_hip_mel_frames(n, n_fft, hop, 0) == ((n - n_fft) // hop + 1 if n >= n_fft else 0)


def hz_to_mel(f, scale):
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return 3.0 * f / 200.0 if f < 1000.0 else 15.0 + 27.0 * np.log(f / 1000.0) / np.log(6.4)


def mel_to_hz(m, scale):
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return 200.0 * m / 3.0 if m < 15.0 else 1000.0 * np.exp((m - 15.0) * np.log(6.4) / 27.0)


@pytest.mark.parametrize("scale", ["slaney", "htk"])
@pytest.mark.parametrize("norm", ["slaney", None])
@pytest.mark.parametrize("sr,n_fft,n_mels,f_min,f_max", [(16000, 400, 80, 0.0, None), (44100, 1024, 128, 20.0, 16000.0),
                                                         (8000, 64, 10, 100.0, None)])
def test_mel_filters(scale, norm, sr, n_fft, n_mels, f_min, f_max):
    got = tensor.mel_filters(sr, n_fft, n_mels, f_min=f_min, f_max=f_max, mel_scale=scale, norm=norm)
    K = n_fft // 2 + 1
    assert got.dtype == np.float32 and got.shape == (n_mels, K)
    hi = sr / 2.0 if f_max is None else f_max
    lo_m, hi_m = hz_to_mel(f_min, scale), hz_to_mel(hi, scale)
    p = [mel_to_hz(lo_m + (hi_m - lo_m) * i / (n_mels + 1), scale) for i in range(n_mels + 2)]
    want = np.zeros((n_mels, K))
    for m in range(n_mels):
        for k in range(K):
            f = k * sr / n_fft
            v = max(0.0, min((f - p[m]) / (p[m + 1] - p[m]), (p[m + 2] - f) / (p[m + 2] - p[m + 1])))
            want[m, k] = v * (2.0 / (p[m + 2] - p[m]) if norm == "slaney" else 1.0)
    assert np.all(got >= 0)
    assert np.allclose(got, want, rtol=1e-6, atol=1e-9)
    for m in range(n_mels):  # nothing outside the triangle's support
        f = np.arange(K) * sr / n_fft
        assert not got[m][(f <= p[m] - 1e-6) | (f >= p[m + 2] + 1e-6)].any()
    if norm is None:
        assert got.max() <= 1.0
    else:  # unit area: the bins sample the triangle every sr / n_fft Hz
        wide = [m for m in range(n_mels) if p[m + 2] - p[m] > 16 * sr / n_fft]
        for m in wide:
            assert abs(got[m].sum() * sr / n_fft - 1.0) < 0.05, m


def test_mel_filters_peak_and_errors():
    # the Slaney scale is linear below 1 kHz: 15 filters over 0..800 Hz have their peaks every 50 Hz, on the bins
    got = tensor.mel_filters(1600, 64, 15, f_max=800.0, norm=None)
    assert np.allclose(got.max(axis=1), 1.0, atol=1e-6)
    assert np.array_equal(got.argmax(axis=1), 2 * (np.arange(15) + 1))
    w = tensor.mel_filters(16000, 400, 80)
    assert w.shape == (80, 201) and w[:, 0].max() == 0 and (w.sum(axis=1) > 0).all()
    for kw in (dict(mel_scale="bark"), dict(norm="l2"), dict(f_min=9000.0), dict(f_max=0.0)):
        with pytest.raises(ValueError):
            tensor.mel_filters(16000, 400, 80, **kw)
    with pytest.raises(ValueError):
        tensor.mel_filters(16000, 401, 80)
