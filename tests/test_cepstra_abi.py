"""CPU tests of the boundary of the cepstra plans (zflac_hip_cepstra_create / _destroy / _features /
_delta_scales / _project / _cmvn / _deltas): the header's names and struct layouts in the library and
the binding, the arguments refused before the device is touched, a strict-C11 consumer
(tests/c/cepstra_consumer.c), and the Python layer's refusals."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import torch  # noqa: F401  before zflac_amd loads its library (zflac_amd/tensor.py)

import pytest

import zflac_amd
from zflac_amd import _lib, tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zflac_hip_cepstra_create", "zflac_hip_cepstra_destroy", "zflac_hip_cepstra_features",
         "zflac_hip_cepstra_delta_scales", "zflac_hip_cepstra_project", "zflac_hip_cepstra_cmvn", "zflac_hip_cepstra_deltas")
E_DEVICE, E_INVALID = 13, 14


def cdesc(i=0, o=0, layout=0, order=2, n_in=23, n_out=13, window=2, reserved=(0, 0, 0), matrix=True, size=None):
    m = np.full((max(n_out, 1), max(n_in, 1)), 0.25, np.float32) if matrix is True else matrix
    d = _lib.zflac_cepstra_desc(ctypes.sizeof(_lib.zflac_cepstra_desc) if size is None else size, i, o, layout, order, n_in,
                                n_out, window, (ctypes.c_uint8 * 3)(*reserved),
                                None if m is None else m.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    return d, m


def test_header_names_and_the_unchanged_abi():
    L = _lib.load()
    text = open(os.path.join(ROOT, "include", "zflac_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", text) and hasattr(L, name), name
        assert re.search(rf"Added without a bump.*\b{name}\b", text, re.S), name
    for name in ("zflac_cepstra_desc", "zflac_cepstra_project_desc", "zflac_cepstra_delta_desc", "zflac_cepstra,"):
        assert re.search(rf"Added without a bump.*{name}", text, re.S), name
    assert int(re.search(r"#define ZFLAC_HIP_ABI_VERSION (\d+)", text).group(1)) == 5 and L.zflac_hip_abi_version() == 5
    for word in ("use_energy", "dither", "splicing", "low-frame-rate", "compute_deltas", "ComputeDeltas"):
        assert word in text, word  # what is out of scope, and what the deltas are and are not, is said in the header
    assert len(_lib.SIGNATURES["zflac_hip_cepstra_create"][1]) == 3 and len(_lib.SIGNATURES["zflac_hip_cepstra_delta_scales"][1]) == 4
    for name in ("zflac_hip_cepstra_project", "zflac_hip_cepstra_cmvn", "zflac_hip_cepstra_deltas"):
        assert len(_lib.SIGNATURES[name][1]) == 3 and _lib.SIGNATURES[name][0] is ctypes.c_int
    assert _lib.SIGNATURES["zflac_hip_cepstra_cmvn"][1][1]._type_ is _lib.zflac_mel_cmvn_desc  # the same descriptor


def test_struct_layouts():
    D, P, Q = _lib.zflac_cepstra_desc, _lib.zflac_cepstra_project_desc, _lib.zflac_cepstra_delta_desc
    assert ctypes.sizeof(D) == 24
    assert [(n, getattr(D, n).offset) for n, _ in D._fields_] == [
        ("size", 0), ("in_dtype", 4), ("out_dtype", 5), ("layout", 6), ("delta_order", 7), ("n_in", 8), ("n_out", 10),
        ("delta_window", 12), ("reserved", 13), ("matrix", 16)]
    assert ctypes.sizeof(P) == 40
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("size", 0), ("reserved", 4), ("src_device", 8), ("dst_device", 16), ("rows", 24), ("frames", 32)]
    assert ctypes.sizeof(Q) == 56
    assert [(n, getattr(Q, n).offset) for n, _ in Q._fields_] == [
        ("size", 0), ("reserved", 4), ("src_device", 8), ("dst_device", 16), ("rows", 24), ("frames", 32),
        ("valid_device", 40), ("pad_value", 48), ("reserved2", 52)]
    assert ctypes.sizeof(_lib.zflac_mel_cmvn_desc) == 64 and ctypes.sizeof(_lib.zflac_mel_desc) == 40
    text = open(os.path.join(ROOT, "include", "zflac_hip.h")).read()
    for s in ("sizeof(zflac_cepstra_desc): 24", "sizeof(zflac_cepstra_project_desc): 40", "sizeof(zflac_cepstra_delta_desc): 56"):
        assert s in text


def test_arguments_before_the_device():
    L = _lib.load()
    h = ctypes.c_void_p()
    create = L.zflac_hip_cepstra_create
    d, keep = cdesc()
    for device in (-1, 1 << 20):  # no such device: the arguments passed
        assert create(ctypes.byref(d), device, ctypes.byref(h)) == E_DEVICE and not h.value
    only, _ = cdesc(n_in=13, n_out=13, matrix=None, i=2, o=2)
    assert create(ctypes.byref(only), -1, ctypes.byref(h)) == E_DEVICE
    nan = np.full((13, 23), 0.25, np.float32)
    nan[12, 22] = np.nan
    bad = [dict(size=23), dict(i=3), dict(o=4), dict(layout=2), dict(order=4), dict(n_in=0), dict(n_in=257), dict(n_out=0),
           dict(n_out=257), dict(window=0), dict(window=6), dict(order=0, window=2), dict(reserved=(0, 0, 1)),
           dict(matrix=None), dict(matrix=None, n_in=13, i=0, o=1), dict(matrix=None, n_in=13, order=0, window=0),
           dict(matrix=nan)]
    for kw in bad:
        for device in (0, -1):
            b, keep2 = cdesc(**kw)
            assert create(ctypes.byref(b), device, ctypes.byref(h)) == E_INVALID and not h.value, kw
    assert create(None, -1, ctypes.byref(h)) == E_INVALID and create(ctypes.byref(d), -1, None) == E_INVALID
    if zflac_amd.device_count() == 0:
        assert create(ctypes.byref(d), 0, ctypes.byref(h)) == E_DEVICE and not h.value
    del keep


def test_calls_on_no_plan():
    """NULL plan: ZFLAC_E_INVALID_ARGUMENT from every run call, with no GPU needed."""
    L = _lib.load()
    r = _lib.zflac_cepstra_project_desc(ctypes.sizeof(_lib.zflac_cepstra_project_desc), 0, 0x1000, 0x2000, 1, 1)
    q = _lib.zflac_cepstra_delta_desc(ctypes.sizeof(_lib.zflac_cepstra_delta_desc), 0, 0x1000, 0x2000, 1, 1, None, 0.0, 0)
    c = _lib.zflac_mel_cmvn_desc(ctypes.sizeof(_lib.zflac_mel_cmvn_desc), 1, 0, 0, 0x1000, 1, 1, None, None, None, 1e-5, 0.0)
    assert L.zflac_hip_cepstra_project(None, ctypes.byref(r), None) == E_INVALID
    assert L.zflac_hip_cepstra_deltas(None, ctypes.byref(q), None) == E_INVALID
    assert L.zflac_hip_cepstra_cmvn(None, ctypes.byref(c), None) == E_INVALID
    assert L.zflac_hip_cepstra_features(None) == 0
    buf = (ctypes.c_float * 8)()
    assert L.zflac_hip_cepstra_delta_scales(None, 1, buf, 8) == -E_INVALID
    L.zflac_hip_cepstra_destroy(None)


def test_strict_c11_consumer(tmp_path):
    exe = str(tmp_path / "cepstra_consumer")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O2", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "cepstra_consumer.c"), "-o", exe,
                           "-L", os.path.join(ROOT, "zflac_amd"), "-lzflac_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "zflac_amd")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr + p.stdout
    assert json.loads(p.stdout) == {"good": 13, "bad_window": 14, "nan_matrix": 14, "deltas_only": 13, "neither": 14,
                                    "project_null": 14, "cmvn_null": 14, "deltas_null": 14, "features_null": 0,
                                    "scales_null": -14, "abi": 5}


BAD_ARGS = [dict(mfcc=0), dict(mfcc=81), dict(mfcc=13, dct_norm="slaney"), dict(mfcc=13, lifter=-1.0),
            dict(mfcc=13, lifter=float("inf")), dict(lifter=22.0), dict(mfcc=np.ones((13, 79), np.float32)),
            dict(mfcc=np.ones((257, 80), np.float32)), dict(mfcc=np.ones(80, np.float32)),
            dict(mfcc=np.full((13, 80), np.nan, np.float32)), dict(mfcc=np.ones((13, 80), np.float32), lifter=22.0),
            dict(deltas=2), dict(deltas=(2,)), dict(deltas=(0, 2)), dict(deltas=(4, 2)), dict(deltas=(2, 0)), dict(deltas=(2, 6)),
            dict(deltas=(1, 2, 3))]


@pytest.mark.parametrize("kw", BAD_ARGS, ids=lambda kw: "-".join(f"{k}={v if not hasattr(v, 'shape') else 'array'}" for k, v in kw.items()))
def test_python_layer_refuses(kw):
    with pytest.raises(ValueError):
        tensor.MelSpectrogram(16000, **kw)


def test_kaldi_mfcc_refusals_and_arguments():
    with pytest.raises(ValueError, match="not provided"):
        tensor.MelSpectrogram.kaldi_mfcc(use_energy=True)
    with pytest.raises(TypeError):
        tensor.MelSpectrogram.kaldi_mfcc(mfcc=20)
    with pytest.raises(ValueError):
        tensor.MelSpectrogram.kaldi_mfcc(num_ceps=24)  # more cepstra than the 23 bins
    try:
        m = tensor.MelSpectrogram.kaldi_mfcc(deltas=(2, 2), dtype=torch.float16)
    except zflac_amd.errors.ZflacError as e:  # noqa: PERF203
        assert zflac_amd.device_count() == 0 and "Device" in type(e).__name__ + str(e)
        return
    with m:
        assert (m.n_bins, m.n_base, m.n_features, m.deltas, m.dtype) == (23, 13, 39, (2, 2), torch.float16)
        assert np.array_equal(m.dct, tensor.dct_matrix(13, 23, lifter=22.0)) and m.layout == "frames_first"
