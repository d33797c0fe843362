"""CPU tests of the boundary of the split-bf16 feature plans (zflac_hip_mel_create_ex,
zflac_hip_mel_math): the header's names and constants in the library and the binding, the math
argument checked behind the descriptor and before the device, and the Python layer's refusal."""
import ctypes
import os
import re

import torch  # noqa: F401  before zflac_amd loads its library (zflac_amd/tensor.py)

import pytest

import zflac_amd
from zflac_amd import _lib, tensor

from .test_mel_abi import desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zflac_hip_mel_create_ex", "zflac_hip_mel_math")
MATHS = {"F32": 0, "BF16X6": 1, "BF16X3": 2}


def test_header_names_constants_and_the_unchanged_abi():
    L = _lib.load()
    text = open(os.path.join(ROOT, "include", "zflac_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", text) and hasattr(L, name), name
        assert re.search(rf"Added without a bump.*\b{name}\b", text, re.S), name
    assert _lib.SIGNATURES["zflac_hip_mel_create_ex"][1][1] is ctypes.c_uint32 and len(_lib.SIGNATURES["zflac_hip_mel_create_ex"][1]) == 4
    hdr = {n: int(v) for n, v in re.findall(r"#define ZFLAC_MEL_MATH_(\w+)\s+UINT32_C\((\d+)\)", text)}
    assert hdr == MATHS
    assert hdr == {n: getattr(_lib, "MEL_MATH_" + n) for n in hdr}
    assert tensor._MEL_MATHS == {"f32": 0, "bf16x6": 1, "bf16x3": 2}
    assert int(re.search(r"#define ZFLAC_HIP_ABI_VERSION (\d+)", text).group(1)) == 5 and L.zflac_hip_abi_version() == 5
    assert ctypes.sizeof(_lib.zflac_mel_desc) == 40  # the descriptor did not grow: the choice is an argument


def test_math_is_checked_behind_the_descriptor_and_before_the_device():
    L = _lib.load()
    h = ctypes.c_void_p()
    d, keep = desc()
    for math in (3, 4, 255, 0x80000000, 0xFFFFFFFF):
        assert L.zflac_hip_mel_create_ex(ctypes.byref(d), math, 0, ctypes.byref(h)) == 14, math
        assert L.zflac_hip_mel_create_ex(ctypes.byref(d), math, -1, ctypes.byref(h)) == 14, math  # not the device's answer
    for math in MATHS.values():
        assert L.zflac_hip_mel_create_ex(ctypes.byref(d), math, -1, ctypes.byref(h)) == 13 and not h.value
        assert L.zflac_hip_mel_create_ex(ctypes.byref(d), math, 1 << 20, ctypes.byref(h)) == 13 and not h.value
        assert L.zflac_hip_mel_create_ex(None, math, 0, ctypes.byref(h)) == 14
        assert L.zflac_hip_mel_create_ex(ctypes.byref(d), math, 0, None) == 14
        for kw in (dict(size=39), dict(n_fft=401), dict(reserved=1), dict(floor=0.0), dict(window=False), dict(filters=False)):
            bad, keep2 = desc(**kw)
            assert L.zflac_hip_mel_create_ex(ctypes.byref(bad), math, 0, ctypes.byref(h)) == 14, (math, kw)
    if zflac_amd.device_count() == 0:
        for math in MATHS.values():
            assert L.zflac_hip_mel_create_ex(ctypes.byref(d), math, 0, ctypes.byref(h)) == 13, math
            assert not h.value
    del keep


def test_math_of_no_plan():
    L = _lib.load()
    assert L.zflac_hip_mel_math(None) == -14


def test_python_layer_refuses_an_unknown_math():
    for bad in ("nope", "BF16X6", "", None, 1):
        with pytest.raises(ValueError):
            tensor.MelSpectrogram(16000, math=bad)
        with pytest.raises(ValueError):
            tensor.MelSpectrogram.whisper(math=bad)
