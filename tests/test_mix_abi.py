"""CPU tests of the mixed exports' boundary: null arguments, zflac_mix_desc's layout as ctypes,
the header's text and a strict C11 compiler see it, the unchanged ABI beside it, and the "mono"
and "stereo" presets of zflac_amd.tensor."""
import ctypes
import os
import re
import subprocess

import torch  # noqa: F401  before zflac_amd loads its library (zflac_amd/tensor.py)

import numpy as np
import pytest

from zflac_amd import _lib, tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["size", "reserved", "matrix"]
NAMES = ("zflac_hip_batch_export_mixed", "zflac_hip_batch_export_resampled_mixed")


def test_null_arguments():
    L = _lib.load()
    e = _lib.zflac_export_desc(ctypes.sizeof(_lib.zflac_export_desc), _lib.EXPORT_F32, _lib.LAYOUT_PLANAR, 1, 1, None)
    r = _lib.zflac_resample_desc(ctypes.sizeof(_lib.zflac_resample_desc), _lib.EXPORT_F32, _lib.LAYOUT_PLANAR, 1, 1, None,
                                 16000, 16, 0, 0.85, 8.555504641634386)
    mix = _lib.zflac_mix_desc(ctypes.sizeof(_lib.zflac_mix_desc), 0)
    for fn, d in ((L.zflac_hip_batch_export_mixed, e), (L.zflac_hip_batch_export_resampled_mixed, r)):
        assert fn(None, ctypes.byref(d), ctypes.byref(mix), None, 0, None, None) == 14
        assert fn(None, ctypes.byref(d), None, None, 0, None, None) == 14
        assert fn(None, None, ctypes.byref(mix), None, 0, None, None) == 14
        assert fn(None, None, None, None, 0, None, None) == 14


def test_mix_desc_layout_matches_header():
    """72 bytes on LP64: size u32 @0, reserved u32 @4, matrix: eight pointers @8."""
    D = _lib.zflac_mix_desc
    assert [n for n, _ in D._fields_] == FIELDS
    assert [(n, getattr(D, n).offset, getattr(D, n).size) for n in FIELDS] == [
        ("size", 0, 4), ("reserved", 4, 4), ("matrix", 8, 64)]
    assert ctypes.sizeof(D) == 72 and _lib.MIX_MAX_CHANNELS == 8
    text = open(os.path.join(ROOT, "include", "zflac_hip.h")).read()
    body = re.search(r"typedef struct zflac_mix_desc \{(.*?)\} zflac_mix_desc;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()) for decl in body.split(";") if decl.strip()]
    assert members == ["size", "reserved", "*matrix[8]"]
    assert int(re.search(r"#define ZFLAC_MIX_MAX_CHANNELS (\d+)", text).group(1)) == 8
    # the ABI beside it is where it was
    assert int(re.search(r"#define ZFLAC_HIP_ABI_VERSION (\d+)", text).group(1)) == 5
    assert ctypes.sizeof(_lib.zflac_export_desc) == 24 and ctypes.sizeof(_lib.zflac_resample_desc) == 48
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", text), name
        assert len(_lib.SIGNATURES[name][1]) == 7


def test_header_layout_by_the_c_compiler(tmp_path):
    """sizeof / offsetof of the header's structs from a strict C11 compile (-pedantic -Werror: the
    header itself is still C11)."""
    offs = ", ".join(f"offsetof(zflac_mix_desc, {f})" for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zflac_hip.h"\n'
                   "int main(void) {\n"
                   f"    size_t v[] = {{sizeof(zflac_mix_desc), {offs}, sizeof(zflac_export_desc),\n"
                   "                  sizeof(zflac_resample_desc), sizeof(((zflac_mix_desc *)0)->matrix[0])};\n"
                   "    for (size_t i = 0; i < sizeof v / sizeof v[0]; i++) printf(\"%zu \", v[i]);\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    D = _lib.zflac_mix_desc
    assert got == [72, 0, 4, 8, 24, 48, 8]
    assert got[:4] == [ctypes.sizeof(D)] + [getattr(D, n).offset for n in FIELDS]


def test_mono_preset():
    m = tensor.mix_preset("mono")
    assert sorted(m) == [2, 3, 4, 5, 6, 7, 8]  # mono streams have no matrix
    for n, rows in m.items():
        a = np.asarray(rows, dtype=np.float32)
        assert a.shape == (1, n)
        assert np.array_equal(a.view(np.uint32), np.full((1, n), np.float32(1.0 / n)).view(np.uint32)), n


def test_stereo_preset():
    m = tensor.mix_preset("stereo")
    assert sorted(m) == [1, 3, 4, 5, 6, 7, 8]  # stereo streams have no matrix
    a, h = np.float32(np.sqrt(0.5)), np.float32(0.5)
    want = {
        1: ([1], [1]),
        3: ([1, 0, a], [0, 1, a]),                                # L R C
        4: ([1, 0, a, 0], [0, 1, 0, a]),                          # FL FR BL BR
        5: ([1, 0, a, a, 0], [0, 1, a, 0, a]),                    # FL FR FC BL BR
        6: ([1, 0, a, 0, a, 0], [0, 1, a, 0, 0, a]),              # FL FR FC LFE BL BR: LFE dropped
        7: ([1, 0, a, 0, h, a, 0], [0, 1, a, 0, h, 0, a]),        # FL FR FC LFE BC SL SR
        8: ([1, 0, a, 0, a, 0, a, 0], [0, 1, a, 0, 0, a, 0, a]),  # FL FR FC LFE BL BR SL SR
    }
    for n, rows in m.items():
        got = np.asarray(rows, dtype=np.float32)
        assert got.shape == (2, n)
        assert np.array_equal(got.view(np.uint32), np.asarray(want[n], dtype=np.float32).view(np.uint32)), n
    for n in (6, 7, 8):  # LFE is source channel 3
        assert not np.asarray(m[n], dtype=np.float32)[:, 3].any()
    assert float(np.asarray(m[8], dtype=np.float32)[0].sum()) > 1.0  # no normalisation


def test_unknown_preset():
    with pytest.raises(ValueError):
        tensor.mix_preset("quad")
