"""CPU tests of zflac_hip_mel_run_ex's boundary: zflac_mel_run_desc as ctypes and as a strict C11
compiler see it (104 bytes, every offset), the names declared, exported and bound, the constants,
the unchanged ABI version, and the refusals that need no device."""
import ctypes
import os
import re
import subprocess

import torch  # noqa: F401  before zflac_amd loads its library (zflac_amd/tensor.py)

from zflac_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["size", "pad", "norm", "reserved", "wave_device", "rows", "wave_frames", "row_stride", "lengths_device",
          "first_frame", "frames", "dst_device", "dst_bytes", "row_max_device", "range", "add", "mul", "reserved2"]
WANT = [104, 0, 4, 5, 6, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 92, 96, 100]
CONSTANTS = {"PAD_ZEROS": 0, "PAD_REFLECT": 1, "NORM_NONE": 0, "NORM_ROW_MAX": 1}


def header():
    with open(os.path.join(ROOT, "include", "zflac_hip.h")) as f:
        return f.read()


def test_names_constants_and_the_unchanged_abi():
    L = _lib.load()
    text = header()
    name = "zflac_hip_mel_run_ex"
    assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", text) and hasattr(L, name)
    assert len(_lib.SIGNATURES[name][1]) == 3 and _lib.SIGNATURES[name][0] is ctypes.c_int
    for n in (name, "zflac_mel_run_desc", r"ZFLAC_PAD_\*", r"ZFLAC_NORM_\*"):
        assert re.search(rf"Added without a bump.*{n}", text, re.S), n
    for n, v in CONSTANTS.items():
        assert re.findall(rf"#define ZFLAC_{n}\s+(\d+)", text) == [str(v)], n
        assert getattr(_lib, n) == v
    assert not re.search(r"#define ZFLAC_MEL_(PAD|NORM)", text)
    assert int(re.search(r"#define ZFLAC_HIP_ABI_VERSION (\d+)", text).group(1)) == 5 and L.zflac_hip_abi_version() == 5
    # the old entry is as it was
    assert len(_lib.SIGNATURES["zflac_hip_mel_run"][1]) == 10 and ctypes.sizeof(_lib.zflac_mel_desc) == 40


def test_desc_layout_matches_header(tmp_path):
    D = _lib.zflac_mel_run_desc
    assert [n for n, _ in D._fields_] == FIELDS
    assert [ctypes.sizeof(D)] + [getattr(D, n).offset for n in FIELDS] == WANT
    offs = ", ".join(f"offsetof(zflac_mel_run_desc, {f})" for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zflac_hip.h"\n'
                   "int main(void) {\n"
                   f"    size_t v[] = {{sizeof(zflac_mel_run_desc), {offs}}};\n"
                   "    for (size_t i = 0; i < sizeof v / sizeof v[0]; i++) printf(\"%zu \", v[i]);\n"
                   "    return ZFLAC_PAD_ZEROS + ZFLAC_NORM_NONE + (ZFLAC_PAD_REFLECT - 1) + (ZFLAC_NORM_ROW_MAX - 1);\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == WANT


def desc(**kw):
    d = _lib.zflac_mel_run_desc(ctypes.sizeof(_lib.zflac_mel_run_desc), 0, 0, 0, 0x1000, 1, 10, 10, None, 0, 1, 0x2000,
                                1 << 20, None, 0.0, 0.0, 0.0, 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_refusals_without_a_device():
    """No plan, no descriptor or a bad descriptor: ZFLAC_E_INVALID_ARGUMENT (14) whether or not a GPU is there."""
    L = _lib.load()
    assert L.zflac_hip_mel_run_ex(None, ctypes.byref(desc()), None) == 14
    assert L.zflac_hip_mel_run_ex(None, None, None) == 14
    for kw in (dict(size=103), dict(pad=2), dict(norm=2), dict(reserved=1), dict(reserved2=1), dict(frames=0),
               dict(pad=_lib.PAD_REFLECT, norm=_lib.NORM_ROW_MAX, row_max_device=0x3000, range=8.0, add=4.0, mul=0.25)):
        assert L.zflac_hip_mel_run_ex(None, ctypes.byref(desc(**kw)), None) == 14, kw
