"""CPU tests of the dense-export boundary: null arguments, the descriptor's layout, the
numpy reference the GPU tests compare against (pinned by hand vectors), and the
one-HIP-runtime-per-process check of zflac_amd.tensor."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

from zflac_amd import _lib

from .export_ref import convert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_arguments():
    L = _lib.load()
    d = _lib.zflac_export_desc(ctypes.sizeof(_lib.zflac_export_desc), _lib.EXPORT_F32, _lib.LAYOUT_PLANAR, 1, 1, None)
    ms = ctypes.c_double()
    assert L.zflac_hip_batch_export(None, ctypes.byref(d), None, 0, None, None) == 14
    assert L.zflac_hip_batch_export(None, None, None, 0, None, None) == 14
    assert L.zflac_hip_batch_export_ms(None, ctypes.byref(ms)) == 14
    assert L.zflac_hip_batch_export_ms(None, None) == 14


def test_export_desc_layout_matches_header():
    """size u32 @0, dtype u8 @4, layout u8 @5, channels u16 @6, frames u64 @8, starts ptr @16:
    24 bytes on LP64, as a C compiler lays the header's struct out."""
    D = _lib.zflac_export_desc
    assert [(n, getattr(D, n).offset, getattr(D, n).size) for n, _ in D._fields_] == [
        ("size", 0, 4), ("dtype", 4, 1), ("layout", 5, 1), ("channels", 6, 2), ("frames", 8, 8),
        ("starts", 16, ctypes.sizeof(ctypes.c_void_p))]
    assert ctypes.sizeof(D) == 16 + ctypes.sizeof(ctypes.c_void_p)
    # the header declares the same members in the same order, and the constants agree
    text = open(os.path.join(ROOT, "include", "zflac_hip.h")).read()
    body = re.search(r"typedef struct zflac_export_desc \{(.*?)\} zflac_export_desc;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.strip() for decl in body.split(";") if decl.strip()
               for m in re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()).split(",")]
    assert [m.lstrip("*") for m in members] == [n for n, _ in D._fields_]
    for name in ("EXPORT_F32", "EXPORT_F16", "EXPORT_BF16", "EXPORT_I32", "LAYOUT_PLANAR", "LAYOUT_INTERLEAVED"):
        m = re.search(rf"#define ZFLAC_{name} (\d+)", text)
        assert m and int(m.group(1)) == getattr(_lib, name), name


def test_header_layout_by_the_c_compiler(tmp_path):
    """sizeof / offsetof of the header's struct, from a strict C11 compile."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zflac_hip.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(zflac_export_desc),\n'
                   "           offsetof(zflac_export_desc, size), offsetof(zflac_export_desc, dtype),\n"
                   "           offsetof(zflac_export_desc, layout), offsetof(zflac_export_desc, channels),\n"
                   "           offsetof(zflac_export_desc, frames), offsetof(zflac_export_desc, starts));\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    D = _lib.zflac_export_desc
    assert got == [ctypes.sizeof(D)] + [getattr(D, n).offset for n, _ in D._fields_]


def test_reference_pinned_by_hand_vectors():
    s = np.array([1, -32768, 32767], dtype=np.int16)
    assert convert_bits(s, "float16").tolist() == [0x0200, 0xBC00, 0x3C00]
    assert convert_bits(s, "bfloat16").tolist() == [0x3800, 0xBF80, 0x3F80]
    # f32: exact powers of two; 2^-15, -1, 1 - 2^-15
    assert convert_bits(s, "float32").tolist() == [0x38000000, 0xBF800000, 0x3F7FFE00]
    assert convert_bits(s, "int32").tolist() == [1, 0xFFFF8000, 32767]
    # 8- and 32-bit containers: 2^-7 and 2^-31; 2^24 + 1 rounds to even in f32
    assert convert_bits(np.array([1, -128], dtype=np.int8), "float32").tolist() == [0x3C000000, 0xBF800000]
    assert convert_bits(np.array([1, (1 << 24) + 1, (1 << 24) + 3], dtype=np.int32), "float32").tolist() == [
        0x30000000, 0x3C000000, 0x3C000002]


def _run(code):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)


def test_library_first_then_torch_is_refused():
    """libzflac_hip.so loaded before torch: two HIP runtimes in the process, and the check
    every export starts with raises the documented error."""
    r = _run("from zflac_amd import _lib\n_lib.load()\nimport zflac_amd.tensor as t\n"
             "try:\n    t.check_single_runtime()\nexcept RuntimeError as e:\n    print('REFUSED:', e)\n"
             "else:\n    print('PASSED', t.hip_runtimes())\n")
    assert r.returncode == 0, r.stderr
    assert "REFUSED: import torch before zflac_amd loads its library" in r.stdout, r.stdout


def test_torch_first_shares_one_runtime():
    r = _run("import torch\nfrom zflac_amd import _lib\n_lib.load()\nimport zflac_amd.tensor as t\n"
             "t.check_single_runtime()\nprint('RUNTIMES', len(t.hip_runtimes()))\n")
    assert r.returncode == 0, r.stderr
    assert "RUNTIMES 1" in r.stdout, r.stdout
