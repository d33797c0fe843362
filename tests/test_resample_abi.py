"""CPU tests of the resampled export's boundary: null arguments, the descriptor's layout as
ctypes, the header's text and a strict C11 compiler see it, and the header still being C11."""
import ctypes
import os
import re
import subprocess

from zflac_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["size", "dtype", "layout", "channels", "frames", "starts", "sample_rate", "zeros", "reserved", "rolloff",
          "beta"]


def _desc(**kw):
    base = dict(size=ctypes.sizeof(_lib.zflac_resample_desc), dtype=_lib.EXPORT_F32, layout=_lib.LAYOUT_PLANAR,
                channels=1, frames=1, starts=None, sample_rate=16000, zeros=16, reserved=0, rolloff=0.85,
                beta=8.555504641634386)
    base.update(kw)
    return _lib.zflac_resample_desc(*[base[f] for f in FIELDS])


def test_null_arguments():
    L = _lib.load()
    d = _desc()
    built, held = ctypes.c_uint64(), ctypes.c_uint64()
    assert L.zflac_hip_batch_export_resampled(None, ctypes.byref(d), None, 0, None, None) == 14
    assert L.zflac_hip_batch_export_resampled(None, None, None, 0, None, None) == 14
    assert L.zflac_hip_batch_resample_tables(None, ctypes.byref(built), ctypes.byref(held)) == 14
    assert L.zflac_hip_batch_resample_tables(None, None, None) == 14


def test_resample_desc_layout_matches_header():
    """48 bytes on LP64: size u32 @0, dtype u8 @4, layout u8 @5, channels u16 @6, frames u64 @8,
    starts ptr @16, sample_rate u32 @24, zeros u16 @28, reserved u16 @30, rolloff f64 @32,
    beta f64 @40. The first 24 bytes are zflac_export_desc."""
    D = _lib.zflac_resample_desc
    assert [n for n, _ in D._fields_] == FIELDS
    assert [(n, getattr(D, n).offset, getattr(D, n).size) for n in FIELDS] == [
        ("size", 0, 4), ("dtype", 4, 1), ("layout", 5, 1), ("channels", 6, 2), ("frames", 8, 8), ("starts", 16, 8),
        ("sample_rate", 24, 4), ("zeros", 28, 2), ("reserved", 30, 2), ("rolloff", 32, 8), ("beta", 40, 8)]
    assert ctypes.sizeof(D) == 48
    E = _lib.zflac_export_desc
    assert [(n, getattr(D, n).offset) for n, _ in E._fields_] == [(n, getattr(E, n).offset) for n, _ in E._fields_]
    text = open(os.path.join(ROOT, "include", "zflac_hip.h")).read()
    body = re.search(r"typedef struct zflac_resample_desc \{(.*?)\} zflac_resample_desc;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.strip() for decl in body.split(";") if decl.strip()
               for m in re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()).split(",")]
    assert [m.lstrip("*") for m in members] == FIELDS
    # the plain export's ABI is where it was
    assert ctypes.sizeof(E) == 24
    assert int(re.search(r"#define ZFLAC_HIP_ABI_VERSION (\d+)", text).group(1)) == 5
    for name in ("zflac_hip_batch_export_resampled", "zflac_hip_resampled_frames", "zflac_hip_batch_resample_tables"):
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", text), name


def test_header_layout_by_the_c_compiler(tmp_path):
    """sizeof / offsetof of the header's struct from a strict C11 compile (-pedantic -Werror:
    the header itself is still C11)."""
    offs = ", ".join(f"offsetof(zflac_resample_desc, {f})" for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zflac_hip.h"\n'
                   "int main(void) {\n"
                   f"    size_t v[] = {{sizeof(zflac_resample_desc), {offs}}};\n"
                   "    for (size_t i = 0; i < sizeof v / sizeof v[0]; i++) printf(\"%zu \", v[i]);\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    D = _lib.zflac_resample_desc
    assert got == [48] + [getattr(D, n).offset for n in FIELDS]
    assert got == [ctypes.sizeof(D)] + [getattr(D, n).offset for n in FIELDS]
