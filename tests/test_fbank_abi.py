"""CPU tests of the boundary of the framed plans and the CMVN call (zflac_hip_mel_create_framed,
zflac_hip_mel_plan_frames, zflac_hip_mel_cmvn): the header's names, constants and struct layouts in
the library and the binding, the arguments checked before the device, a strict-C11 consumer
(tests/c/fbank_consumer.c), and the Python layer's refusals."""
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

from .test_mel_abi import desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zflac_hip_mel_create_framed", "zflac_hip_mel_plan_frames", "zflac_hip_mel_cmvn")


def frame(nw=400, framing=_lib.FRAMING_SNIP, dc=1, a=0.97, g=32768.0, reserved=0, size=None):
    return _lib.zflac_mel_frame_desc(ctypes.sizeof(_lib.zflac_mel_frame_desc) if size is None else size, nw, framing, dc, a,
                                     g, reserved)


def kaldi_desc(**kw):
    kw.setdefault("n_fft", 512)
    kw.setdefault("center", 0)
    d, keep = desc(**kw)
    return d, keep


def test_header_names_constants_and_the_unchanged_abi():
    L = _lib.load()
    text = open(os.path.join(ROOT, "include", "zflac_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", text) and hasattr(L, name), name
        assert re.search(rf"Added without a bump.*\b{name}\b", text, re.S), name
    for name in ("zflac_mel_frame_desc", "ZFLAC_FRAMING_", "ZFLAC_PAD_MIRROR", "zflac_mel_cmvn_desc", "ZFLAC_CMVN_"):
        assert re.search(rf"Added without a bump.*{name}", text, re.S), name
    consts = {n: int(v) for n, v in re.findall(r"#define ZFLAC_(FRAMING_\w+|CMVN_\w+|PAD_\w+)\s+(\d+)", text)}
    assert consts == {"FRAMING_STFT": 0, "FRAMING_SNIP": 1, "FRAMING_KALDI_CENTER": 2, "CMVN_MEAN": 0, "CMVN_MEAN_VAR": 1,
                      "PAD_ZEROS": 0, "PAD_REFLECT": 1, "PAD_MIRROR": 2}
    assert consts == {n: getattr(_lib, n) for n in consts}
    assert tensor._MEL_FRAMINGS == {"stft": 0, "snip": 1, "kaldi_center": 2}
    assert tensor._MEL_PADS == {"zeros": 0, "reflect": 1, "mirror": 2} and tensor._MEL_CMVN == {"mean": 0, "mean_var": 1}
    assert int(re.search(r"#define ZFLAC_HIP_ABI_VERSION (\d+)", text).group(1)) == 5 and L.zflac_hip_abi_version() == 5
    for word in ("dither", "use_energy", "VTLN", "NeMo"):  # what is out of scope is said in the header
        assert word in text, word


def test_struct_layouts():
    F, C = _lib.zflac_mel_frame_desc, _lib.zflac_mel_cmvn_desc
    assert ctypes.sizeof(F) == 20
    assert [(n, getattr(F, n).offset) for n, _ in F._fields_] == [
        ("size", 0), ("win_length", 4), ("framing", 6), ("remove_dc", 7), ("preemphasis", 8), ("sample_scale", 12),
        ("reserved", 16)]
    assert ctypes.sizeof(C) == 64
    assert [(n, getattr(C, n).offset) for n, _ in C._fields_] == [
        ("size", 0), ("mode", 4), ("ddof", 5), ("reserved", 6), ("feat_device", 8), ("rows", 16), ("frames", 24),
        ("valid_device", 32), ("mean_device", 40), ("std_device", 48), ("eps", 56), ("pad_value", 60)]
    assert ctypes.sizeof(_lib.zflac_mel_desc) == 40 and ctypes.sizeof(_lib.zflac_mel_run_desc) == 104
    text = open(os.path.join(ROOT, "include", "zflac_hip.h")).read()
    assert "sizeof(zflac_mel_frame_desc): 20" in text and "sizeof(zflac_mel_cmvn_desc): 64" in text


def test_arguments_before_the_device():
    L = _lib.load()
    h = ctypes.c_void_p()
    d, keep = kaldi_desc()
    create = L.zflac_hip_mel_create_framed
    for math in (0, 1, 2):
        assert create(ctypes.byref(d), ctypes.byref(frame()), math, -1, ctypes.byref(h)) == 13 and not h.value
        assert create(ctypes.byref(d), ctypes.byref(frame()), math, 1 << 20, ctypes.byref(h)) == 13 and not h.value
    bad_frames = [dict(size=19), dict(nw=0), dict(nw=513), dict(framing=3), dict(dc=2), dict(a=-0.5), dict(a=1.5),
                  dict(a=float("nan")), dict(g=0.0), dict(g=float("inf")), dict(g=2.0 ** 65), dict(g=2.0 ** -65), dict(reserved=1),
                  dict(nw=159)]
    for kw in bad_frames:
        for device in (0, -1):
            assert create(ctypes.byref(d), ctypes.byref(frame(**kw)), 0, device, ctypes.byref(h)) == 14, kw
    assert create(ctypes.byref(d), None, 0, -1, ctypes.byref(h)) == 14
    assert create(None, ctypes.byref(frame()), 0, -1, ctypes.byref(h)) == 14
    assert create(ctypes.byref(d), ctypes.byref(frame()), 0, -1, None) == 14
    assert create(ctypes.byref(d), ctypes.byref(frame()), 3, -1, ctypes.byref(h)) == 14
    centred, keep2 = kaldi_desc(center=1)
    for framing in (_lib.FRAMING_SNIP, _lib.FRAMING_KALDI_CENTER):
        assert create(ctypes.byref(centred), ctypes.byref(frame(framing=framing)), 0, -1, ctypes.byref(h)) == 14
    assert create(ctypes.byref(centred), ctypes.byref(frame(framing=_lib.FRAMING_STFT)), 0, -1, ctypes.byref(h)) == 13
    for kw in (dict(size=39), dict(n_fft=401), dict(reserved=1), dict(floor=0.0), dict(window=False), dict(filters=False)):
        bad, keep3 = kaldi_desc(**kw)
        assert create(ctypes.byref(bad), ctypes.byref(frame(nw=300)), 0, -1, ctypes.byref(h)) == 14, kw
    if zflac_amd.device_count() == 0:
        assert create(ctypes.byref(d), ctypes.byref(frame()), 0, 0, ctypes.byref(h)) == 13 and not h.value
    del keep, keep2


def test_calls_on_no_plan():
    L = _lib.load()
    assert L.zflac_hip_mel_plan_frames(None, 16000) == 0
    c = _lib.zflac_mel_cmvn_desc(ctypes.sizeof(_lib.zflac_mel_cmvn_desc), 1, 0, 0, 0x1000, 1, 1, None, None, None, 1e-5, 0.0)
    assert L.zflac_hip_mel_cmvn(None, ctypes.byref(c), None) == 14


def test_strict_c11_consumer(tmp_path):
    exe = str(tmp_path / "fbank_consumer")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O2", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "fbank_consumer.c"), "-o", exe,
                           "-L", os.path.join(ROOT, "zflac_amd"), "-lzflac_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "zflac_amd")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr + p.stdout
    assert json.loads(p.stdout) == {"good": 13, "bad_frame": 14, "bad_order": 14, "cmvn_null": 14, "frames_null": 0, "abi": 5}


BAD_ARGS = [dict(framing="kaldi"), dict(framing="snip"), dict(framing="kaldi_center", center=True),
            dict(pad="mirror", center=False), dict(pad="mirror", framing="snip", center=False), dict(pad="symmetric"),
            dict(win_length=0), dict(win_length=401), dict(win_length=100, hop=160), dict(preemphasis=-0.1),
            dict(preemphasis=1.01), dict(preemphasis=float("nan")), dict(sample_scale=0.0), dict(sample_scale=float("inf")),
            dict(sample_scale=2.0 ** 65), dict(cmvn="std"), dict(cmvn="mean", cmvn_eps=-1.0), dict(cmvn="mean", cmvn_ddof=2),
            dict(cmvn="mean", cmvn_pad=float("inf")), dict(win_length=300, window=np.ones(400, np.float32)),
            dict(window="hann_window")]


@pytest.mark.parametrize("kw", BAD_ARGS, ids=lambda kw: "-".join(f"{k}={v if not hasattr(v, 'shape') else 'array'}" for k, v in kw.items()))
def test_python_layer_refuses(kw):
    with pytest.raises(ValueError):
        tensor.MelSpectrogram(16000, **kw)


def test_kaldi_fbank_arguments_reach_the_library_or_the_device():
    """Without a GPU a good kaldi_fbank() fails at the device (the arguments passed); with one it
    is a plan. Either way the Python-side derivations are Kaldi's."""
    try:
        m = tensor.MelSpectrogram.kaldi_fbank()
    except zflac_amd.errors.ZflacError as e:  # noqa: PERF203
        assert zflac_amd.device_count() == 0 and "Device" in type(e).__name__ + str(e)
        return
    with m:
        assert (m.n_fft, m.win_length, m.hop, m.n_bins) == (512, 400, 160, 80)
        assert m.framing == "snip" and m.layout == "frames_first" and m.scale == "ln" and m.floor == 2.0 ** -23
        assert m.mel_frames(16000) == 98
