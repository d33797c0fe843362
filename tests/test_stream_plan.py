"""The host planner (zflac_amd/csrc/stream_plan.cpp: metadata and first-frame parsing) against
the oracle, without a GPU. The planner and the frame-header parser it shares with the kernels
(frame_header.h) are built here with plain g++: that they compile is the check that both are
free of HIP."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle

from . import malformed
from .util import GOLDEN, load_fixture_manifest, load_kats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zflac_amd", "csrc")

# the errors only the host planner decides (zflac_hip_batch_create never asks the GPU)
METADATA_ERRORS = ("InvalidSignature", "InvalidMetadataHeader", "MissingStreaminfo")
# malformed cases whose error plan_stream is expected to find on its own
HOST_CASES = ("bad_signature", "starts_at_frame", "unparsable_start", "reserved_metadata_type", "metadata_type_127",
              "missing_streaminfo", "incorrect_metadata_length", "wrong_channel_count", "reserved_depth_first_frame",
              "no_frames_known_total")


class PlanResult(ctypes.Structure):
    _fields_ = [("host_err", ctypes.c_int), ("no_frames", ctypes.c_int), ("kind", ctypes.c_int),
                ("nch", ctypes.c_int), ("rate", ctypes.c_uint), ("bps", ctypes.c_int)]


@pytest.fixture(scope="module")
def plan():
    srcs = [os.path.join(ROOT, "tests", "c", "plan_probe.cpp"), os.path.join(CSRC, "stream_plan.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("stream_plan.h", "frame_header.h", "common.h")]
    lib = os.path.join(ROOT, "tests", "c", "_build", "libplan_probe.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Werror", "-O2", "-shared", "-fPIC", "-I", CSRC,
                               *srcs, "-o", lib])
    dll = ctypes.CDLL(lib)
    dll.plan_probe.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(PlanResult)]
    dll.plan_probe.restype = None

    def run(data: bytes) -> PlanResult:
        r = PlanResult()
        dll.plan_probe(data, len(data), ctypes.byref(r))
        return r

    return run


def _inputs():
    for name, (data, _) in malformed.cases().items():
        yield "malformed/" + name, data
    for fx in load_fixture_manifest()["fixtures"]:
        with open(os.path.join(GOLDEN, fx["file"]), "rb") as f:
            yield "golden/" + fx["file"], f.read()
    for kat in load_kats():
        yield "kat/" + kat["name"], bytes.fromhex(kat["flac_hex"])


def test_plan_stream_matches_oracle(plan):
    host_errors, compared = [], 0
    for name, data in _inputs():
        p, o = plan(data), oracle.decode(data)
        if p.host_err:  # what the planner rejects, zflac rejects the same way
            assert oracle.ERROR_NAMES[p.host_err] == o.error, name
            host_errors.append(name)
        if o.error in METADATA_ERRORS:
            assert oracle.ERROR_NAMES.get(p.host_err) == o.error, name
        if p.host_err == 0 and o.samples is not None:  # OK or InvalidChecksum
            kind = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}[o.samples.dtype]
            assert p.kind == kind, name
            if p.no_frames:  # zero samples, no first frame to take the rest from
                assert o.samples.size == 0, name
                continue
            assert (p.nch, p.rate, p.bps) == (o.channels, o.sample_rate, o.bits_per_sample), name
            compared += 1
    found = {n[len("malformed/"):] for n in host_errors if n.startswith("malformed/")}
    assert len(found) >= 8 and found >= set(HOST_CASES), sorted(set(HOST_CASES) - found)
    assert compared >= 20, compared
