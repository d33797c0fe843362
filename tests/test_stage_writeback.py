"""The staged PCM write-back of the 16-bit decode kernels (Stage::store / store_rsrc, decode/pcm_stage.h):
a chunk's 32 samples per frame go back to memory as whole rows at the next chunk start, through a
buffer resource over the class's output (the default) or through the pointer (ZFLAC_STAGE_WB=ptr).
A row of a frame that must not be written (an error frame, a redone chunk, a frame on the generic
path) is masked; its neighbours in the same store instruction are written.

Every case runs under both forms, stereo mid/side and mono, twice per batch: a store that strayed
shows up in the neighbouring stream, one that was wrongly dropped leaves what the run before (or
the allocation) put there and fails the comparison or the STREAMINFO MD5."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
import synth
import zflac_amd
from zflac_amd import errors

pytestmark = pytest.mark.gpu

# one Rice partition per frame, so that every whole 32-sample chunk takes the fast (staged) path
LAYOUTS = {
    "stereo_ms": dict(channels=2, bps=16, stereo_mode=10, predictor=synth.FG_LPC, order=8, precision=12, max_shift=12,
                      partition_order=0),
    "mono": dict(channels=1, bps=16, predictor=synth.FG_FIXED, order=2, partition_order=0, rice_k=4, noise_lsb=4.5,
                 tone_amp=0.05),
}
N_STREAMS, N_FRAMES = 40, 3  # 120 frames: 3.75 waves of 32 stereo frames, 1.875 waves of 64 mono frames

_REF: dict = {}
_BATCHES: dict = {}


def ref(data: bytes):
    if data not in _REF:
        _REF[data] = oracle.decode(data)
    return _REF[data]


def streams(layout: str, block: int, seed0: int, n=N_STREAMS, extra=0):
    return [s for s in synth.generate_many([dict(LAYOUTS[layout], block_size=block, n_samples=block * N_FRAMES + extra,
                                                 seed=seed0 + i) for i in range(n)])]


def batches(layout: str) -> dict:
    """name -> (streams' bytes, index of the error stream or None)"""
    if layout in _BATCHES:
        return _BATCHES[layout]
    seed = 7000 if layout == "mono" else 8000
    b64 = streams(layout, 64, seed)
    out = {
        # A: two whole chunks per frame; three whole chunks; two whole chunks and a partial one,
        # which goes the generic path while its frame's first chunks are still staged
        "block64": ([s.flac for s in b64], None),
        "block96": ([s.flac for s in streams(layout, 96, seed + 100)], None),
        "block80": ([s.flac for s in streams(layout, 80, seed + 200)], None),
    }
    # B: stream 17's second frame with a broken subframe header (its padding bit set): its rows
    # are masked beside its neighbours' live ones; stream 5 ends in a short last frame
    bad = b64[17]
    at = synth.header_crc8_index(bad.flac, int(bad.frame_offsets[1])) + 1
    data = [s.flac for s in b64]
    data[17] = bad.flac[:at] + bytes([bad.flac[at] | 0x80]) + bad.flac[at + 1:]
    data[5] = streams(layout, 64, seed + 300, n=1, extra=-24)[0].flac  # 64 + 64 + 40 samples
    out["masked_rows"] = (data, 17)
    # C: a block size that is no multiple of 8 in the same launch: its frames are not 16-byte
    # aligned in the output, so they never stage (per-sample stores) beside the staged streams
    out["unstaged_beside"] = ([s.flac for s in b64] + [streams(layout, 100, seed + 400, n=1)[0].flac], None)
    _BATCHES[layout] = out
    return out


@pytest.mark.parametrize("form", ["rsrc", "ptr"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("case", ["block64", "block96", "block80", "masked_rows", "unstaged_beside"])
def test_staged_writeback(gpu_ready, monkeypatch, case, layout, form):
    if form == "ptr":
        monkeypatch.setenv("ZFLAC_STAGE_WB", "ptr")
    else:
        monkeypatch.delenv("ZFLAC_STAGE_WB", raising=False)
    data, bad = batches(layout)[case]
    for i, d in enumerate(data):
        assert (ref(d).error != "OK") == (i == bad), (i, ref(d).error)
    b = zflac_amd.Batch(data)
    try:
        for run in range(2):
            b.run()
            for i, d in enumerate(data):
                r = ref(d)
                rc, _ = b.info(i)
                assert ("OK" if rc == 0 else errors.NAMES.get(rc, f"E{rc}")) == r.error, (run, i)
                if i == bad:
                    continue
                got = b.read(i, verify_md5=True)  # raises on a STREAMINFO MD5 mismatch
                np.testing.assert_array_equal(got.samples.values, r.samples, err_msg=f"run {run} stream {i}")
    finally:
        b.close()
