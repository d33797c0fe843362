"""k_hop's header extraction (hop.hip): a lane finds the sync codes of its 64 bytes of a probe
window, moves the 16 bytes from a code on into four registers (two levels of selects over the 20
loaded dwords, then a byte shift), parses them and checks their CRC-8 in a fixed number of steps.

Batches of 8 streams x 4 frames of 64 samples under the hop front. By the model of the hop's first
window (test_hop_front.first_window_offsets) the second frame's header starts at every byte
0..63 of a lane's share over the batches, 61..63 included, where the header runs into the 16 bytes
the lane loads past its own. A further batch plants 0xFFF8 sync codes that are no headers (a
verbatim sample of -8) before the true header in its lane, in the next lane, and both.

There is no accessor for the frame table, so its positions are compared with the scan front's
through what depends on them: every stream certified by the parallel pass under both fronts (the
chain check accepts a table only if every frame ends where the next one begins and the frames add up
to the stream), no stream handed to the sequential planner, and samples equal to the oracle's."""
from __future__ import annotations

import numpy as np
import pytest

import synth

from . import test_hop_front as hf

pytestmark = pytest.mark.gpu

LANE, WINDOW = hf.LANE, hf.WINDOW
BLOCK, FRAMES, PER_BATCH = 64, 4, 8

_COVER: dict = {}


def lane_offset(data: bytes, frames_begin: int, frame_offsets) -> int:
    """Byte of its lane's 64 at which the first hop finds the second frame's header."""
    o = hf.first_window_offsets(frames_begin, frame_offsets, len(data))[0]
    assert 0 <= o < WINDOW, o
    return o % LANE


def covering_streams():
    """64 streams, one per lane offset 0..63 of the second header: Rice-coded mono frames whose first
    frame's size varies with the seed and the noise level, behind 0..15 bytes of padding."""
    if _COVER:
        return _COVER
    for seed in range(400):
        st = hf.gen(BLOCK * FRAMES, 3000 + seed, block_size=BLOCK, **dict(hf.FIXED2, noise_lsb=1.5 * (1 + seed % 24)))
        assert len(st.frame_offsets) == FRAMES
        for k in range(16):
            fb = st.frames_begin + 4 + k
            data_len = len(st.flac) + 4 + k
            o = hf.first_window_offsets(fb, [int(x) + 4 + k for x in st.frame_offsets], data_len)[0]
            if 0 <= o < WINDOW and o % LANE not in _COVER:
                data = hf.padded(st, k)
                assert lane_offset(data, fb, [int(x) + 4 + k for x in st.frame_offsets]) == o % LANE
                _COVER[o % LANE] = data
        if len(_COVER) == LANE:
            break
    assert sorted(_COVER) == list(range(LANE)), sorted(set(range(LANE)) - set(_COVER))
    return _COVER


@pytest.mark.parametrize("batch", range(LANE // PER_BATCH))
def test_header_at_every_lane_offset(gpu_ready, batch):
    """Offsets batch, batch + 8, ..: each batch holds headers early and late in a lane; the last
    three batches hold 61, 62 and 63."""
    cover = covering_streams()
    data = [cover[o] for o in range(batch, LANE, LANE // PER_BATCH)]
    assert len(data) == PER_BATCH
    for d in data:
        assert hf.ref(d).error == "OK"
    hop = hf.check(data, [(hf.HOP, hf.HOP)])
    assert hop[0][2] == 0  # every stream certified by the parallel pass: the table is the true chain


def verbatim_with_syncs(seed: int, pad: int, where):
    """A verbatim mono stream (4 frames of 64 samples) behind `pad` bytes of padding, with the 16-bit
    sample -8 (bytes FF F8: a sync code, no header) wherever `where(position relative to the second
    header's lane start)` holds for a sample of frames 0 and 1. Returns (bytes, planted positions
    relative to that lane's start, the header's offset in its lane)."""
    rng = np.random.default_rng(seed)
    pcm = rng.integers(-20000, 20000, BLOCK * FRAMES).astype(np.int32)
    pcm[(pcm & 0xFF00) == 0xFF00] = 1234  # no sample begins with FF: no other sync code in the samples
    pcm[(pcm & 0xFF) == 0xFF] = 4321      # ... nor ends with it (FF then F8 / F9 across two samples)
    st = synth.generate(pcm=pcm, block_size=BLOCK, **hf.VERBATIM)
    shift = 4 + pad
    fo = [int(x) + shift for x in st.frame_offsets]
    fb = st.frames_begin + shift
    o = hf.first_window_offsets(fb, fo, len(st.flac) + shift)[0]
    lane0 = fo[1] - o % LANE  # the header's lane starts here (file offset)
    planted = []
    for f in (0, 1):
        first = synth.header_crc8_index(st.flac, int(st.frame_offsets[f])) + 2 + shift  # sample 0 of frame f
        for i in range(BLOCK):
            if where(first + 2 * i - lane0):
                pcm[f * BLOCK + i] = -8
                planted.append(first + 2 * i - lane0)
    st = synth.generate(pcm=pcm, block_size=BLOCK, **hf.VERBATIM)
    data = hf.padded(st, pad)
    assert [int(x) + shift for x in st.frame_offsets] == fo
    for p in planted:
        assert data[lane0 + p:lane0 + p + 2] == b"\xff\xf8"
    return data, planted, o % LANE


def test_false_syncs_beside_the_header(gpu_ready):
    """Sync codes that are no headers: one and two before the true header in its lane (the true one
    is the lane's second and third candidate), one in the next lane, and on both sides."""
    cases = [
        lambda p, o: o - 5 <= p < o - 3,                       # one: the sample before the frame's CRC-16
        lambda p, o: 0 <= p < 2,                               # one, at the lane's first bytes
        lambda p, o: 0 <= p < 2 or o - 5 <= p < o - 3,         # two before the true header
        lambda p, o: LANE <= p < LANE + 2,                     # one in the next lane
        lambda p, o: LANE + 30 <= p < LANE + 32,
        lambda p, o: (0 <= p < 2) or (LANE <= p < LANE + 2),   # both sides
        lambda p, o: 0 <= p < o - 3 and p % 8 < 2,             # every 8 bytes up to the header
        lambda p, o: False,                                    # none (control)
    ]
    data, seen, offs = [], [], []
    for i, fn in enumerate(cases):
        for pad in range(16):  # a padding that puts the header well into its lane
            _, _, o = verbatim_with_syncs(500 + i, pad, lambda p: False)
            if o >= 24:
                break
        assert o >= 24, o
        d, planted, o2 = verbatim_with_syncs(500 + i, pad, lambda p, o=o, fn=fn: fn(p, o))
        assert o2 == o
        data.append(d)
        seen.append(planted)
        offs.append(o)
        assert hf.ref(d).error == "OK"
    assert [len(p) for p in seen[:4]] == [1, 1, 2, 1] and len(seen[5]) == 2 and len(seen[6]) >= 3 and not seen[7], seen
    assert all(p < offs[2] for p in seen[2]) and all(p >= LANE for p in seen[3])
    hop = hf.check(data, [(hf.HOP, hf.HOP)])
    assert hop[0][2] == 0
