"""The chunk start of the 16-bit decode kernels (decode/run_subframe.h, decode/pcm_stage.h): the
staged rows' lane masks taken on the scalar unit, the chunk offset as the stores' scalar offset,
and the form selectors held between the chunks where their inputs can change.

Every stream here is ONE frame written by tests/craft.py, so a wave's 32 stereo (64 mono) frames
are 32 (64) streams in batch order: a frame in error is a stream of its own whose neighbours can
still be read, and frames of different block sizes share a wave. A case states, per wave, the
form of every chunk ("W" warm-up, "P" pairs, "O" one code per step, "E" escapes, "S" generic
path), whether the wave holds the mid/side selector, and the chunks at which the k-range and escape
selectors are taken again. `held_model` works these out from craft's per-lane chunk model with the
rules of run_subframe.h; the CPU tests hold the statements to it and the streams to the oracle.

The GPU tests run each case under both write-back forms (buffer resource, ZFLAC_STAGE_WB=ptr) and
both walks. The batch's output span is filled with a canary between two runs: afterwards every OK
stream's bytes equal the oracle's and the writer's PCM, both forms left the same bytes, and every
byte outside an OK stream (the rows of frames in error, the gaps) still holds the canary."""
from __future__ import annotations

import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import oracle
import zflac_amd
from zflac_amd import errors

from . import craft
from .craft import Sub
from .rice_edges import code, filler, no_sync

CANARY = 0xA5


@dataclasses.dataclass
class Case:
    name: str
    streams: list            # one-frame Crafted streams, in batch order
    bad: tuple = ()          # streams whose frame is in error
    shifted: tuple = ()      # streams with wasted bits (or a justify shift) in some channel
    forms: tuple = ()        # per wave: the chunks' forms
    ms: tuple = ()           # per wave: the held mid/side selector
    taken: tuple = ()        # per wave: chunks at which the k-range / escape selectors are taken

    @property
    def mono(self):
        return self.streams[0].channels == 1


# ---- the model: craft.simulate_wave's rules with the selectors held ---------------------------
def held_model(case: Case, wave: int) -> dict:
    ch = case.streams[0].channels
    per = 64 // ch
    members = [i for i in range(wave * per, min((wave + 1) * per, len(case.streams))) if i not in case.bad]
    lanes = [(case.streams[i], c) for c in range(ch) for i in members]
    infos = [craft.chunks(cr, 0, c) for cr, c in lanes]
    # taken once per subframe, over the lanes with a subframe
    ms = all((cr.assignment == "ms" or ch == 1) and cr.bps == 16 for cr, _ in lanes) and not any(
        i in case.shifted for i in members)
    stale, k_bad, esc = True, False, False
    cool = fail = 0
    forms, taken = "", []
    for ci in range(max(len(x) for x in infos)):
        base = ci * craft.CHUNK
        row = [inf[ci] for inf in infos if ci < len(inf)]
        for cr, c in lanes:  # a lane reads a partition header at this chunk start
            L = cr.layout[0][c]
            if L.order <= base < L.bs and base in L.pstart[1:-1]:
                stale = True
        if any(not x.fast for x in row):
            forms += "S"
            stale = True
            continue
        if stale:
            k_bad = any(not (2 <= x.k <= craft.PAIR_KMAX) or x.esc for x in row)
            esc = any(x.esc for x in row)
            stale = False
            taken.append(ci)
        pairs = cool == 0 and ci != 0 and not k_bad
        form = "W" if ci == 0 else "E" if esc else "P" if pairs else "O"
        redo = any(x.pair_max > 32 for x in row) if form == "P" else any(not x.esc and x.longest > 32 for x in row)
        if pairs and redo:
            cool = (8 << min(fail, 4)) if ch == 1 else 8
            fail += 1
        elif ch == 1 and pairs:
            fail = 0
        elif cool:
            cool -= 1
        if redo:
            stale = True
            form = form.lower()  # redone on the generic path
        forms += form
    return dict(forms=forms, ms=ms, taken=tuple(taken))


# ---- the streams ------------------------------------------------------------------------------
def _values(rng, n, what, val):
    if what == "k":
        return filler(rng, n, val)
    return rng.integers(-(1 << (val - 1)) + 1, 1 << (val - 1), n)  # escape width val


def _sub(rng, bs, params=(("k", 4),), wasted=0, long_at=None):
    """FIXED order 0 (residual = sample). `long_at`: (sample, quotient) of one long code."""
    porder = len(params).bit_length() - 1
    ps = bs // len(params)
    r = np.concatenate([_values(rng, ps, what, val) for what, val in params])
    if long_at:
        r[long_at[0]] = code(rng, long_at[1], params[long_at[0] // ps][1])
    return Sub(kind="fixed", order=0, porder=porder, params=tuple(params), residuals=r, wasted=wasted)


def _frame(seed, bs, channels=2, assignment="ms", bps=16, special=None):
    """One sync-free one-frame stream; `special`: channel -> _sub keyword arguments."""
    def build(salt):
        rng = np.random.default_rng([seed, salt])
        subs = [_sub(rng, bs, **((special or {}).get(c, {}))) for c in range(channels)]
        return craft.write(channels, bps, bs, [subs], assignment=assignment if channels == 2 else "indep")
    return no_sync(build)


def _break(cr: craft.Crafted) -> craft.Crafted:
    """The frame's first subframe header with its padding bit set: the reader refuses the frame."""
    at = cr.frame_offsets[0] + 4 + 1 + (1 if cr.bs <= 256 else 2) + 1
    return dataclasses.replace(cr, flac=cr.flac[:at] + bytes([cr.flac[at] | 0x80]) + cr.flac[at + 1:])


def _wave(seed, n, bs, special_at=None, special=None, **kw):
    return [_frame(seed + i, bs, special=special if i == special_at else None, **kw) for i in range(n)]


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    K = lambda *ks: tuple(("k", k) for k in ks)  # noqa: E731
    out = []
    # 1. a frame in error in the middle of wave 0's 32 frames and one in its last row; wave 1 whole
    s = _wave(100, 64, 64)
    s[13], s[30] = _break(s[13]), _break(s[30])
    out.append(Case("error_rows", s, bad=(13, 30), forms=("WP", "WP"), ms=(True, True), taken=((0,), (0,))))
    # 2. a wave of 8 frames after a whole one: its rows 1..3 hold no frame
    out.append(Case("short_wave", _wave(200, 40, 96), forms=("WPP", "WPP"), ms=(True, True), taken=((0,), (0,))))
    # 3. one lane's block ends early (64 of 192) and it alone is left/side: the held selector stays
    #    on the generic decorrelation after it has finished; and the reverse
    s = _wave(300, 32, 192)
    s[9] = _frame(399, 64, assignment="ls")
    out.append(Case("short_lane_ls", s, forms=("WPPPPP",), ms=(False,), taken=((0,),)))
    s = _wave(400, 32, 192, assignment="ls")
    s[9] = _frame(499, 64, assignment="ms")
    out.append(Case("short_lane_ms", s, forms=("WPPPPP",), ms=(False,), taken=((0,),)))
    # 4. wasted bits in one lane only; and, a class of its own, 12-bit streams (justify shift 4)
    s = _wave(500, 32, 96, special_at=5, special={0: dict(wasted=2)})
    out.append(Case("wasted_one_lane", s, shifted=(5,), forms=("WPP",), ms=(False,), taken=((0,),)))
    s = _wave(600, 32, 96, bps=12)
    out.append(Case("justify_12bit", s, shifted=tuple(range(32)), forms=("WPP",), ms=(False,), taken=((0,),)))
    # 5. one lane's k leaves the pair range at a partition boundary in mid-subframe (partitions of
    #    two chunks) and comes back two partitions later
    s = _wave(700, 32, 512, special_at=7, special={0: dict(params=K(4, 4, 4, 12, 12, 4, 4, 4))})
    out.append(Case("k_leaves_pairs", s, forms=("WPPPPPOOOOPPPPPP",), ms=(True,), taken=((0, 2, 4, 6, 8, 10, 12, 14),)))
    # 6. an escape partition appears in mid-subframe in one lane
    s = _wave(800, 32, 256, special_at=7, special={0: dict(params=(("k", 4), ("k", 4), ("e", 6), ("k", 4)))})
    out.append(Case("escape_mid", s, forms=("WPPPEEPP",), ms=(True,), taken=((0, 2, 4, 6),)))
    # 7. a 35-bit code in chunk 2 of one lane: the pair chunk is redone, eight chunks of one code
    #    per step follow, then pairs resume
    s = _wave(900, 32, 512, special_at=3, special={0: dict(long_at=(70, 30))})
    out.append(Case("redo_then_pairs", s, forms=("WPpOOOOOOOOPPPPP",), ms=(True,), taken=((0, 3),)))
    # 8. mono: a frame in error in wave 0, six frames in wave 1
    s = _wave(1000, 70, 96, channels=1)
    s[21] = _break(s[21])
    out.append(Case("mono", s, bad=(21,), forms=("WPP", "WPP"), ms=(True, True), taken=((0,), (0,))))
    # 9. partitions of 48 samples in one lane: chunks 1 and 4 hold a boundary and go the generic
    #    path, where k changes; the chunk after each must take the selectors again (k = 12: one
    #    code per step), and chunk 3 starts on a boundary (k = 4 again: pairs)
    s = _wave(1100, 32, 192, special_at=4, special={0: dict(params=K(4, 12, 4, 12))})
    out.append(Case("generic_then_fast", s, forms=("WSOPSO",), ms=(True,), taken=((0, 2, 3, 5),)))
    return tuple(out)


# (named here so that collecting the tests builds no stream)
NAMES = ["error_rows", "short_wave", "short_lane_ls", "short_lane_ms", "wasted_one_lane", "justify_12bit", "k_leaves_pairs",
         "escape_mid", "redo_then_pairs", "mono", "generic_then_fast"]


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def refs(name: str) -> tuple:
    return tuple(oracle.decode(cr.flac) for cr in case(name).streams)


# ---------------------------------------------------------------------------- CPU
def test_case_names():
    assert [c.name for c in cases()] == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_cases_state_their_selectors(name):
    c = case(name)
    per = 64 // c.streams[0].channels
    waves = -(-len(c.streams) // per)
    assert 1 <= waves <= 2 and len(c.forms) == len(c.ms) == len(c.taken) == waves
    for w in range(waves):
        m = held_model(c, w)
        assert (m["forms"], m["ms"], m["taken"]) == (c.forms[w], c.ms[w], c.taken[w]), (w, m)
    assert all(64 <= cr.bs <= 512 and len(cr.layout) == 1 for cr in c.streams)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_decodes_what_the_writer_wrote(name):
    c = case(name)
    for i, (cr, r) in enumerate(zip(c.streams, refs(name))):
        assert (r.error != "OK") == (i in c.bad), (i, r.error)
        assert not craft.sync_frames(cr), i
        if i not in c.bad:
            np.testing.assert_array_equal(r.samples, cr.justified(), err_msg=str(i))


# ---------------------------------------------------------------------------- GPU
def _hip():
    for n in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            h = ctypes.CDLL(n)
            break
        except OSError:
            continue
    else:
        raise RuntimeError("libamdhip64.so not found")
    h.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return h


def _run_form(c: Case, rs, walk, form, monkeypatch):
    """Decode the case twice with a canary between the runs; returns the output span's bytes."""
    if form == "ptr":
        monkeypatch.setenv("ZFLAC_STAGE_WB", "ptr")
    else:
        monkeypatch.delenv("ZFLAC_STAGE_WB", raising=False)
    hip = _hip()
    ok = [i for i in range(len(c.streams)) if i not in c.bad]
    b = zflac_amd.Batch([cr.flac for cr in c.streams], timing=True, device_md5=True, walk=walk)
    try:
        b.run()
        nbytes = {i: b.info(i)[1].samples_bytes for i in ok}
        at = {i: b.device_samples(i) for i in ok}
        assert all(at[i] for i in ok) and [at[i] for i in ok] == sorted(at[i] for i in ok)
        lo, hi = at[ok[0]], at[ok[-1]] + nbytes[ok[-1]]
        assert hi - lo < 1 << 22
        assert hip.hipMemset(lo, CANARY, hi - lo) == 0
        b.run()
        span = np.zeros(hi - lo, np.uint8)
        assert hip.hipMemcpy(span.ctypes.data, lo, hi - lo, 2) == 0  # device to host
        outside = np.ones(hi - lo, bool)
        for i in range(len(c.streams)):
            rc, _ = b.info(i)
            assert ("OK" if rc == 0 else errors.NAMES.get(rc, f"E{rc}")) == rs[i].error, (form, walk, i)
            if i in c.bad:
                continue
            got = b.read(i, verify_md5=True).samples.values
            np.testing.assert_array_equal(got, rs[i].samples, err_msg=f"{form} {walk} stream {i}: oracle")
            np.testing.assert_array_equal(got, c.streams[i].justified(), err_msg=f"{form} {walk} stream {i}: writer")
            assert b.md5(i) == c.streams[i].md5, (form, walk, i)
            a = at[i] - lo
            assert span[a:a + nbytes[i]].tobytes() == got.tobytes(), (form, walk, i)
            outside[a:a + nbytes[i]] = False
        # the rows of the frames in error (whole frames lie between their neighbours) and the gaps
        for i in c.bad:
            prev, nxt = max(j for j in ok if j < i), min(j for j in ok if j > i)
            assert at[nxt] - (at[prev] + nbytes[prev]) >= c.streams[i].bs * c.streams[i].channels * 2, i
        assert (span[outside] == CANARY).all(), (form, walk, np.flatnonzero(outside & (span != CANARY))[:8])
        # (the host looks again at a stream whose frame the kernels refused, and at no other)
        assert b.timings().sequential_streams <= len(c.bad), (form, walk)
        return span.tobytes()
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("walk", ["lane", "wave"])
@pytest.mark.parametrize("name", NAMES)
def test_chunk_start(gpu_ready, monkeypatch, name, walk):
    c, rs = case(name), refs(name)
    spans = [_run_form(c, rs, walk, form, monkeypatch) for form in ("rsrc", "ptr")]
    assert spans[0] == spans[1], "the two write-back forms left different bytes"
