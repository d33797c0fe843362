"""Streams that sit on the Rice path's exact bit-count edges, built from chosen residuals with
tests/craft.py: pair fit (A), single-code fit (B), redo isolation (C), partition geometry (D),
escapes (E), long zero runs (F), bit rate (G), k_walk_wave's segments and scans (H), and the
rest of what the writer can write (W).

`family(name)` returns the family's cases. A `Case` is a crafted stream, the error the oracle
must report and a `claim`: a function that asserts, through craft's precondition model, that
the stream sits where it says ("wave 3: lane 24 alone spoils chunk 1, with a pair of exactly 33
bits"). A builder module like edges.py and decode_matrix.py: tests/test_rice_edges.py holds the
assertions.

A stream here is made of whole waves: 64 // channels frames each, in batch order, so a
64-frame mono stream is lanes 0..63 of one wave, and the streams of a family never share a
wave. Filler codes have a quotient of at least 1 and a remainder with a zero in every run of
seven bits, so no filler byte is FF; what else could spell a byte-aligned frame sync (raw
escape values, check sums) is found by `craft.sync_positions` and moved off by another salt."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from zflac_amd import _lib

from . import craft
from .craft import Sub

FAMILIES = ("A", "B", "C", "D", "E", "F", "G", "H", "W")


@dataclasses.dataclass
class Case:
    name: str
    cr: craft.Crafted
    error: str = "OK"
    claim: object = None


# ---- residual helpers ---------------------------------------------------------------------------
def unzig(zz):
    zz = np.asarray(zz, dtype=np.int64)
    return np.where(zz & 1, -((zz + 1) >> 1), zz >> 1)


def safe_rem(rng, k: int, shape=None):
    """Random k-bit remainders whose top bit and every seventh bit below it are 0."""
    m = (1 << k) - 1
    for b in range(k - 1, -1, -7):
        m &= ~(1 << b)
    return rng.integers(0, 1 << k, shape) & m if k else np.zeros(shape, np.int64) if shape else 0


def filler(rng, shape, k: int, qmax: int = 2):
    """Residuals whose codes are short: quotient 1..qmax, sync-safe remainder."""
    return unzig((rng.integers(1, qmax + 1, shape) << k) | safe_rem(rng, k, shape))


def code(rng, q: int, k: int, rem=None) -> int:
    """The residual whose code has quotient q (and remainder rem, else a sync-safe one)."""
    return int(unzig((q << k) | (int(safe_rem(rng, k)) if rem is None else rem)))


def mono_frames(R, **kw) -> list:
    return [[Sub(residuals=row, **kw)] for row in R]


def no_sync(build, tries: int = 400):
    """build(salt) -> Crafted, for the first salt whose frames hold no byte-aligned sync pattern."""
    for salt in range(tries):
        out = build(salt)
        cr = out[0] if isinstance(out, tuple) else out
        if not craft.sync_frames(cr):
            return out
    raise AssertionError("no salt gives a sync-free stream")


def write_sync_free(channels: int, bps: int, bs: int, n: int, make, tries: int = 60, **kw):
    """craft.write of frames make(i, salt), i < n: a frame that holds a byte-aligned sync pattern
    is made again with the next salt (a frame's bytes do not depend on the other frames)."""
    salts = [0] * n
    frames = [make(i, 0) for i in range(n)]
    for _ in range(tries):
        cr = craft.write(channels, bps, bs, frames, **kw)
        bad = craft.sync_frames(cr)
        if not bad:
            return cr
        for f in bad:
            salts[f] += 1
            frames[f] = make(f, salts[f])
    raise AssertionError("no salt gives a sync-free stream")


def waves_of(cr) -> int:
    per = 64 // cr.channels
    assert len(cr.layout) % per == 0, "streams are made of whole waves"
    return len(cr.layout) // per


def assert_quiet(cr, sim, except_chunks=()):
    """No chunk of the wave is redone, but the named ones."""
    for ci, rec in enumerate(sim):
        if ci not in except_chunks:
            assert not rec["redo"], (ci, rec)


def assert_one_spoiler(sim, ci: int, lane, form=None):
    rec = sim[ci]
    assert rec["redo"] and [s[0] for s in rec["spoilers"]] == [lane], (ci, lane, rec)
    assert form is None or rec["form"] == form, (ci, rec)


# ---- A: pair fit ----------------------------------------------------------------------------------
def _pair_q(rng, T: int, k: int, q1: int):
    S = T - 2 * (k + 1)
    return code(rng, q1, k), code(rng, S - q1, k)


def _A_fit(k: int):
    """One mono 16-bit wave, block 128: aligned pairs of 31 and 32 bits in chunks 1..3, every
    split of the quotient sum, at moving pair slots. No chunk is redone: every chunk after the
    first decodes in the pair form."""
    combos = [(T, q1) for T in (31, 32) for q1 in range(T - 2 * (k + 1) + 1)]

    def build(salt):
        rng = np.random.default_rng(0xA000 + 16 * k + 4096 * salt)
        R = filler(rng, (64, 128), k, 2)
        where = []
        for i, (T, q1) in enumerate(combos):
            lane, ci, slot = i % 64, 1 + (i // 64 + i) % 3, (5 * i + i // 64) % 16
            a = 32 * ci + 2 * slot
            R[lane, a], R[lane, a + 1] = _pair_q(rng, T, k, q1)
            where.append((lane, ci, slot, T, q1))
        return craft.write(1, 16, 128, mono_frames(R, params=(("k", k),))), where

    cr, where = no_sync(build)

    def claim():
        sim = craft.simulate_wave(cr)
        assert [r["form"] for r in sim] == ["warm", "pair", "pair", "pair"]
        assert_quiet(cr, sim)
        seen = set()
        for lane, ci, slot, T, q1 in where:
            n = cr.layout[lane][0].clen
            a = 32 * ci + 2 * slot
            assert n[a] + n[a + 1] == T and n[a] == q1 + k + 1, (lane, ci, slot, T, q1)
            seen.add((T, q1))
        assert seen == set(combos)
        assert max(x.pair_max for f in range(64) for x in craft.chunks(cr, f, 0)[1:]) == 32
    return Case(f"A_fit_k{k}", cr, claim=claim)


def _A_over(k: int):
    """Mono 16-bit, block 64, one wave per case: exactly one lane holds, in chunk 1, one aligned
    pair that does not fit. Pairs of 33 and of 34 bits in every split; a first code
    that alone has 32 and 33 bits; a first code of 32 zeros (an all-zero peek)."""
    S33, S34 = 33 - 2 * (k + 1), 34 - 2 * (k + 1)
    plan = [("pair33", q1, S33 - q1) for q1 in range(S33 + 1)]
    plan += [("pair34", q1, S34 - q1) for q1 in range(S34 + 1)]
    plan += [("first32", 32 - k - 1, 1), ("first33", 33 - k - 1, 1), ("zero_peek", 32, 1)]

    def build(salt):
        rng = np.random.default_rng(0xA100 + 16 * k + 4096 * salt)
        R = filler(rng, (64 * len(plan), 64), k, 2)
        where = []
        for w, (what, q1, q2) in enumerate(plan):
            lane, slot = (7 * w + 3) % 64, (5 * w + 1) % 16
            a = 32 + 2 * slot
            R[64 * w + lane, a], R[64 * w + lane, a + 1] = code(rng, q1, k), code(rng, q2, k)
            where.append((w, lane, slot, what, q1, q2))
        return craft.write(1, 16, 64, mono_frames(R, params=(("k", k),))), where

    cr, where = no_sync(build)

    def claim():
        assert waves_of(cr) == len(plan)
        for w, lane, slot, what, q1, q2 in where:
            sim = craft.simulate_wave(cr, w)
            assert [r["form"] for r in sim] == ["warm", "pair"]
            assert_quiet(cr, sim, (1,))
            assert_one_spoiler(sim, 1, (64 * w + lane, 0))
            x = craft.chunks(cr, 64 * w + lane, 0)[1]
            total = q1 + q2 + 2 * (k + 1)
            assert (x.pair_at, x.pair_max) == (slot, total) and total > 32, (w, x)
            n = cr.layout[64 * w + lane][0].clen[32 + 2 * slot]
            assert n == q1 + k + 1
            assert {"pair33": total == 33 and x.longest <= 32, "pair34": total == 34 and x.longest <= 32,
                    "first32": n == 32, "first33": n == 33, "zero_peek": x.zero_peeks == 1}[what], (w, what, x)
    return Case(f"A_over_k{k}", cr, claim=claim)


def _A_outside(k: int):
    """k = 1 and k = 10, just outside the decode pair range: pairs of 31..34 bits in a mono 16-bit
    wave that never takes the pair form, so nothing is redone."""
    def build(salt):
        rng = np.random.default_rng(0xA200 + k + 4096 * salt)
        R = filler(rng, (64, 128), k, 2)
        for lane in range(64):
            T = 31 + lane % 4
            S = T - 2 * (k + 1)
            a = 32 * (1 + lane % 3) + 2 * ((3 * lane) % 16)
            R[lane, a], R[lane, a + 1] = code(rng, S // 2, k), code(rng, S - S // 2, k)
        return craft.write(1, 16, 128, mono_frames(R, params=(("k", k),)))

    cr = no_sync(build)

    def claim():
        sim = craft.simulate_wave(cr)
        assert [r["form"] for r in sim] == ["warm", "one", "one", "one"]
        assert_quiet(cr, sim)
        tot = {x.pair_max for f in range(64) for x in craft.chunks(cr, f, 0)[1:]}
        assert {31, 32, 33, 34} <= tot and max(tot) == 34
    return Case(f"A_outside_k{k}", cr, claim=claim)


def _A_walk(bps: int, k: int):
    """Stereo (left/right), k in channel 0: the lane walk (k_walk) pairs codes for every container
    and from k = 1. Chunk 1 holds pairs of 31 and 32 bits, chunk 2 one pair of 33 bits in one
    lane; the decode kernels pair only 16-bit containers with k >= 2."""
    def build(salt):
        rng = np.random.default_rng(0xA300 + bps * 32 + k + 4096 * salt)
        R0, R1 = filler(rng, (32, 128), k, 2), filler(rng, (32, 128), 3, 2)
        for lane in range(32):
            T = 31 + lane % 2
            S = T - 2 * (k + 1)
            q1 = (lane * 3) % (S + 1)
            a = 32 + 2 * ((5 * lane) % 16)
            R0[lane, a], R0[lane, a + 1] = code(rng, q1, k), code(rng, S - q1, k)
        S = 33 - 2 * (k + 1)
        R0[11, 64 + 2 * 6], R0[11, 64 + 2 * 6 + 1] = code(rng, S // 2, k), code(rng, S - S // 2, k)
        fr = [[Sub(residuals=R0[f], params=(("k", k),)), Sub(residuals=R1[f], params=(("k", 3),))] for f in range(32)]
        return craft.write(2, bps, 128, fr)

    cr = no_sync(build)

    def claim():
        sim = craft.simulate_wave(cr, walk=True)
        assert [r["form"] for r in sim] == ["warm", "pair", "pair", "one"]
        assert_quiet(cr, sim, (2,))
        assert_one_spoiler(sim, 2, (11, 0))
        assert craft.chunks(cr, 11, 0)[2].pair_max == 33 and craft.chunks(cr, 11, 0)[2].longest <= 32
        assert {craft.chunks(cr, f, 0)[1].pair_max for f in range(32)} == {31, 32}
        dec = craft.simulate_wave(cr)
        if craft.widths(bps)[0] != 16 or k < 2:
            assert all(r["form"] in ("warm", "one") for r in dec) and not any(r["redo"] for r in dec)
    return Case(f"A_walk_{bps}bit_k{k}", cr, claim=claim)


def family_A():
    out = [_A_fit(k) for k in (2, 5, 9)] + [_A_over(k) for k in (2, 5, 9)] + [_A_outside(k) for k in (1, 10)]
    out += [_A_walk(8, 1), _A_walk(16, 1), _A_walk(16, 2), _A_walk(24, 1), _A_walk(24, 9)]
    return out


# ---- B: single-code fit ---------------------------------------------------------------------------
LENS_FIT, LENS_OVER = (31, 32), (33, 64, 65)


def _fits(bps: int, k: int, n: int) -> bool:
    """Can an order-0 subframe of this depth hold a code of n bits at parameter k?"""
    q = n - k - 1
    return q >= 0 and ((q + 1) << k) <= (1 << bps)


def _B_stream(tag: str, channels: int, bps: int, ks, method: int = 0):
    """Block 128 in two partitions of 64. Wave 0: codes of 31 and 32 bits for every k of `ks`
    in chunk 0 (warm form), chunk 1 and chunks 2 and 3, where the last lane is in an escape
    partition (escape form): nothing is redone. Then one wave per (k, length over 32), its
    chunk moving from wave to wave: exactly one lane holds one code that is longer than the
    peek. Lanes keep their own k (ks[lane % len(ks)]) in every wave."""
    per = 64 // channels
    over = [(k, n) for k in ks for n in LENS_OVER if _fits(bps, k, n)]
    fit = [(k, n) for k in ks for n in LENS_FIT if _fits(bps, k, n)]
    n_waves = 1 + len(over)
    lanes = per * channels
    lane_k = [ks[i % len(ks)] for i in range(lanes)]

    def build(salt):
        rng = np.random.default_rng(0xB000 + bps * 64 + channels * 8 + method + 4096 * salt)
        R = np.zeros((n_waves, lanes, 128), np.int64)
        for i, k in enumerate(lane_k):
            R[:, i, :] = filler(rng, (n_waves, 128), k, max(1, min(2, 31 - k)))
        esc_lane = lanes - 1
        R[:, esc_lane, 64:] = rng.integers(0, 100, (n_waves, 64))
        where_fit, where_over = [], []
        for j, (k, n) in enumerate(fit):
            cands = [i for i in range(lanes - 1) if lane_k[i] == k]
            for ci in range(4):
                lane = cands[(j + ci) % len(cands)]
                at = 32 * ci + (7 * j + 3 * ci) % 32
                R[0, lane, at] = code(rng, n - k - 1, k)
                where_fit.append((lane, ci, at, k, n))
        for w, (k, n) in enumerate(over, start=1):
            cands = [i for i in range(lanes - 1) if lane_k[i] == k]
            lane, ci = cands[(3 * w) % len(cands)], w % 4
            at = 32 * ci + (11 * w) % 32
            R[w, lane, at] = code(rng, n - k - 1, k)
            where_over.append((w, lane, ci, at, k, n))
        frames = []
        for w in range(n_waves):
            for f in range(per):
                subs = []
                for c in range(channels):
                    i = c * per + f
                    params = (("k", lane_k[i]), ("e", 8) if i == esc_lane else ("k", lane_k[i]))
                    subs.append(Sub(residuals=R[w, i], method=method, porder=1, params=params))
                frames.append(subs)
        return craft.write(channels, bps, 128, frames), where_fit, where_over

    cr, where_fit, where_over = no_sync(build)
    forms = ["warm", "one", "esc", "esc"]

    def lane_fc(w, lane):
        return w * per + lane % per, lane // per

    def claim():
        assert waves_of(cr) == n_waves and fit and over
        sim = craft.simulate_wave(cr, 0)
        assert_quiet(cr, sim)
        assert [r["form"] for r in sim] == forms, [r["form"] for r in sim]
        for lane, ci, at, k, n in where_fit:
            f, c = lane_fc(0, lane)
            assert cr.layout[f][c].clen[at] == n and craft.chunks(cr, f, c)[ci].k == k
        assert {(k, n) for _, _, _, k, n in where_fit} == set(fit)
        for w, lane, ci, at, k, n in where_over:
            sim = craft.simulate_wave(cr, w)
            assert_quiet(cr, sim, (ci,))
            assert_one_spoiler(sim, ci, lane_fc(w, lane), forms[ci])
            x = craft.chunks(cr, *lane_fc(w, lane))[ci]
            assert (x.longest, x.longest_at, x.k) == (n, at % 32, k), (w, x)
            assert x.zero_peeks == (1 if n - k - 1 >= 32 else 0)
        if channels == 1 and min(ks) >= 2:
            assert all(x.k >= 2 for f in range(per) for x in craft.chunks(cr, f, 0)[:2])
    return Case(f"B_{tag}", cr, claim=claim)


def family_B():
    return [_B_stream("mono8", 1, 8, (0, 1, 2)),
            _B_stream("mono16", 1, 16, (0, 1, 2, 9, 14)),
            _B_stream("mono16_kge2", 1, 16, (2, 14, 10)),  # every lane k >= 2, no pairs: the mono residual form
            _B_stream("mono32", 1, 32, (0, 1, 2, 9, 14)),
            _B_stream("mono32_rice2", 1, 32, (15, 22, 30), method=1),
            _B_stream("mono24_rice2", 1, 24, (15, 22), method=1),
            _B_stream("stereo16", 2, 16, (2, 9, 14)),
            _B_stream("stereo8", 2, 8, (0, 2)),
            _B_stream("ch3_16", 3, 16, (1, 9)),
            _B_stream("ch3_32", 3, 32, (0, 14))]


# ---- C: redo isolation ----------------------------------------------------------------------------
C_BS = 384
LPC2 = dict(kind="lpc", order=2, coefs=(7, -3), precision=4, shift=2)
FIX2 = dict(kind="fixed", order=2)


def _signal(rng, shape, amp=1000, period=20.0, noise=5):
    n = shape[-1]
    ph = rng.uniform(0, 6.28, shape[:-1] + (1,))
    return (amp * np.sin(np.arange(n) / period + ph)).astype(np.int64) + rng.integers(-noise, noise + 1, shape)


def _C_spikes():
    """Mono 16-bit, block 384 (12 chunks), k = 4, one wave per case; even waves FIXED order 2, odd
    waves LPC order 2, every lane its own signal. One lane's signal has one spike: of 400 (a code
    over 32 bits) in chunk c for every c, or of 80 (a pair over 32 bits with no code over 32) in
    chunk c for every c >= 1. The last waves hold two spikes, in consecutive chunks of two lanes."""
    plan = [("single", c, 400) for c in range(12)] + [("pair", c, 80) for c in range(1, 12)]
    plan += [("two", 0, 400), ("two", 4, 400), ("two", 10, 400)]

    where, spikes = [], {}
    for w, (what, c, amp) in enumerate(plan):
        lane = (11 * w + 5) % 64
        # an even sample, its three residuals inside the chunk
        spikes[64 * w + lane] = (32 * c + 2 * ((3 * w) % 14) + 2, amp)
        spots = [(lane, c)]
        if what == "two":
            lane2 = (lane + 17) % 64
            spikes[64 * w + lane2] = (32 * (c + 1) + 8, amp)
            spots.append((lane2, c + 1))
        where.append((w, what, spots))

    def make(i, salt):
        x = _signal(np.random.default_rng([0xC000, i, salt]), (C_BS,))
        if i in spikes:
            x[spikes[i][0]] += spikes[i][1]
        return [Sub(samples=x, params=(("k", 4),), **(LPC2 if (i // 64) % 2 else FIX2))]

    cr = write_sync_free(1, 16, C_BS, 64 * len(plan), make)

    def claim():
        for w, what, spots in where:
            sim = craft.simulate_wave(cr, w)
            chunks_hit = [c for _, c in spots]
            assert_quiet(cr, sim, chunks_hit)
            for lane, c in spots:
                assert_one_spoiler(sim, c, (64 * w + lane, 0))
                x = craft.chunks(cr, 64 * w + lane, 0)[c]
                if what == "pair":
                    assert sim[c]["form"] == "pair" and x.pair_max > 32 and x.longest <= 32, (w, x)
                else:
                    assert x.longest > 32, (w, x)
            c0 = chunks_hit[0]
            assert sim[c0]["form"] == ("warm" if c0 == 0 else "pair")
            if what == "two" and c0:  # the first failure switched pairs off: the second is a long code in the one-code form
                assert sim[c0 + 1]["form"] == "one" and sim[c0 + 1]["cool"] == 8
    return Case("C_spikes", cr, claim=claim)


def _C_geometry():
    """Block 352 (11 chunks), k = 4, three waves over FIXED-2 / LPC-2 histories. Wave 0: one lane
    has two partitions of 176, so 16 codes are left at chunk 5 and only that chunk goes back.
    Wave 1: one lane's second of four partitions (88 each: chunks 2, 5 and 8 are cut) is an
    escape partition. Wave 2: one order-0 lane reads 32 codes of 32 bits (k = 11) in each of chunks
    3..6: 4 * 32 words against a ring that holds at most 61 unread words and gains at most 16 per
    chunk, so it runs dry there, in chunk 6 at the latest, with no code or pair too long and
    every lane fast."""
    def make(i, salt):
        rng = np.random.default_rng([0xC100, i, salt])
        x = _signal(rng, (352,))
        if i == 9:
            return [Sub(samples=x, porder=1, params=(("k", 4), ("k", 5)), **FIX2)]
        if i == 64 + 30:
            return [Sub(samples=x, porder=2, params=(("k", 4), ("e", 9), ("k", 3), ("k", 4)), **LPC2)]
        if i == 128 + 41:
            r = filler(rng, 352, 11, 2)
            r[96:224] = unzig((20 << 11) | safe_rem(rng, 11, 128))
            return [Sub(residuals=r, params=(("k", 11),))]
        return [Sub(samples=x, params=(("k", 4),), **(LPC2 if i % 2 else FIX2))]

    cr = write_sync_free(1, 16, 352, 192, make)

    def claim():
        sim = craft.simulate_wave(cr, 0)
        assert_quiet(cr, sim, (5,))
        assert sim[5]["form"] == "slow" and sim[5]["spoilers"] == [((9, 0), "partition ends")]
        sim = craft.simulate_wave(cr, 1)
        assert [ci for ci, r in enumerate(sim) if r["redo"]] == [2, 5, 8]
        assert all(sim[ci]["spoilers"] == [((94, 0), "partition ends")] for ci in (2, 5, 8))
        assert [r["form"] for r in sim][3:5] == ["esc", "esc"] and sim[1]["form"] == "pair"
        sim = craft.simulate_wave(cr, 2)
        assert_quiet(cr, sim)
        assert all(r["form"] == "one" for r in sim[1:])
        x = craft.chunks(cr, 169, 0)
        assert [y.bits for y in x[3:7]] == [1024] * 4 and all(y.longest == 32 for y in x[3:7])
        assert 4 * 1024 > craft.RING_BITS - 3 * 32 + 3 * 512
    return Case("C_geometry", cr, claim=claim)


C_FAILS = (1, 10, 27, 70)


def _C_backoff():
    """The mono pair back-off: one wave, block 4096 (128 chunks), FIXED-2, k = 4. A pair over 32
    bits in chunks 1, 10, 27 and 70 (each the first chunk that tries pairs again): the cool-down
    is 8, then 16, then 32 chunks; the good pair chunks after chunk 60 reset it, so the failure
    in chunk 70 costs 8 again."""
    at = {(13 * i + 2) % 64: 32 * c + 6 for i, c in enumerate(C_FAILS)}

    def make(i, salt):
        x = _signal(np.random.default_rng([0xC200, i, salt]), (4096,))
        if i in at:
            x[at[i]] += 80
        return [Sub(samples=x, params=(("k", 4),), **FIX2)]

    cr = write_sync_free(1, 16, 4096, 64, make)

    def claim():
        sim = craft.simulate_wave(cr)
        assert [ci for ci, r in enumerate(sim) if r["redo"]] == list(C_FAILS)
        assert all(sim[c]["form"] == "pair" for c in C_FAILS)
        assert [sim[c + 1]["cool"] for c in C_FAILS] == [8, 16, 32, 8]
        assert [r["form"] for r in sim[2:10]] == ["one"] * 8 and sim[59]["form"] == "one" and sim[60]["form"] == "pair"
        for i, c in enumerate(C_FAILS):
            x = craft.chunks(cr, (13 * i + 2) % 64, 0)[c]
            assert x.pair_max > 32 and x.longest <= 32
    return Case("C_backoff", cr, claim=claim)


def family_C():
    return [_C_spikes(), _C_geometry(), _C_backoff()]


# ---- D: partition geometry ------------------------------------------------------------------------
def _D_case(tag, bps, bs, order, porder, params, method, fast, forms=None, channels=1):
    def make(f, salt):
        rng = np.random.default_rng([0xD000, sum(map(ord, tag)), f, salt])
        subs = []
        for c in range(channels):
            if order:
                kw = dict(samples=_signal(rng, (bs,), amp=300, noise=2), kind="fixed", order=order)
            else:
                kw = dict(residuals=np.concatenate([filler(rng, bs >> porder, v, 2) for _, v in params]))
            subs.append(Sub(method=method, porder=porder, params=params, **kw))
        return subs

    cr = write_sync_free(channels, bps, bs, 64 // channels, make)

    def claim():
        for f, c in craft.wave_lanes(cr):
            assert [x.fast for x in craft.chunks(cr, f, c)] == fast, (tag, f, c)
        sim = craft.simulate_wave(cr)
        assert [r["form"] == "slow" for r in sim] == [not x for x in fast]
        if forms:
            assert [r["form"] for r in sim] == forms, [r["form"] for r in sim]
        assert not any(r["redo"] for r in sim if r["form"] != "slow")
    return Case(f"D_{tag}", cr, claim=claim)


def family_D():
    k4 = lambda n: (("k", 4),) * n  # noqa: E731
    walk = (("k", 2), ("k", 10), ("k", 0), ("k", 9))
    return [
        _D_case("psize16", 16, 128, 0, 3, k4(8), 0, [False] * 4),
        _D_case("psize32", 16, 128, 0, 2, k4(4), 0, [True] * 4, ["warm"] + ["pair"] * 3),
        _D_case("psize64", 16, 128, 0, 1, k4(2), 0, [True] * 4),
        _D_case("psize32_fixed4", 16, 128, 4, 2, k4(4), 0, [True] * 4),
        _D_case("psize16_stereo", 16, 128, 0, 3, k4(8), 0, [False] * 4, channels=2),
        _D_case("psize32_ch3_24", 24, 128, 0, 2, k4(4), 0, [True] * 4, ["warm"] + ["one"] * 3, channels=3),
        # partition order 4 of a 960-sample block: 60 codes each, so 28 are left after a fast chunk
        _D_case("first60", 16, 960, 0, 4, k4(16), 0, [i % 15 % 2 == 0 for i in range(30)]),
        _D_case("k_walk", 16, 128, 0, 2, walk, 0, [True] * 4, ["warm", "one", "one", "pair"]),
        _D_case("k_walk_512", 16, 512, 0, 2, walk, 0, [True] * 16, ["warm"] + ["pair"] * 3 + ["one"] * 8 + ["pair"] * 4),
        _D_case("k_walk_8bit", 8, 128, 0, 2, (("k", 2), ("k", 5), ("k", 0), ("k", 4)), 0, [True] * 4),
        _D_case("rice2_small_k", 16, 128, 0, 2, (("k", 3), ("k", 14), ("k", 0), ("k", 7)), 1, [True] * 4),
        _D_case("rice2_small_k_24", 24, 128, 0, 2, (("k", 3), ("k", 14), ("k", 0), ("k", 7)), 1, [True] * 4),
    ]


# ---- E: escapes -----------------------------------------------------------------------------------
E_WIDTHS = (0, 1, 2, 15, 16, 17, 31)


def _esc_values(rng, n: int, w: int, bps: int, wide: bool):
    """n values for a w-bit escape partition of an order-0 subframe: as wide as the field and the
    depth allow, or (`wide`) small values in a field wider than they need."""
    if w == 0:
        return np.zeros(n, np.int64)
    b = min(w, bps, 3 if wide else 99)
    if b == w or b < 3:
        return rng.integers(-(1 << (b - 1)), 1 << (b - 1), n)
    # sign-extended in the field: a negative value's run of ones is followed by 01, never by
    # the 00 of a frame sync (bits 1 0 1 x.. in b bits)
    neg = -(1 << (b - 1)) + (1 << (b - 3)) + rng.integers(0, 1 << (b - 3), n)
    return np.where(rng.integers(0, 2, n) == 1, neg, rng.integers(0, 1 << (b - 1), n))


def _E_stream(tag: str, channels: int, bps: int, assignment: str = "indep"):
    """Block 128 in four partitions of 32: escape and Rice partitions alternate, the escape
    widths walk through 0, 1, 2, 15, 16, 17 and 31 as far as the container's InterType goes,
    every other escape partition wider than its values need. Every chunk is fast: the chunks of
    an escape partition take the escape form, a width of 0 reads no bits at all."""
    W = craft.widths(bps)[1]
    ws = [w for w in E_WIDTHS if w <= W]
    per = 64 // channels
    room = bps - (1 if assignment != "indep" else 0)  # mid/side sums stay inside the depth

    used = [ws[i % len(ws)] for i in range(per * channels)] + [ws[(i // 2 + 3) % len(ws)] for i in range(per * channels)]

    def make(f, salt):
        rng = np.random.default_rng([0xE000, bps, channels, f, salt])
        subs = []
        for c in range(channels):
            i = c * per + f
            w1, w2 = ws[i % len(ws)], ws[(i // 2 + 3) % len(ws)]
            params = (("e", w1), ("k", 3), ("e", w2), ("k", 5)) if i % 2 == 0 else (("k", 3), ("e", w1), ("k", 5), ("e", w2))
            parts = [_esc_values(rng, 32, v, room - 1, (i + p) % 4 == 0) if what == "e" else filler(rng, 32, v, 2)
                     for p, (what, v) in enumerate(params)]
            subs.append(Sub(residuals=np.concatenate(parts), porder=2, params=params))
        return subs

    cr = write_sync_free(channels, bps, 128, per, make, assignment=assignment)

    def claim():
        assert set(used) == set(ws)
        sim = craft.simulate_wave(cr)
        assert_quiet(cr, sim)
        assert [r["form"] for r in sim] == ["warm"] + ["esc"] * 3
        zero = [x for f, c in craft.wave_lanes(cr) for x in craft.chunks(cr, f, c) if x.esc and x.escw == 0]
        assert zero and all(x.fast and x.bits <= 9 for x in zero)
        full = [x for f, c in craft.wave_lanes(cr) for x in craft.chunks(cr, f, c) if x.esc and x.escw == max(ws)]
        assert full and all(x.fast for x in full)
    return Case(f"E_{tag}", cr, claim=claim)


def _E_fixed2():
    """Escape partitions over a FIXED-2 history, 16-bit mono: widths 7 (needed) and 8."""
    def make(i, salt):
        x = _signal(np.random.default_rng([0xE100, i, salt]), (128,))
        return [Sub(samples=x, porder=2, params=(("k", 4), ("e", 7 if i % 2 else 8), ("k", 4), ("e", 7)), **FIX2)]

    cr = write_sync_free(1, 16, 128, 64, make)

    def claim():
        sim = craft.simulate_wave(cr)
        assert_quiet(cr, sim)
        assert [r["form"] for r in sim] == ["warm", "esc", "pair", "esc"]
    return Case("E_fixed2_mono16", cr, claim=claim)


def _E_too_wide():
    """An escape width of 17 in an 8-bit container (16-bit InterType): the reader's assertion."""
    rng = np.random.default_rng(0xE200)
    r = np.concatenate([filler(rng, 64, 2, 2), rng.integers(-100, 100, 64)])
    fr = [[Sub(residuals=r if f == 1 else filler(rng, 128, 2, 2), porder=1,
               params=(("k", 2), ("e", 17) if f == 1 else ("k", 2)))] for f in range(3)]
    cr = craft.write(1, 8, 128, fr)

    def claim():
        assert cr.layout[1][0].pesc == (-1, 17) and craft.widths(8)[1] == 16
    return Case("E_escw17_8bit", cr, error="OutOfDomain", claim=claim)


def family_E():
    return [_E_stream("mono8", 1, 8), _E_stream("mono16", 1, 16), _E_stream("mono32", 1, 32),
            _E_stream("stereo16_ms", 2, 16, "ms"), _E_stream("stereo24_ls", 2, 24, "ls"), _E_stream("ch3_16", 3, 16),
            _E_fixed2(), _E_too_wide()]


# ---- F: long zero runs ----------------------------------------------------------------------------
F_RUNS = (31, 32, 63, 64, 95, 96, 2047, 2048, 4095, 4096, 65534)


def _k0_filler(rng, shape):
    """k = 0 codes 01, 001 and 0001: never two 1 bits in a row."""
    return unzig(rng.integers(1, 4, shape))


def _F_stream(tag: str, bps: int, runs, chunk: int):
    """Mono, k = 0, block 128: lane i holds one zero run of runs[i % len(runs)] bits in chunk
    `chunk`, at a sample that moves with the lane; at least two full chunks follow it."""
    def build(salt):
        rng = np.random.default_rng(0xF000 + bps + chunk * 64 + 4096 * salt)
        R = _k0_filler(rng, (64, 128))
        for lane in range(64):
            R[lane, 32 * chunk + (5 * lane) % 32] = int(unzig(runs[lane % len(runs)]))
        return craft.write(1, bps, 128, mono_frames(R, params=(("k", 0),)))

    cr = no_sync(build)

    def claim():
        sim = craft.simulate_wave(cr)
        assert_quiet(cr, sim, (chunk,))
        assert sim[chunk]["redo"] and len(sim[chunk]["spoilers"]) == sum(q >= 32 for q in (runs * 64)[:64])
        assert chunk + 2 < len(sim) and all(r["form"] == "one" for r in sim[chunk + 1:])
        for lane in range(64):
            q = runs[lane % len(runs)]
            x = craft.chunks(cr, lane, 0)[chunk]
            assert (x.longest, x.longest_at, x.zero_peeks) == (q + 1, (5 * lane) % 32, 1 if q >= 32 else 0)
    return Case(f"F_{tag}", cr, claim=claim)


def _F_discard():
    """16-bit container, method 1, k = 20: a quotient of 4096 is shifted out of the 32-bit
    residual type, and the value is the remainder alone. One lane per wave position, chunk 1."""
    def build(salt):
        rng = np.random.default_rng(0xF100 + 4096 * salt)
        frames, rems = [], []
        for lane in range(64):
            r = unzig(rng.integers(1, 3, 128) << 14 | safe_rem(rng, 14, 128)) if lane % 8 else np.zeros(128, np.int64)
            k = 14 if lane % 8 else 20
            raw = None
            if k == 20:
                r = unzig(safe_rem(rng, 15, 128))  # quotient 0, remainders below 2**15
                rem = int(safe_rem(rng, 16)) | 1
                raw = {32 + lane // 2: (4096, rem)}
                rems.append((lane, rem))
            frames.append([Sub(residuals=r, method=1, params=(("k", k),), raw=raw)])
        return craft.write(1, 16, 128, frames), rems

    cr, rems = no_sync(build)

    def claim():
        assert len(rems) == 8
        for lane, rem in rems:
            x = craft.chunks(cr, lane, 0)[1]
            assert (x.longest, x.longest_at) == (4096 + 21, lane // 2)
            assert cr.pcm[128 * lane + 32 + lane // 2] == int(unzig(rem)) == craft.decoded_raw(4096, rem, 20, 32)
        sim = craft.simulate_wave(cr)
        assert_quiet(cr, sim, (1,))
        assert len(sim[1]["spoilers"]) == 8
    return Case("F_discard_k20", cr, claim=claim)


def _F_error(tag: str, q: int):
    """8-bit container: a quotient of 0xFFFF decodes to -32768, outside the SampleType; one of
    0x10000 does not fit the 16-bit residual type. Both are the reader's OutOfDomain."""
    rng = np.random.default_rng(0xF200 + q)
    fr = [[Sub(residuals=_k0_filler(rng, 128), params=(("k", 0),), raw={40: (q, 0)} if f == 1 else None)] for f in range(3)]
    cr = craft.write(1, 8, 128, fr)

    def claim():
        assert craft.chunks(cr, 1, 0)[1].longest == q + 1 and not any(craft.sync_positions(cr, f) for f in range(3))
    return Case(f"F_{tag}", cr, error="OutOfDomain", claim=claim)


def family_F():
    return [_F_stream("mono16_chunk1", 16, F_RUNS, 1), _F_stream("mono16_chunk0", 16, F_RUNS, 0),
            _F_stream("mono8_chunk1", 8, (31, 32, 63, 64, 95, 96, 255), 1),
            _F_stream("mono24_chunk1", 24, F_RUNS + (65535, 100000), 1),
            _F_discard(), _F_error("mono8_q65535", 0xFFFF), _F_error("mono8_q65536", 0x10000)]


# ---- G: bit rate ----------------------------------------------------------------------------------
def _G_stream(tag: str, bps: int, ks, method: int, rate_bits: int):
    """Mono, block 384 (12 chunks), order 0. Lane i has k = ks[i % len(ks)]: with k = 0 every
    residual is 0 (one bit per sample), else the quotient is 1..3, more than `rate_bits` per
    sample: what a top-up brings in per chunk."""
    def build(salt):
        rng = np.random.default_rng(0x6000 + bps + len(ks) + sum(ks) * 64 + 4096 * salt)
        frames = []
        for lane in range(64):
            k = ks[lane % len(ks)]
            r = filler(rng, 384, k, 3) if k else np.zeros(384, np.int64)
            frames.append([Sub(residuals=r, method=method, params=(("k", k),))])
        return craft.write(1, bps, 384, frames)

    cr = no_sync(build)

    def claim():
        assert_quiet(cr, craft.simulate_wave(cr))
        for lane in range(64):
            k = ks[lane % len(ks)]
            bits = [x.bits for x in craft.chunks(cr, lane, 0)]
            if k:
                assert min(bits) > 32 * rate_bits, (lane, bits)
            else:
                assert bits == [32] * 12
    return Case(f"G_{tag}", cr, claim=claim)


def family_G():
    return [_G_stream("thin16", 16, (0,), 0, 16), _G_stream("fat16_k14", 16, (14,), 0, 16),
            _G_stream("thin_fat16", 16, (0, 14), 0, 16), _G_stream("fat24_k22", 24, (22,), 1, 24),
            _G_stream("thin_fat24", 24, (22, 0), 1, 24), _G_stream("thin8", 8, (0,), 0, 16)]


# ---- H: k_walk_wave -------------------------------------------------------------------------------
def _H_runs(channels: int, bps: int, k: int):
    """Blocks of 64, one partition. In every channel but the last, frame f holds in sample 20 a
    zero run that covers exactly 1 + f % 3 whole 64-bit segments of k_walk_wave's scan, and in
    sample 40 a code that ends exactly on a segment boundary. (Positions come from a first
    writing with placeholders: neither code moves when its own length changes.)"""
    per = 64 // channels

    def build(salt):
        rng = np.random.default_rng(0x8000 + channels * 64 + bps + k + 4096 * salt)
        R = filler(rng, (per, channels, 64), k, 2)

        def wr(n=per):
            return craft.write(channels, bps, 64, [[Sub(residuals=R[f, c], params=(("k", k),)) for c in range(channels)]
                                                   for f in range(n)])
        for f in range(per):  # in stream order: a placement moves every later code, and a frame every later frame
            for c in range(channels - 1):
                for at in (20, 40):
                    L = wr(f + 1).layout[f][c]
                    s = int(L.cpos[at])
                    to_edge = ((int(L.cpos[0]) & ~31) - s) % 64
                    if at == 20:
                        # zeros from s on: `to_edge` to the boundary, n whole segments, a few more
                        q = to_edge + 64 * (1 + f % 3) + (f % 7)
                    else:
                        q = (to_edge - k - 1) % 64 + (64 if f % 2 else 0)
                    R[f, c, at] = code(rng, q, k)
        return wr()

    cr = no_sync(build)

    def claim():
        whole = set()
        for f in range(per):
            for c in range(channels - 1):
                L = cr.layout[f][c]
                seg = craft.segments(cr, f, c, 0)
                assert len(seg) == 1
                wbase = seg[0]["wbase"]
                s, n = int(L.cpos[20]), int(L.clen[20])
                first = wbase + -(-(s - wbase) // 64) * 64          # first segment boundary at or after the run's start
                covered = (s + (n - k - 1) - first) // 64           # whole segments inside the zeros
                assert covered == 1 + f % 3 and s >= wbase, (f, c, s, n)
                whole.add(covered)
                assert (int(L.cpos[40]) + int(L.clen[40]) - wbase) % 64 == 0, (f, c)
        assert whole == {1, 2, 3}
    return Case(f"H_runs_ch{channels}_{bps}bit_k{k}", cr, claim=claim)


def _H_scans(channels: int):
    """16-bit, block 384, two partitions of 192, k = 9. Channel 0's first partition ends exactly
    at bit 4096 of its first scan (its last code's quotient is chosen for that); the second
    partition, and both of the other walked channels, are longer than a scan."""
    per = 64 // channels

    def build(salt):
        rng = np.random.default_rng(0x8100 + channels + 4096 * salt)
        R = unzig((rng.integers(10, 21, (per, channels, 384)) << 9) | safe_rem(rng, 9, (per, channels, 384)))
        Q = rng.integers(8, 15, (per, 190))
        R[:, 0, :190] = unzig((Q << 9) | safe_rem(rng, 9, (per, 190)))

        def wr(n=per):
            return craft.write(channels, 16, 384, [[Sub(residuals=R[f, c], porder=1, params=(("k", 9), ("k", 9)))
                                                    for c in range(channels)] for f in range(n)])
        for f in range(per):  # (a frame's length moves every later frame)
            L = wr(f + 1).layout[f][0]
            wbase = int(L.cpos[0]) & ~31
            q = wbase + 4096 - int(L.cpos[190]) - 20  # the quotients of the last two codes
            assert 0 <= q <= 2 * 127, q  # (an order-0 16-bit sample: quotient < 128 at k = 9)
            R[f, 0, 190], R[f, 0, 191] = code(rng, q - q // 2, 9), code(rng, q // 2, 9)
        return wr()

    cr = no_sync(build)

    def claim():
        for f in range(per):
            seg = craft.segments(cr, f, 0, 0)
            assert len(seg) == 1 and seg[0]["next"] == seg[0]["wbase"] + 4096, (f, seg[0]["next"] - seg[0]["wbase"])
            assert len(craft.segments(cr, f, 0, 1)) >= 2
            for c in range(1, channels - 1):
                assert len(craft.segments(cr, f, c, 0)) >= 2
    return Case(f"H_scans_ch{channels}", cr, claim=claim)


def _H_k30(channels: int):
    """32-bit, method 1, k = 30, block 64: remainders of all zeros and of all ones in the walked
    channels, each followed by a code that starts 01 (no FF F8 can follow the ones)."""
    per = 64 // channels
    ones = (1 << 30) - 1

    def build(salt):
        rng = np.random.default_rng(0x8200 + channels + 4096 * salt)
        R = unzig((rng.integers(1, 2, (per, channels, 64)) << 30) | safe_rem(rng, 30, (per, channels, 64)))
        for f in range(per):
            for c in range(channels - 1):
                for j, at in enumerate(range(3 + f % 5, 60, 9)):
                    R[f, c, at] = code(rng, (f + j) % 3, 30, rem=ones if (j + f + c) % 2 else 0)
        return craft.write(channels, 32, 64, [[Sub(residuals=R[f, c], method=1, params=(("k", 30),))
                                               for c in range(channels)] for f in range(per)])

    cr = no_sync(build)

    def claim():
        seen = set()
        for f in range(per):
            for c in range(channels - 1):
                v = cr.pcm_array.reshape(-1, 64, channels)[f, :, c]
                zz = np.where(v >= 0, 2 * v, -2 * v - 1)
                seen |= set((zz[(zz & ones) == 0] >> 30).tolist()) | {-1 - int(x) for x in (zz[(zz & ones) == ones] >> 30)}
        assert {0, 1, 2, -1, -2, -3} <= seen
    return Case(f"H_k30_ch{channels}", cr, claim=claim)


def family_H():
    return [_H_runs(3, 16, 0), _H_runs(3, 16, 3), _H_runs(2, 16, 5), _H_runs(2, 24, 9), _H_runs(3, 24, 1),
            _H_scans(3), _H_scans(2), _H_k30(3), _H_k30(2)]


# ---- W: what else the writer writes ---------------------------------------------------------------
def _W_case(tag, channels, bps, bs, sub_of, assignment="indep", forms=None):
    """One wave whose subframes come from sub_of(rng, frame, channel, signal): the writer's
    subframe types, wasted bits, LPC fields, channel assignments and channel counts, held to
    the oracle like every other case and decoded in the bucket their orders name."""
    per = 64 // channels

    def make(f, salt):
        rng = np.random.default_rng([0x3000, sum(map(ord, tag)), f, salt])
        amp = 1 << (bps - 4)
        return [sub_of(rng, f, c, _signal(rng, (bs,), amp=amp, period=9.0 + c, noise=max(1, amp >> 7)))
                for c in range(channels)]

    cr = write_sync_free(channels, bps, bs, per, make, assignment=assignment)

    def claim():
        sim = craft.simulate_wave(cr)
        if forms:
            assert [r["form"] for r in sim] == forms, [r["form"] for r in sim]
        assert not any(r["redo"] for r in sim if r["form"] != "slow")
    return Case(f"W_{tag}", cr, claim=claim)


def _fit_k(r) -> int:
    """A Rice parameter that keeps every code of these residuals short."""
    return max(0, int(np.abs(np.asarray(r)).max()).bit_length() - 1)


def family_W():
    def fixed_and_lpc(rng, f, c, x):
        """channel 0: FIXED order 2; channel 1 (the side channel, where there is one): LPC order 3
        with 2 wasted bits."""
        if c == 0:
            sub = Sub(kind="fixed", order=2, samples=x)
        else:
            sub = Sub(kind="lpc", order=3, coefs=(5, -4, 1), precision=5, shift=1, wasted=2, samples=x >> 3)
        k = _fit_k(craft._sub_values(sub, x.size, 64)[1])
        sub.method, sub.params = (1 if k > 14 else 0), (("k", k),)
        return sub

    def mixed(rng, f, c, x):
        if c == 0:
            return Sub(kind="const", samples=[int(x[0]) >> 1], wasted=1 if f % 2 else 0)
        if c == 1:
            return Sub(kind="verbatim", samples=x >> 2, wasted=2 if f % 3 == 0 else 0)
        sub = Sub(kind="fixed", order=1, samples=x, method=1)
        sub.params = (("k", _fit_k(craft._sub_values(sub, x.size, 64)[1])),)
        return sub

    def orders(rng, f, c, x):
        sub = Sub(kind="fixed", order=(c + f) % 5, samples=x, porder=1)
        k = min(14, _fit_k(craft._sub_values(sub, x.size, 32)[1]))
        sub.params = (("k", k), ("e", min(31, k + 3)))
        return sub

    def lpc8(rng, f, c, x):
        sub = Sub(kind="lpc", order=8, coefs=(1500, -700, 300, -100, 40, -20, 8, -3), precision=12, shift=10, samples=x,
                  method=1, porder=2)
        k = _fit_k(craft._sub_values(sub, x.size, 64)[1])
        sub.params = (("k", k), ("k", k + 1), ("e", min(31, k + 3)), ("k", k))
        return sub

    out = [_W_case(f"stereo16_{a}", 2, 16, 192, fixed_and_lpc, a) for a in ("indep", "ls", "sr", "ms")]
    out += [_W_case("stereo8_ms", 2, 8, 96, fixed_and_lpc, "ms"), _W_case("stereo32_ls", 2, 32, 96, fixed_and_lpc, "ls"),
            _W_case("mix_ch3_24", 3, 24, 96, mixed, forms=["mixed"] * 3),
            _W_case("orders_ch8_12", 8, 12, 128, orders), _W_case("orders_ch5_16", 5, 16, 64, orders),
            _W_case("lpc8_mono20", 1, 20, 256 + 128, lpc8)]
    return out


@functools.lru_cache(maxsize=None)
def family(name: str) -> tuple:
    return tuple(globals()[f"family_{name}"]())


def all_cases() -> list:
    return [c for name in FAMILIES for c in family(name)]


def expected_buckets(crs) -> int:
    """The decode buckets the frame groups of a batch of crafted streams classify into: per class
    (container, channel count) the frames in batch order, 64 // channels at a time."""
    classes = {}
    for cr in crs:
        rows = classes.setdefault((craft.widths(cr.bps)[0], cr.channels), [])
        for subs in cr.layout:
            rows.append((max([s.order for s in subs if s.kind in ("fixed", "lpc")], default=0),
                         any(s.kind in ("const", "verbatim") for s in subs)))
    used = 0
    for (_, nch), rows in classes.items():
        per = 64 // nch
        for g in range(0, len(rows), per):
            order = max(o for o, _ in rows[g:g + per])
            mix = any(m for _, m in rows[g:g + per])
            if mix:
                used |= _lib.BUCKET_MIX_8 if order <= 8 else _lib.BUCKET_MIX_32
            else:
                used |= next(getattr(_lib, f"BUCKET_{mb}") for mb in (4, 8, 12, 16, 32) if order <= mb)
    return used
