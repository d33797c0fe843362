"""Streams that sit on the exact value-range edges of the predictor and of the stereo
decorrelation, built with tests/craft.py from chosen samples: the SampleType of a predicted
sample (S), the InterType of the LPC products and partial sums for 8-bit (I) and 16-bit (J)
containers, the decorrelation (D), the raw reads (R) and which error wins (P).

`model()` is an exact-integer restatement of the value checks of Debug zflac
(src/zflac.zig:425-578), in Python integers, from the `Sub`s of a stream alone: it knows neither
the oracle nor the kernels. It returns the first trap in zflac's read order, or None.

A `Case` is a stream of three frames with the edge in frame 1, the error name the reader must
report, the trap the case aims at (`aim`: frame, channel, sample, check) and the kernel path the
edge sample's chunk takes: "fast" (a whole chunk past the first), "warm" (the subframe's first
chunk) or "generic" (a block's tail, or an `unsafe` lane). Every edge comes as a pair: the last
admissible value (OK, decoded exactly) and the first inadmissible one.

`batch(name)` orders a family's cases for one zflac_amd.Batch. The decode kernels take the
frames of a class (container, channel count) in batch order, 64 // channels to a wave, and one
lane that needs the generic path sends its whole wave there for that chunk. So the cases are
sorted by class and `group`, and every group is padded to whole waves by a plain stream:
`assert_paths` then shows, from craft's chunk model, that no lane of a fast or warm case's wave
spoils the edge's chunk. A builder module like rice_edges.py: tests/test_value_edges.py holds
the assertions."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from . import craft
from .craft import Sub
from .rice_edges import write_sync_free

FAMILIES = ("S", "I", "J", "D", "R", "P")
BS_OF = {"fast": 64, "warm": 32, "generic": 48}
LPC2 = dict(kind="lpc", order=2, coefs=(7, -3), precision=4, shift=2)  # keeps a constant: (7 - 3) / 4
PREDICTORS = {"fixed1": dict(kind="fixed", order=1), "fixed4": dict(kind="fixed", order=4), "lpc": LPC2}


# ---- the model ------------------------------------------------------------------------------------
def fits(v: int, bits: int) -> bool:
    return -(1 << (bits - 1)) <= v <= (1 << (bits - 1)) - 1


def wrap(v: int, bits: int) -> int:
    m = 1 << bits
    v &= m - 1
    return v - m if v >> (bits - 1) else v


class _Trap(Exception):
    pass


def sub_residuals(sub: Sub, bs: int):
    """(warm-up samples, residuals) of a fixed / lpc subframe as Python integers."""
    o = sub.order
    coefs = craft.FIXED_COEFS[o] if sub.kind == "fixed" else tuple(int(c) for c in sub.coefs)
    if sub.samples is None:
        assert not sub.raw
        return coefs, [int(x) for x in sub.warmup], [int(x) for x in sub.residuals]
    s = [int(x) for x in sub.samples]
    assert len(s) == bs
    res = [s[i] - (sum(coefs[j] * s[i - 1 - j] for j in range(o)) >> sub.shift) for i in range(o, bs)]
    return coefs, s[:o], res


def _model_sub(sub: Sub, bs: int, bps: int, ubps: int, SB: int, W: int) -> list:
    """One subframe (src/zflac.zig:444-541): its samples after the wasted-bits shift."""
    def need(ok, i, what):
        if not ok:
            raise _Trap(i, what)
    w = sub.wasted
    if sub.kind == "const":  # :447 the frame's depth, @intCast to the SampleType
        v = int(np.asarray(sub.samples).reshape(-1)[0])
        need(fits(v, SB), 0, "const")
        return [wrap(v << w, SB)] * bs
    if sub.kind == "verbatim":  # :459,463
        out = []
        for i, v in enumerate(int(x) for x in sub.samples):
            need(fits(v, SB), i, "verbatim")
            out.append(wrap(v << w, SB))
        return out
    coefs, warm, res = sub_residuals(sub, bs)
    o = sub.order
    for i, v in enumerate(warm):  # :474,506
        need(fits(v, SB), i, "warmup")
    assert all(fits(r, W) for r in res), "a residual outside the ResidualType"
    buf = warm + res
    if sub.kind == "lpc" and bs > o:  # :531 @intCast(shift) to Log2Int(InterType)
        need(sub.shift < W, o, "shift")
    for i in range(o, bs):  # :526-533
        p = 0
        for j in range(o - 1, -1, -1):  # oldest sample first
            prod = buf[i - 1 - j] * coefs[j]
            need(fits(prod, W), i, "product")
            p += prod
            need(fits(p, W), i, "partial")
        v = buf[i] + (p >> sub.shift)
        need(fits(v, W), i, "inter")
        buf[i] = v
    out = []
    for i, v in enumerate(buf):  # :536-540 @intCast, then the wasted-bits shift, which wraps
        need(fits(v, SB), i, "sample")
        out.append(wrap(v << w, SB))
    return out


def model(frames, channels: int, bps: int, bs: int, assignment: str = "indep"):
    """(first trap or None, PCM up to it): the trap is (frame, channel, sample, check)."""
    SB, W = craft.widths(bps)
    code = craft.ASSIGN[assignment]
    pcm = []
    for f, subs in enumerate(frames):
        ch = []
        for c, sub in enumerate(subs):
            side = code is not None and c == (0 if code == 9 else 1)
            try:
                ch.append(_model_sub(sub, bs, bps, bps + (1 if side else 0), SB, W))
            except _Trap as t:
                return (f, c) + t.args, pcm
        for i in range(bs if code else 0):  # :553-578
            x0, x1 = ch[0][i], ch[1][i]
            if code == 8:
                if not fits(x0 - x1, SB):
                    return (f, 1, i, "decor"), pcm
                ch[1][i] = x0 - x1
            elif code == 9:
                if not fits(x0 + x1, SB):
                    return (f, 0, i, "decor"), pcm
                ch[0][i] = x0 + x1
            else:
                mid = (x0 << 1) + (x1 & 1)
                assert fits(mid + x1, W) and fits(mid - x1, W)
                for c, v in enumerate(((mid + x1) >> 1, (mid - x1) >> 1)):
                    if not fits(v, SB):
                        return (f, c, i, "decor"), pcm
                    ch[c][i] = v
        pcm += [ch[c][i] for i in range(bs) for c in range(channels)]
    return None, pcm


# ---- cases ----------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    name: str
    cr: craft.Crafted
    frames: list
    error: str = "OK"
    aim: tuple = None        # (frame, channel, sample, check) of the trap the case is built for
    path: str = "fast"       # of the chunk holding sample `at` of frame 1
    at: int = 0
    group: str = ""
    pure_ms: bool = False    # the wave must take the mid/side forms (D_MS)
    flac: bytes = None       # the bytes, where they are not the writer's (family P)

    @property
    def data(self) -> bytes:
        return self.flac if self.flac is not None else self.cr.flac


def choose_k(res) -> tuple:
    """(k, longest code) for these residuals: the fewest bits among the parameters whose
    longest code fits the 32-bit peek, else the shortest longest code."""
    zz = [2 * r if r >= 0 else -2 * r - 1 for r in (int(x) for x in res)] or [0]
    best = ()
    for k in range(1, 31):  # (k = 0 writes a run of zero residuals as a run of 1 bits: FF bytes)
        longest = (max(zz) >> k) + 1 + k
        key = (longest > 32, sum((z >> k) + 1 + k for z in zz) if longest <= 32 else longest, k)
        best = min(best, key) if best else key
    return best[2], (max(zz) >> best[2]) + 1 + best[2]


def coded(sub: Sub, bs: int, bump: int = 0) -> Sub:
    """The subframe with Rice parameters chosen: two partitions for a block of 64 (so that what
    chunk 0 needs does not lengthen chunk 1's codes), else one. `bump` raises the first
    partition's parameter where its codes stay within 32 bits: another bit layout, same values."""
    if sub.kind in ("const", "verbatim"):
        return sub
    _, _, res = sub_residuals(sub, bs)
    sub.porder = 1 if bs == 64 else 0
    b = craft._part_bounds(dataclasses.replace(sub, params=(("k", 0),) * (1 << sub.porder)), bs)
    parts = [res[b[p] - sub.order:b[p + 1] - sub.order] for p in range(len(b) - 1)]
    ks = [choose_k(r)[0] for r in parts]
    for _ in range(bump):
        zz = max([2 * r if r >= 0 else -2 * r - 1 for r in parts[0]] or [0])
        if ks[0] < 30 and (zz >> (ks[0] + 1)) + ks[0] + 2 <= 32:
            ks[0] += 1
    sub.method = 1 if max(ks) > 14 else 0
    sub.params = tuple(("k", k) for k in ks)
    return sub


def plain_sub(rng, bs: int, amp: int = 20) -> Sub:
    return coded(Sub(kind="fixed", order=1, samples=rng.integers(-amp, amp + 1, bs)), bs)


def make(name, channels, bps, bs, edge_subs, assignment="indep", **kw) -> Case:
    """Three frames: plain, the edge frame, plain; a frame that holds a byte-aligned sync pattern
    is written again, the plain ones from other noise, the edge frame with another parameter."""
    kept = {}

    def frame(i, salt):
        if i == 1:
            kept[i] = [coded(dataclasses.replace(s), bs, salt) for s in edge_subs]
        else:
            rng = np.random.default_rng([sum(map(ord, name)), bps, bs, i, salt])
            kept[i] = [plain_sub(rng, bs) for _ in range(channels)]
        return kept[i]
    cr = write_sync_free(channels, bps, bs, 3, frame, assignment=assignment)
    kw.setdefault("path", {64: "fast", 32: "warm", 48: "generic"}[bs])
    kw.setdefault("at", bs - 1)
    return Case(name, cr, [kept[i] for i in range(3)], **kw)


def pad_stream(name, like: Case, n: int) -> Case:
    """n plain frames of `like`'s shape, for the end of a group."""
    cr0, kept = like.cr, {}

    def frame(i, salt):
        rng = np.random.default_rng([sum(map(ord, name)), n, i, salt])
        kept[i] = [plain_sub(rng, cr0.bs) for _ in range(cr0.channels)]
        return kept[i]
    cr = write_sync_free(cr0.channels, cr0.bps, cr0.bs, n, frame, assignment=cr0.assignment)
    return Case(name, cr, [kept[i] for i in range(n)], path="pad", group=like.group)


def ramp(bs: int, order: int, level: int, tail=()) -> list:
    """Zeros for the warm-up, a raised-cosine rise to `level` that ends before the block's last
    chunk, `level` held, then `tail` as the block's last samples."""
    end = {64: 28, 32: 22, 48: 36}[bs]
    n = end - order
    s = [0] * order + [int(round(level * (1 - math.cos(math.pi * (i + 1) / n)) / 2)) for i in range(n)]
    s += [level] * (bs - len(s))
    s[-1] = level
    if tail:
        s[-len(tail):] = list(tail)
    return s


def tail_block(bs: int, tail) -> list:
    """Zeros, then `tail` as the block's last samples."""
    return [0] * (bs - len(tail)) + list(tail)


def ok_trap(out, name, builder, ok, bad, aim_check, **kw):
    """The pair of an edge: builder(value) -> make() arguments."""
    for tag, v, err in (("ok", ok, "OK"), ("trap", bad, "OutOfDomain")):
        args, mkw = builder(v)
        mkw = dict(mkw, **kw)
        if err != "OK":
            ch = mkw.pop("aim_ch", 0)
            at = mkw.get("at", args[2] - 1)
            mkw.update(error=err, aim=(1, ch, mkw.pop("aim_at", at), aim_check))
        else:
            mkw.pop("aim_ch", None)
            mkw.pop("aim_at", None)
        out.append(make(f"{name}_{tag}", *args, **mkw))


# ---- S: the SampleType of a predicted sample ------------------------------------------------------
def family_S():
    out = []
    depths = (8, 12, 16, 20, 24, 32)
    for di, bps in enumerate(depths):
        SB = craft.widths(bps)[0]
        hi, lo = (1 << (SB - 1)) - 1, -(1 << (SB - 1))
        for pi, path in enumerate(("fast", "warm", "generic")):
            bs = BS_OF[path]
            names = list(PREDICTORS) if bps in (8, 16) else [list(PREDICTORS)[(pi + di) % 3]]
            for pn in names:
                pred = PREDICTORS[pn]
                for side, level, ok, bad in (("max", hi - 5, hi, hi + 1), ("min", lo + 5, lo, lo - 1)):
                    def builder(v, level=level, pred=pred, bs=bs, bps=bps):
                        return (1, bps, bs, [Sub(samples=ramp(bs, pred["order"], level, (v,)), **pred)]), {}
                    ok_trap(out, f"S_{bps}_{path}_{pn}_{side}", builder, ok, bad, "sample",
                            group="gen" if path == "generic" else "fast")
    # the corner the 16-bit fast path's comment rests on: r = -2^30 as a 32-bit code against a
    # prediction of -2^30 from the last safe coefficients; the sum -2^31 still reads as out of range
    def corner(v):
        sub = Sub(kind="lpc", order=3, coefs=(16383, 16383, 2), precision=15, shift=0,
                  samples=tail_block(64, (-32768, -32768, -32768, v)))
        return (1, 16, 64, [sub]), {}
    ok_trap(out, "S_16_fast_corner", corner, -32768, -(1 << 31), "sample", group="fast")
    return out


# ---- I: the InterType of 8-bit containers (i16) ---------------------------------------------------
def lpc_tail(bps, bs, coefs, precision, shift, tail, **kw):
    """A mono LPC stream: zeros, then `tail` (the history and the edge sample)."""
    sub = Sub(kind="lpc", order=len(coefs), coefs=tuple(coefs), precision=precision, shift=shift,
              samples=tail_block(bs, tail))
    return (1, bps, bs, [sub]), kw


def sparse_coefs(order: int, lag: int) -> tuple:
    """-255 at `lag`, -1 at lag 1 (bitstream order: index 0 multiplies the previous sample)."""
    c = [0] * order
    c[lag - 1] = -255
    c[0] += -1
    return tuple(c)


def family_I():
    out = []
    c255 = (-32,) * 7 + (-31,)
    # sum |c| = 255: the last safe lane, fast path; the sum is +32640
    ok_trap(out, "I_sum255_shift8", lambda v: lpc_tail(8, 64, c255, 7, 8, (-128,) * 8 + (v,)), 127, 128, "sample", group="fast8")
    ok_trap(out, "I_sum255_shift0", lambda v: lpc_tail(8, 64, c255, 7, 0, (-128,) * 8 + (v,)), 127, 128, "sample", group="fast8")
    # sum |c| = 256: +32768 traps at the last partial sum, +32736 and -32768 do not
    ok_trap(out, "I_sum256_pos", lambda h: lpc_tail(8, 64, (-32,) * 8, 7, 0, (h,) + (-128,) * 7 + (127,)), -127, -128,
            "partial", group="gen8", path="generic")
    out.append(make("I_sum256_neg_ok", *lpc_tail(8, 64, (32,) * 8, 7, 0, (-128,) * 8 + (-128,))[0], group="gen8", path="generic"))
    # one product: -128 * -256 = +32768 traps, -128 * 256 = -32768 does not
    ok_trap(out, "I_product", lambda c: lpc_tail(8, 64, (c,), 10, 0, (-128, -128 if c > 0 else 127)), 256, -256, "product", group="gen4",
            path="generic")
    # a partial sum that leaves the InterType although the whole sum returns to it, and the
    # mirror, where only the newest-first order would leave it
    ok_trap(out, "I_transient", lambda c: lpc_tail(8, 64, c, 9, 15, ((-128, -128, 127, 5) if c[0] > 0 else (127, -128, -128, 127, 5))),
            (200, -200, 200), (-200, -200, -200), "partial", group="gen4", path="generic")
    out.append(make("I_transient_mirror_ok", *lpc_tail(8, 64, (-200, -200, -200), 9, 15, (127, -128, -128, 5))[0], group="gen4",
                    path="generic"))
    # every history bucket: -255 at the oldest (or a middle) lag and -1 at lag 1 over a history that
    # is loud only there: 32640 + 127 = 32767 fits, 32640 + 128 does not
    for order in (2, 3, 8, 12, 16, 32):
        for lag in sorted({order, order // 2 + 1}):
            if lag == 1:
                continue
            def builder(newest, order=order, lag=lag):
                hist = [0] * order
                hist[order - lag] = -128
                hist[-1] = newest
                return lpc_tail(8, 64, sparse_coefs(order, lag), 9, 15, tuple(hist) + (3,))
            bucket = next(m for m in (4, 8, 12, 16, 32) if order <= m)
            ok_trap(out, f"I_order{order}_lag{lag}", builder, -127, -128, "partial", group=f"gen{bucket}", path="generic")
    return out


# ---- J: the InterType of 16-bit containers (i32) --------------------------------------------------
def family_J():
    out = []
    lo = -32768
    # sum |c| = 32768 is the last safe lane, 32769 the first unsafe one: the same samples from both
    for tag, c3, grp, path in (("safe", 2, "fast", "fast"), ("unsafe", 3, "gen", "generic")):
        ok_trap(out, f"J_sum_{tag}", lambda v, c3=c3: lpc_tail(16, 64, (16383, 16383, c3), 15, 0, (lo, lo, lo, v)), lo, lo - 1,
                "sample", group=grp, path=path)
    # the sum -2^31 fits, -2^31 - 1 and +2^31 do not
    c6 = (1, 2, -16384, -16384, -16384, -16384)  # bitstream order: the newest sample first
    ok_trap(out, "J_sum_min", lambda s: lpc_tail(16, 64, c6, 15, 16, (32767,) * 4 + (lo, s, 7)), 0, -1, "partial", group="gen",
            path="generic")
    ok_trap(out, "J_sum_max", lambda h: lpc_tail(16, 64, (-16384,) * 4, 15, 16, (h, lo, lo, lo, 7)), lo + 1, lo, "partial",
            group="gen", path="generic")
    # the transient pair and its mirror
    n, p = -16384, 16383
    ok_trap(out, "J_transient", lambda c: lpc_tail(16, 64, c, 15, 16, ((32767,) if c[1] < 0 else ()) + (lo, lo, lo, lo, 32767, 7)),
            (n, p, n, p, n), (n,) * 5, "partial", group="gen", path="generic")
    out.append(make("J_transient_mirror_ok", *lpc_tail(16, 64, (n,) * 5, 15, 16, (32767, lo, lo, lo, lo, 7))[0], group="gen",
                    path="generic"))
    # shifts 0 and 31 over a sum of -1, which floors to -1
    for shift in (0, 31):
        ok_trap(out, f"J_shift{shift}", lambda v, shift=shift: lpc_tail(16, 64, (-1,), 2, shift, (1, v)), lo, lo - 1, "sample",
                group="fast")
    # 8-bit containers: a shift of 15 is the last one the InterType's shift type holds
    ok_trap(out, "J_8bit_shift", lambda sh: lpc_tail(8, 64, (-1,), 2, sh, (1, 9)), 15, 16, "shift", group="fast8", aim_at=1)
    return out


# ---- D: the decorrelation -------------------------------------------------------------------------
def ms_side(ch: int, M: int, T: int, parity: int) -> int:
    """The side value that makes mid/side output `ch` equal T over mid M: L = M + ceil(S / 2),
    R = M - floor(S / 2); `parity` 1 takes the odd side where there is one."""
    return (2 * (T - M) - parity) if ch == 0 else (2 * (M - T) + parity)


def decor_values(assign: str, ch: int, T: int, SB: int, parity: int):
    """Coded channel values (x0, x1) whose output channel `ch` is T; both fit the SampleType."""
    hi, lo = (1 << (SB - 1)) - 1, -(1 << (SB - 1))
    pos = T > 0
    if assign == "ls":   # R = L - S
        return (hi, hi - T) if pos else (lo, lo - T)
    if assign == "sr":   # L = S + R
        R = hi - 1 if pos else lo + 1
        return T - R, R
    M = hi - 7 if pos else lo + 8
    return M, ms_side(ch, M, T, parity)


def decor_case(out, name, assign, bps, bs, ch, T_ok, T_bad, back, parity=0, wasted_lane=False, **kw):
    """A stereo pair whose output channel `ch` meets T at sample bs - 1 - back."""
    SB = craft.widths(bps)[0]

    def builder(T):
        x0, x1 = decor_values(assign, ch, T, SB, parity)
        q0, q1 = decor_values(assign, ch, T_ok, SB, 0)  # what the channels hold elsewhere: near, inside
        if assign == "ms":
            q1 = 0
        elif assign == "ls":
            q1 = 0
        else:
            q0 = 0
        t0, t1 = ((x0,), (x1,)) if back == 0 else ((x0, q0), (x1, q1))
        subs = [Sub(kind="fixed", order=1, samples=ramp(bs, 1, q0, t0)),
                Sub(kind="fixed", order=1, samples=ramp(bs, 1, q1, t1))]
        if wasted_lane:  # channel 0 of every frame coded with one wasted bit: even values only
            subs[0] = Sub(kind="fixed", order=1, wasted=1, samples=[v >> 1 for v in ramp(bs, 1, q0 & ~1, tuple(t & ~1 for t in t0))])
        return (2, bps, bs, subs), dict(assignment=assign)
    ok_trap(out, name, builder, T_ok, T_bad, "decor", aim_ch=ch, at=bs - 1 - back, **kw)


def family_D():
    out = []
    edges16 = ((32767, 32768), (-32768, -32769))
    chans = {"ls": (1,), "sr": (0,), "ms": (0, 1)}
    # 16-bit, fast: a wave of mid/side lanes with no shifts takes D_MS ...
    for ch in (0, 1):
        for ok, bad in edges16:
            for parity in (0, 1):
                for back in (0, 1):  # the last sample: the high half of its packed pair; the one before: the low half
                    decor_case(out, f"D_16_msform_ch{ch}_{'hi' if ok > 0 else 'lo'}_p{parity}_b{back}", "ms", 16, 64, ch, ok, bad,
                               back, parity, group="ms", pure_ms=True)
    # ... and beside left/side and side/right lanes D_GEN
    i = 0
    for assign in ("ls", "sr", "ms"):
        for ch in chans[assign]:
            for ok, bad in edges16:
                for back in ((0, 1) if assign != "ms" else (i % 2,)):
                    i += 1
                    decor_case(out, f"D_16_gen_{assign}_ch{ch}_{'hi' if ok > 0 else 'lo'}_b{back}", assign, 16, 64, ch, ok, bad, back,
                               i % 2, group="fast")
    # 16-bit generic path (a block's tail), 8-bit containers, and 32-bit samples (the WIDE forms)
    for tag, bps, bs, grp in (("16_tail", 16, 48, "gen"), ("8", 8, 64, "fast"), ("8_tail", 8, 48, "gen"), ("32", 32, 64, "fast"),
                              ("32_tail", 32, 48, "gen")):
        SB = craft.widths(bps)[0]
        hi, lo = (1 << (SB - 1)) - 1, -(1 << (SB - 1))
        for assign in ("ls", "sr", "ms"):
            for ch in chans[assign]:
                for ok, bad in ((hi, hi + 1), (lo, lo - 1)):
                    i += 1
                    decor_case(out, f"D_{tag}_{assign}_ch{ch}_{'hi' if ok > 0 else 'lo'}", assign, bps, bs, ch, ok, bad, 0, i % 2,
                               group=grp)
    # one mid/side lane with a wasted bit: D_GEN for its wave
    for ok, bad in edges16:
        decor_case(out, f"D_16_wasted_ms_ch0_{'hi' if ok > 0 else 'lo'}", "ms", 16, 64, 0, ok, bad, 0, 0, wasted_lane=True,
                   group="wasted")
    # 24-bit samples in their 32-bit container: the wrapping i32 form is exact, nothing traps ...
    for assign, x0, x1 in (("ls", (1 << 23) - 1, -(1 << 23)), ("sr", (1 << 23) - 1, (1 << 23) - 1), ("ms", -(1 << 23), (1 << 24) - 1)):
        subs = [Sub(kind="fixed", order=1, samples=ramp(64, 1, x0)), Sub(kind="fixed", order=1, samples=ramp(64, 1, x1))]
        out.append(make(f"D_24_{assign}_control_ok", 2, 24, 64, subs, assignment=assign, group="d24"))
    # ... until a predicted sample outside the depth, which zflac keeps, meets the container's edge
    hi = (1 << 31) - 1
    # (in waves of their own: beside a 31- or 32-bit lane the whole wave takes the WIDE form)
    for tag, bs, grp in (("", 64, "d24"), ("_tail", 48, "d24gen")):
        def builder(s, bs=bs):
            subs = [Sub(kind="fixed", order=1, samples=ramp(bs, 1, hi - 9, (hi,))),
                    Sub(kind="fixed", order=1, samples=ramp(bs, 1, 0, (s,)))]
            return (2, 24, bs, subs), dict(assignment="ls")
        ok_trap(out, f"D_24_ls_beyond_depth{tag}", builder, 0, -1, "decor", aim_ch=1, group=grp)
    return out


# ---- R: the raw reads -----------------------------------------------------------------------------
def family_R():
    out = []
    for bps in (8, 16):
        hi = (1 << (bps - 1)) - 1
        # a side channel's warm-up sample: one more bit than the container holds
        def warm(v, bps=bps):
            subs = [Sub(kind="fixed", order=1, samples=[0] * 32), Sub(kind="fixed", order=1, samples=[v] + [0] * 31)]
            return (2, bps, 32, subs), dict(assignment="ls", at=0)
        ok_trap(out, f"R_{bps}_side_warmup", warm, hi, hi + 1, "warmup", aim_ch=1, group="fast")
        # a verbatim side channel: in a MIX kernel's fast form and in a block's tail
        for bs, grp in ((64, "mix"), (48, "mixgen")):
            def verb(v, bps=bps, bs=bs):
                subs = [Sub(kind="fixed", order=1, samples=[0] * bs), Sub(kind="verbatim", samples=tail_block(bs, (v,)))]
                return (2, bps, bs, subs), dict(assignment="ls")
            ok_trap(out, f"R_{bps}_side_verbatim_{bs}", verb, hi, hi + 1, "verbatim", aim_ch=1, group=grp)
        # a constant side channel has the frame's depth: it cannot leave the SampleType, the
        # difference can
        def const(l, bps=bps, hi=hi):
            subs = [Sub(kind="fixed", order=1, samples=tail_block(64, (l,))), Sub(kind="const", samples=[hi])]
            return (2, bps, 64, subs), dict(assignment="ls")
        ok_trap(out, f"R_{bps}_side_const", const, -1, -2, "decor", aim_ch=1, group="mix")
    # the wasted-bits shift wraps a predicted sample silently; the @intCast before it does not
    for bs, grp in ((64, "fast"), (48, "gen")):
        def wasted(v, bs=bs):
            return (1, 16, bs, [Sub(kind="fixed", order=1, wasted=1, samples=tail_block(bs, (v,)))]), {}
        ok_trap(out, f"R_16_wasted_wraps_{bs}", wasted, 20000, 32768, "sample", group=grp)
        ok_trap(out, f"R_16_wasted_wraps_max_{bs}", wasted, 32767, 32768, "sample", group=grp)
    return out


# ---- P: which error wins --------------------------------------------------------------------------
def patch_type(data: bytes, bitpos: int, sub_type: int) -> bytes:
    """The 6 subframe type bits of the header at `bitpos` (after its zero bit) replaced."""
    b = bytearray(data)
    for j in range(6):
        at = bitpos + 1 + j
        bit = (sub_type >> (5 - j)) & 1
        b[at >> 3] = (b[at >> 3] & ~(0x80 >> (at & 7))) | (bit << (7 - (at & 7)))
    return bytes(b)


def family_P():
    out = []
    RESERVED = 0b000010

    def spike(v):  # a value trap at sample 40 of a block of 64, then down again
        return Sub(kind="fixed", order=1, samples=[0] * 40 + [v] + [0] * 23)

    # zflac reads every residual of a subframe before it predicts: a stream cut inside the
    # residuals that follow the trap is an EndOfStream
    for tag, v, err in (("ok", 32767, "OK"), ("trap", 32768, "OutOfDomain")):
        c = make(f"P_spike_{tag}", 1, 16, 64, [spike(v)], error=err, aim=None if err == "OK" else (1, 0, 40, "sample"), at=40,
                 group="p")
        out.append(c)
        cut = int(c.cr.layout[1][0].cpos[52]) >> 3
        assert int(c.cr.layout[1][0].cpos[41]) + int(c.cr.layout[1][0].clen[41]) <= 8 * cut
        out.append(dataclasses.replace(c, name=f"P_spike_{tag}_cut", error="EndOfStream", flac=c.cr.flac[:cut], group="pcut"))
    # a value trap in channel 0 comes before a reserved subframe type in channel 1 of its frame
    for tag, v, err in (("ok", 32767, "InvalidSubframeHeader"), ("trap", 32768, "OutOfDomain")):
        c = make(f"P_ch0_{tag}_ch1_reserved", 2, 16, 64, [spike(v), spike(5)], at=40, group="p2",
                 error=err, aim=None if tag == "ok" else (1, 0, 40, "sample"))
        c.flac = patch_type(c.cr.flac, c.cr.layout[1][1].start, RESERVED)
        out.append(c)
    out.append(make("P_stereo_plain_ok", 2, 16, 64, [spike(32767), spike(5)], at=40, group="p2"))
    # ... and a reserved type in frame 1 before a value trap in frame 2
    c = make("P_reserved_in_frame1_value_in_frame2", 1, 16, 64, [spike(7)], at=40, group="p", error="InvalidSubframeHeader")
    frames = [c.frames[0], c.frames[1], [coded(spike(32768), 64)]]
    cr = craft.write(1, 16, 64, frames)
    assert not craft.sync_frames(cr)
    out.append(dataclasses.replace(c, cr=cr, frames=frames, aim=(2, 0, 40, "sample"),
                                   flac=patch_type(cr.flac, cr.layout[1][0].start, RESERVED)))
    return out


@functools.lru_cache(maxsize=None)
def family(name: str) -> tuple:
    return tuple(globals()[f"family_{name}"]())


# ---- the batch ------------------------------------------------------------------------------------
def class_of(c: Case) -> tuple:
    return craft.widths(c.cr.bps)[0], c.cr.channels


@functools.lru_cache(maxsize=None)
def batch(name: str) -> tuple:
    """The family's cases in batch order: by class and group, every group padded to whole waves."""
    cases = list(family(name))
    keys = []
    for c in cases:
        k = class_of(c) + (c.group,)
        if k not in keys:
            keys.append(k)
    out = []
    for k in sorted(keys, key=lambda k: (k[0], k[1], keys.index(k))):
        grp = [c for c in cases if class_of(c) + (c.group,) == k]
        out += grp
        per = 64 // k[1]
        n = -sum(sum(off < len(c.data) for off in c.cr.frame_offsets) for c in grp) % per
        if n:
            out.append(pad_stream(f"{name}_pad_{k[0]}_{k[1]}_{k[2]}", max(grp, key=lambda c: c.cr.bs), n))
    return tuple(out)


def waves(cases) -> dict:
    """(case index, frame) -> the entries of its wave, as the decode kernels group a batch."""
    by_class = {}
    for i, c in enumerate(cases):
        n = sum(off < len(c.data) for off in c.cr.frame_offsets)  # (a cut stream has fewer frames)
        by_class.setdefault(class_of(c), []).extend((i, f) for f in range(n))
    out = {}
    for k, rows in by_class.items():
        per = 64 // k[1]
        for g in range(0, len(rows), per):
            for e in rows[g:g + per]:
                out[e] = rows[g:g + per]
    return out


def assert_paths(cases) -> dict:
    """Every case's edge chunk takes the path the case names, in the wave the batch gives it.
    Returns how many cases sit on each path."""
    wv = waves(cases)
    seen = {}
    for i, c in enumerate(cases):
        if c.path == "pad":
            continue
        cr, ci = c.cr, c.at // craft.CHUNK
        infos = [craft.chunks(cr, 1, ch)[ci] for ch in range(cr.channels)]
        if c.path == "generic":
            assert any(not x.fast for x in infos), (c.name, infos)
            assert all(cr.layout[1][ch].unsafe == (x.why == "unsafe coefficients") for ch, x in enumerate(infos)), c.name
            if cr.bs == 48:
                assert ci == 1 and all(x.why == ("short or wide" if x.mix else "block tail") for x in infos), c.name
        else:
            assert (ci == 0 and cr.bs == 32) if c.path == "warm" else (ci >= 1 and 32 * ci + 32 <= cr.bs), (c.name, ci)
            mates = [(cases[j], f, ch, craft.chunks(cases[j].cr, f, ch)) for j, f in wv[(i, 1)]
                     for ch in range(cases[j].cr.channels)]
            live = [(o, f, ch, xs[ci]) for o, f, ch, xs in mates if ci < len(xs)]
            # two codes per step: 16-bit containers, past the first chunk, every lane's k in 2..PAIR_KMAX
            pairs = class_of(c)[0] == 16 and ci > 0 and all(x.mix or 2 <= x.k <= craft.PAIR_KMAX for _, _, _, x in live)
            for o, f, ch, x in live:
                assert x.fast and x.base == 32 * ci, (c.name, o.name, f, ch, x)
                assert (x.pair_max if pairs else x.longest) <= 32, (c.name, o.name, f, ch, x)
            for j, f in wv[(i, 1)]:
                o = cases[j]
                if c.group == "d24":  # no 31- or 32-bit lane: the wave stays off the WIDE forms
                    assert o.cr.bps <= 30, (c.name, o.name)
                if c.pure_ms:
                    assert o.cr.assignment == "ms" and o.cr.bps == 16 and not o.cr.mix, (c.name, o.name)
                    assert all(s.wasted == 0 for s in o.frames[f]), (c.name, o.name)
        seen[c.path] = seen.get(c.path, 0) + 1
    return seen
