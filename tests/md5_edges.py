"""Streams whose MD5 message sits on the exact byte counts at which the device hash (md5.hip)
changes what it does, built with tests/craft.py: one mono channel of VERBATIM subframes of chosen
samples, so the message length is L = channels x block size x frames x width.

The hash of a stream is a unit loop (hash_units / hash_units_coop: whole units of U = 256 message
bytes, 192 for 24-bit samples, double-buffered) followed by md5_tail (the remaining r bytes, 0x80,
zero fill and the bit length: one block while L mod 64 <= 55, two from 56 on). A case names its
form (the (mode, justify) forms of md5_job, RAW split by width, MD5_S24 by whether the shift is whole bytes), its depth, and L; from L
follow nu = L // U (units: 0 is the tail alone, 1 the loop's exit without a reload, 2 the reload,
3 and 4 the odd and even exits after a full turn) and r = L mod 64.

Per depth:
  * tail edges: for every nu in 0..4, a stream for each tail residue of TAILS (the residues the
    sample width allows nearest 55 | 56, the largest below 64, and 0);
  * unit edges: L = kU - w, kU, kU + w for k = 1..4 (an empty, a one-sample and a nearly full
    tail around every unit count), and one L < U.

Samples are seeded and uniform over the whole depth; every stream holds edge_pattern() at both
ends (the depth's minimum, maximum, -1, 0; in a 16-bit container a negative sample in the low
half of a dword beside a positive one in the high half, and the reverse), so that both the unit
loop's packed words and the tail's bytes meet them.

`shape_*` order those streams into the batches the GPU tests run (lists of the streams above;
`planted()` alone adds streams, for the sequential planner). `job_waves` restates how the host
orders jobs (longest_first, md5_host.cpp) and how the kernels split them into waves of 64.
A builder module like rice_edges.py: tests/test_md5_edges.py holds the assertions."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from . import craft
from .craft import Sub

# form -> (depths, message bytes per sample, message bytes per unit)
FORMS = {
    "raw8": ((8,), 1, 256),
    "raw16": ((16,), 2, 256),
    "raw32": ((32,), 4, 256),
    "s16": ((9, 15), 2, 256),      # MD5_S16_SHIFT: the frame header's depth code is 0 (from STREAMINFO)
    "s32": ((25, 31), 4, 256),     # MD5_S32_SHIFT
    "s24": ((24,), 3, 192),        # MD5_S24, js = 8: the shift of whole bytes (zflac left-justifies 24-bit
                                   # samples in their 32-bit container too, so MD5_S24 has no js = 0 form)
    "s24js": ((17, 20), 3, 192),   # MD5_S24, js = 15 and 12: bits of the sample's low byte cross into the shift
}
MODE_OF = {"raw8": 0, "raw16": 0, "raw32": 0, "s16": 1, "s32": 2, "s24": 3, "s24js": 3}  # Md5Mode (common.h)
DEPTHS = tuple((form, bps) for form, (depths, _, _) in FORMS.items() for bps in depths)
# L mod 64 at the tail's edges, per message bytes of a sample: the largest residue that leaves one
# tail block, the smallest that takes two, the largest at all, and none. (Three-byte samples reach
# every residue; 54 and 57 are the multiples of three beside the edge.)
TAILS = {1: (55, 56, 63, 0), 2: (54, 56, 62, 0), 3: (54, 55, 56, 57, 63, 0), 4: (52, 56, 60, 0)}
NUS = (0, 1, 2, 3, 4)
MIN_SAMPLES = 16  # craft's (and FLAC's) smallest block


def justify_of(bps: int) -> int:
    return 16 - bps if 9 <= bps <= 15 else 32 - bps if 17 <= bps <= 31 else 0


def form_of(bps: int) -> str:
    return next(f for f, b in DEPTHS if b == bps)


def geometry(channels: int, bs: int, frames: int, bps: int) -> tuple:
    """(L, r, nu) of a stream, from its shape and depth alone."""
    _, w, U = FORMS[form_of(bps)]
    assert w == (bps + 7) // 8
    L = channels * bs * frames * w
    return L, L % 64, L // U


def feasible(w: int, U: int, nu: int, r: int) -> list:
    """Every L of width w with nu units and L mod 64 == r that a block of >= 16 samples can make."""
    return [L for L in range(nu * U, (nu + 1) * U) if L % 64 == r and L % w == 0 and L // w >= MIN_SAMPLES]


def lengths(form: str) -> dict:
    """L -> kind ("tail", "unit" or "small") of the form's streams."""
    _, w, U = FORMS[form]
    out = {}
    for nu in NUS:
        for ri, r in enumerate(TAILS[w]):
            fits = feasible(w, U, nu, r)
            if fits:  # (no L: 24-bit samples, nu = 0, r = 0, whose only length is 0)
                out.setdefault(fits[(nu + ri) % len(fits)], "tail")
    for k in (1, 2, 3, 4):
        for L in (k * U - w, k * U, k * U + w):
            out.setdefault(L, "unit")
    out.setdefault(U - 40 * w, "small")
    assert all(L % w == 0 and L // w >= MIN_SAMPLES for L in out)
    return out


def edge_pattern(bps: int, variant: int = 0) -> list:
    """Eight samples from an even index: the depth's minimum, maximum, -1 and 0, with a negative
    sample in the low half of a dword beside a positive one in the high half, and the reverse.
    Two orders: a run of 13 one bits or more (the maximum, -1) followed by two zero bits is a
    frame sync code when it falls byte-aligned, and where it falls depends on the depth alone, not
    on the seed; in the second order nothing that begins with zero bits follows such a run."""
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    return [[lo, hi, 1, -1, 0, -1, -1, hi], [0, 0, 1, lo, lo, hi, -1, hi]][variant % 2]


def samples_of(bps: int, n: int, seed, variant: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    s = rng.integers(lo, hi + 1, n, dtype=np.int64)
    pat = edge_pattern(bps, variant)
    s[:len(pat)] = pat
    s[n - len(pat) - (n - len(pat)) % 2:][:len(pat)] = pat  # (from an even index: the same dword halves)
    return s


def split(n: int) -> tuple:
    """(block size, frames) of n samples: two blocks where both can have 16 samples."""
    return (n // 2, 2) if n % 2 == 0 and n // 2 >= MIN_SAMPLES else (n, 1)


@dataclasses.dataclass
class Case:
    name: str
    form: str
    bps: int
    L: int
    kind: str
    cr: craft.Crafted
    planted: bool = False

    @property
    def data(self) -> bytes:
        return self.cr.flac

    @property
    def r(self) -> int:
        return self.L % 64

    @property
    def nu(self) -> int:
        return self.L // FORMS[self.form][2]


def _write(bps: int, n: int, tag: int, plant: bool = False) -> craft.Crafted:
    """n verbatim samples; the first seed whose stream holds no byte-aligned sync pattern off its
    frame starts (`plant`: but for the copy of the first frame's header inside that frame)."""
    bs, frames = split(n)
    for salt in range(200):
        s = samples_of(bps, n, [bps, n, tag, salt], salt)
        subs = [[Sub(kind="verbatim", samples=s[f * bs:(f + 1) * bs])] for f in range(frames)]
        cr = craft.write(1, bps, bs, subs)
        if plant:
            cr = _plant(cr, bps, bs, s, subs)
            if craft.sync_frames(cr) == [0] and len(craft.sync_positions(cr, 0)) == 1:
                return cr
        elif not craft.sync_frames(cr):
            return cr
    raise AssertionError(f"no seed gives a sync-free stream of {n} {bps}-bit samples")


def _plant(cr, bps, bs, s, subs):
    """The stream again with the first frame's own header, CRC-8 included, as the samples in the
    middle of that frame (16-bit verbatim samples are byte-aligned): a frame start to the
    device's frame search, off the chain. (Not the last frame: the chain check does not look at
    candidates past the STREAMINFO total, so it rules that one out by itself.)"""
    assert bps == 16 and len(subs) == 2
    f = 0
    off = cr.frame_offsets[f]
    hdr = cr.flac[off:off + 7]  # sync, block size and rate, channels and depth, frame number, block size, CRC-8
    assert hdr[:2] == b"\xff\xf8" and cr.layout[f][0].start == 8 * (off + 7) and cr.layout[f][0].cpos[0] == 8 * (off + 8)
    words = np.frombuffer(hdr + b"\x55", ">i2").astype(np.int64)
    s = s.copy()
    at = f * bs + (bs // 2 | 1) + 1  # an even sample of the frame, past the edge pattern
    s[at:at + 4] = words
    subs = [[Sub(kind="verbatim", samples=s[g * bs:(g + 1) * bs])] for g in range(len(subs))]
    out = craft.write(1, bps, bs, subs)
    assert out.flac[:42 - 16] == cr.flac[:42 - 16] and hdr in out.flac[off + 8:]
    return out


@functools.lru_cache(maxsize=None)
def cases(bps: int) -> tuple:
    """The depth's streams, shortest first."""
    form = form_of(bps)
    _, w, _ = FORMS[form]
    out = []
    for L, kind in sorted(lengths(form).items()):
        c = Case("", form, bps, L, kind, _write(bps, L // w, 0))
        c.name = f"{form}_{bps}_{kind}_L{L}_r{c.r}_nu{c.nu}"
        out.append(c)
    return tuple(out)


def all_cases() -> tuple:
    return tuple(c for _, bps in DEPTHS for c in cases(bps))


@functools.lru_cache(maxsize=None)
def planted() -> tuple:
    """16-bit streams with a planted frame header, one per unit count 0..3 and at the tail's edges:
    the chain check refuses them, the sequential planner decodes them, and the synchronous hash
    launch takes their digests."""
    out = []
    # (two blocks, so an even sample count, of at most 256 samples each: a seven-byte header)
    for L in (64 + 56, 256 + 60, 512, 3 * 256 + 56):
        c = Case("", "raw16", 16, L, "planted", _write(16, L // 2, 1, plant=True), planted=True)
        c.name = f"raw16_16_planted_L{L}_r{c.r}_nu{c.nu}"
        out.append(c)
    return tuple(out)


# ---- the batches ------------------------------------------------------------------------------
MD5_WG_WAVES = 4  # ZFLAC_MD5_WG_WAVES' default: waves of a k_md5_coop workgroup


def job_waves(Ls) -> list:
    """The waves of a hash launch over jobs of these message lengths, in batch order: the host
    sorts them longest first (stable) and lane t of the launch takes job t. A list of lists of
    indices into Ls."""
    order = sorted(range(len(Ls)), key=lambda i: -Ls[i])
    return [order[i:i + 64] for i in range(0, len(order), 64)]


def shape_a(bps: int) -> list:
    """Every stream of the depth, with more copies of the longest (nu = 4) and the shortest
    (nu = 0) ones: 70 jobs or more, whose first wave holds nu = 4 lanes beside nu = 0 lanes and
    whose last wave is partial."""
    cs = list(cases(bps))
    top = [c for c in cs if c.nu == 4]
    low = [c for c in cs if c.nu == 0]
    out = cs + top * 3 + low * 4
    return out + low * (0 if len(out) >= 72 else 1)


def shape_b(bps: int) -> list:
    """Every stream of the depth once, then the tail-only ones (nu = 0) again and again: more
    jobs than one workgroup of k_md5_coop has lanes, so a second workgroup and a partial last wave."""
    cs = list(cases(bps))
    low = [c for c in cs if c.nu == 0]
    want = 64 * MD5_WG_WAVES + 5
    return cs + [low[i % len(low)] for i in range(want - len(cs))]


def shape_c() -> list:
    """The 16-bit streams with the planted ones spread among them (the test adds a malformed
    stream of tests/malformed.py: it comes from synth)."""
    cs = list(cases(16))
    for i, p in enumerate(planted()):
        cs.insert(5 + 7 * i, p)
    return cs


D_PAIRS = ((8, 9), (16, 25), (32, 24), (15, 17), (31, 20))  # every depth once, two forms per batch


def shape_d(pair) -> list:
    """Two depths of different forms in one batch: no common mode, so k_md5_multi."""
    a, b = cases(pair[0]), cases(pair[1])
    assert MODE_OF[a[0].form] != MODE_OF[b[0].form]
    out = []
    for x, y in zip(a, b):  # interleaved (the lists differ in length by a few)
        out += [x, y]
    return out + list(a[len(b):]) + list(b[len(a):])


def shape_e(bps: int) -> list:
    """Every stream of the depth: run with lane loads forced."""
    return list(cases(bps))
