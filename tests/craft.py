"""A residual-level FLAC stream writer and a CPU model of the decode kernels' chunk loop.

`write()` takes the coded representation itself: per frame and channel a `Sub` that names the
subframe type, its wasted bits, the residual coding method, the partition order, one Rice
parameter or escape width per partition and the residuals (or the channel's samples, from which
the residuals follow). It is independent of synth/flacgen.cpp and of the oracle. It returns a
`Crafted`: the bytes, the expected interleaved PCM as exact integers, the frame offsets and a
layout with the bit position and length of every code, per frame, channel and sample.

What the writer writes follows the reader it is aimed at (src/zflac.zig), quirks included:
a CONSTANT subframe's value has the frame's bits per sample even on a side channel, and the
side channel of L/S, S/R and M/S frames is one bit wider everywhere else.

Two things to know when building cases:
  * The escape width field has 5 bits, so a width of 32 cannot be written.
  * With FIXED order >= 1 (or LPC), free-running residuals integrate out of the SampleType
    within a block and the reader answers OutOfDomain. Build such subframes from `samples`:
    a bounded signal, differenced by the writer. Order 0 (residual = sample) is the workhorse.

The precondition model (`chunks`, `simulate_wave`, `segments`) works from the layout alone. It
restates the conditions under which zflac_amd/csrc/decode/run_subframe.h takes a chunk of 32
samples on the fast path (`lane_fast`), which form it picks, and what sends the wave back to
the generic path: a code longer than the 32-bit peek (NC = 1), an aligned pair of codes longer
than 32 bits together (NC = 2), a lane that is not fast. Whether the lane's ring ran dry is
outside the model (it depends on where the stream lies in device memory); the model reports
the bits each chunk reads, and cases argue from bounds: the ring of an 8- or 16-bit container
holds 64 words (RING_BITS; 128 for 32-bit containers), and a top-up adds 16 words (24 for 32-bit
containers) per chunk at the most.
"""
from __future__ import annotations

import dataclasses
import hashlib

import numpy as np

CHUNK = 32
PAIR_KMAX = 9
RING_BITS = 64 * 32
FIXED_COEFS = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}
ASSIGN = {"indep": None, "ls": 8, "sr": 9, "ms": 10}
_DEPTH_CODE = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


def widths(bps: int):
    """(SampleType bits, InterType bits) of the container of a `bps`-bit stream."""
    return {8: (8, 16), 16: (16, 32), 24: (32, 64), 32: (32, 64)}[(bps + 7) // 8 * 8]


@dataclasses.dataclass
class Sub:
    """One subframe. `kind`: "const", "verbatim", "fixed" or "lpc".
    fixed / lpc: give `samples` (the channel's block before the wasted-bits shift; the writer
    differences it) or `residuals` (bs - order of them) with `warmup` (order samples).
    `coefs` (lpc) in bitstream order: coefs[0] multiplies the previous sample.
    `params`: one per partition, ("k", rice parameter) or ("e", escape width 0..31).
    `raw`: residual index -> (quotient, remainder): that code is written as given, whatever it
    decodes to (quotients that the reader's `<<` discards, or that leave its integer type)."""
    kind: str = "fixed"
    order: int = 0
    coefs: tuple = ()
    precision: int = 0
    shift: int = 0
    wasted: int = 0
    method: int = 0
    porder: int = 0
    params: tuple = (("k", 0),)
    samples: object = None
    residuals: object = None
    warmup: tuple = ()
    raw: dict = None


@dataclasses.dataclass
class SubLayout:
    kind: str
    order: int
    bs: int
    start: int          # bit position of the subframe header in the stream
    end: int            # bit position after the subframe's last bit
    cpos: np.ndarray    # [bs] bit position of sample i's code (warm-up / verbatim: its raw bits)
    clen: np.ndarray    # [bs] length of sample i's code (0 for a CONSTANT subframe's samples)
    part: np.ndarray    # [bs] partition of sample i, -1 for warm-up and non-residual samples
    pk: tuple           # per partition: rice parameter, or -1 for an escape partition
    pesc: tuple         # per partition: escape width, or -1
    pstart: tuple       # per partition: first sample, and one past the last at the end
    phdr: tuple         # per partition: bit position of its header
    method: int
    cbps: int           # bits of a warm-up / verbatim sample
    unsafe: bool        # LPC coefficients large enough for the kernels' generic path


@dataclasses.dataclass
class Crafted:
    flac: bytes
    pcm: list                 # interleaved, un-justified, exact Python integers
    frame_offsets: list
    layout: list              # [frame][channel] -> SubLayout
    channels: int
    bps: int
    bs: int
    assignment: str
    max_order: int
    mix: bool

    @property
    def pcm_array(self) -> np.ndarray:
        return np.asarray(self.pcm, dtype=np.int64)

    @property
    def md5(self) -> bytes:
        return self.flac[26:42]

    def justified(self) -> np.ndarray:
        """The PCM as zflac hands it out: left-justified in its container (src/zflac.zig:287-306)."""
        b = self.bps
        js = 16 - b if 9 <= b <= 15 else 32 - b if 17 <= b <= 31 else 0
        return (self.pcm_array << js).astype({8: np.int8, 16: np.int16, 32: np.int32}[widths(b)[0]])

    def frame_bytes(self, f: int) -> bytes:
        o = self.frame_offsets + [len(self.flac)]
        return self.flac[o[f]:o[f + 1]]


# ---- bit fields -------------------------------------------------------------------------------
class _Fields:
    """(value, bit count) fields of a whole stream, packed MSB first in one vectorised pass.
    A value is below 2**64 and below 2**count; the count itself is unbounded (long zero runs)."""

    def __init__(self):
        self.v, self.n, self.count, self.bits = [], [], 0, 0

    def add(self, vals, nbits) -> int:
        """Append fields; returns the index of the first."""
        vals = np.atleast_1d(np.asarray(vals, dtype=np.uint64))
        nbits = np.broadcast_to(np.atleast_1d(np.asarray(nbits, dtype=np.int64)), vals.shape)
        first = self.count
        self.v.append(vals)
        self.n.append(nbits)
        self.count += vals.size
        self.bits += int(nbits.sum())
        return first

    def pack(self):
        v = np.concatenate(self.v) if self.v else np.zeros(0, np.uint64)
        n = np.concatenate(self.n) if self.n else np.zeros(0, np.int64)
        end = np.cumsum(n)
        assert end.size == 0 or end[-1] % 8 == 0
        bits = np.zeros(int(end[-1]) if end.size else 0, np.uint8)
        live = v != 0
        vv, ee = v[live], end[live]
        b = 0
        while vv.size:
            one = (vv & np.uint64(1)) != 0
            bits[ee[one] - 1 - b] = 1
            vv = vv >> np.uint64(1)
            keep = vv != 0
            vv, ee = vv[keep], ee[keep]
            b += 1
        return np.packbits(bits), end - n


def _crc_table(poly: int, width: int):
    t = np.zeros(256, np.uint32)
    top, mask = 1 << (width - 1), (1 << width) - 1
    for i in range(256):
        c = i << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) if c & top else (c << 1)
        t[i] = c & mask
    return t


_CRC8, _CRC16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def _crc_rows(buf: np.ndarray, starts, ends, table, width: int) -> np.ndarray:
    """CRC (MSB first, initial value 0) of buf[starts[i]:ends[i]] for every i, all rows a byte at a time."""
    starts, ends = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    order = np.argsort(-(ends - starts), kind="stable")  # longest first: the live rows are a prefix
    s, length = starts[order], (ends - starts)[order]
    crc = np.zeros(s.size, np.uint32)
    mask, sh = np.uint32((1 << width) - 1), np.uint32(width - 8)
    live = s.size
    j = 0
    while live and j < int(length[0]):
        while live and length[live - 1] <= j:
            live -= 1
        if live <= 2:  # a few rows far longer than the rest (a 2 MiB frame): plain integers from here
            tab, m, k = table.tolist(), int(mask), int(sh)
            for i in range(live):
                c = int(crc[i])
                for b in buf[int(s[i]) + j:int(s[i]) + int(length[i])].tolist():
                    c = ((c << 8) & m) ^ tab[((c >> k) ^ b) & 0xFF]
                crc[i] = c
            break
        c = crc[:live]
        crc[:live] = ((c << np.uint32(8)) & mask) ^ table[((c >> sh) ^ buf[s[:live] + j]) & np.uint32(0xFF)]
        j += 1
    out = np.zeros(s.size, np.uint32)
    out[order] = crc
    return out


def _utf8(n: int) -> list:
    if n < 0x80:
        return [n]
    out, lead, cap = [], 0xC0, 0x20
    while True:
        out.append(0x80 | (n & 0x3F))
        n >>= 6
        if n < cap:
            return [lead | n] + out[::-1]
        lead, cap = (lead >> 1) | 0x80, cap >> 1


RATE_TABLE = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000,
              11: 96000}
_BS_TABLE = {192: 1, **{576 << k: 2 + k for k in range(4)}, **{1 << k: k for k in range(8, 16)}}


def _bs_code(bs: int, bs_field):
    """(block-size code, the bytes of its field) of a frame of `bs` samples."""
    if bs_field == "table" and bs in _BS_TABLE:
        return _BS_TABLE[bs], []
    if bs_field == 8 or bs_field == "table" and bs <= 256:
        assert bs <= 256
        return 6, [bs - 1]
    return 7, [(bs - 1) >> 8, (bs - 1) & 0xFF]


def _zigzag(r: np.ndarray) -> np.ndarray:
    r = np.asarray(r, dtype=np.int64)
    return np.where(r >= 0, r << 1, ((-r) << 1) - 1).astype(np.uint64)


def decoded_raw(q: int, rem: int, k: int, W: int) -> int:
    """What zflac makes of quotient q and remainder rem: `q << k` discards in the W-bit
    unsigned residual type (src/zflac.zig:657-663)."""
    mask = (1 << W) - 1
    zz = ((q << k) & mask) + rem
    u = ((zz >> 1) ^ (-(zz & 1))) & mask
    return u - (1 << W) if u >> (W - 1) else u


def _predict(hist, coefs, shift) -> int:
    return sum(c * s for c, s in zip(coefs, reversed(hist[-len(coefs):]))) >> shift if coefs else 0


def _sub_values(sub: Sub, bs: int, W: int):
    """(samples before the wasted shift, residuals) of a fixed / lpc subframe, as int64 arrays."""
    o = sub.order
    coefs = FIXED_COEFS[o] if sub.kind == "fixed" else tuple(sub.coefs)
    assert len(coefs) == o
    if sub.samples is not None:
        assert sub.residuals is None and not sub.raw
        s = np.asarray(sub.samples, dtype=np.int64)
        assert s.size == bs
        pred = np.zeros(bs - o, np.int64)
        for j, c in enumerate(coefs):
            pred += c * s[o - 1 - j:bs - 1 - j]
        return s, s[o:] - (pred >> sub.shift)
    r = np.array(sub.residuals, dtype=np.int64)
    assert r.size == bs - o and len(sub.warmup) == o
    for i, (q, rem) in (sub.raw or {}).items():
        r[i] = decoded_raw(q, rem, _param_of(sub, bs, i), W)
    if o == 0:
        return r.copy(), r
    s = [int(x) for x in sub.warmup]
    for x in r.tolist():
        s.append(x + _predict(s, coefs, sub.shift))
    return np.asarray(s, dtype=np.int64), r


def _part_bounds(sub: Sub, bs: int):
    n = 1 << sub.porder
    assert bs % n == 0 and bs // n >= sub.order and len(sub.params) == n, (bs, sub.porder, len(sub.params))
    ps = bs // n
    return [max(p * ps, sub.order) for p in range(n)] + [bs]


def _param_of(sub: Sub, bs: int, ri: int) -> int:
    b = _part_bounds(sub, bs)
    p = next(p for p in range(len(b) - 1) if b[p] <= ri + sub.order < b[p + 1])
    assert sub.params[p][0] == "k"
    return sub.params[p][1]


def _signed_field(v: np.ndarray, n: int) -> np.ndarray:
    v = np.asarray(v, dtype=np.int64)
    assert n == 0 and not v.any() or n and (v >= -(1 << (n - 1))).all() and (v < (1 << (n - 1))).all(), (n, v.min(), v.max())
    return (v & np.int64((1 << n) - 1 if n < 64 else -1)).astype(np.uint64)


def _write_sub(F: _Fields, sub: Sub, bs: int, bps: int, ubps: int, W: int):
    """Append one subframe's fields; returns (channel values after the wasted shift, a
    SubLayout whose positions are still field indices)."""
    SB = widths(bps)[0]
    w = sub.wasted
    type_code = {"const": 0, "verbatim": 1, "fixed": 8 + sub.order, "lpc": 31 + sub.order}[sub.kind]
    first = F.add([type_code << 1 | (1 if w else 0)], 8)
    if w:
        F.add([1], w)
    cbps = ubps - w
    n = np.zeros(bs, np.int64)
    idx = np.full(bs, -1, np.int64)
    part = np.full(bs, -1, np.int64)
    lay = dict(kind=sub.kind, order=sub.order, bs=bs, pk=(), pesc=(), pstart=(), phdr=(), method=sub.method,
               cbps=cbps, unsafe=False)
    if sub.kind == "const":
        v = int(np.asarray(sub.samples).reshape(-1)[0])
        F.add(_signed_field([v], bps - w), bps - w)  # the frame's depth, also on a side channel
        vals = np.full(bs, v, np.int64)
    elif sub.kind == "verbatim":
        vals = np.asarray(sub.samples, dtype=np.int64)
        assert vals.size == bs
        i0 = F.add(_signed_field(vals, cbps), cbps)
        idx, n = i0 + np.arange(bs), np.full(bs, cbps, np.int64)
    else:
        assert sub.kind in ("fixed", "lpc") and (sub.kind == "lpc" or sub.order <= 4)
        vals, res = _sub_values(sub, bs, W)
        o = sub.order
        if o:
            i0 = F.add(_signed_field(vals[:o], cbps), cbps)
            idx[:o], n[:o] = i0 + np.arange(o), cbps
        if sub.kind == "lpc":
            assert 1 <= sub.precision <= 15 and 1 <= o <= 32
            F.add([sub.precision - 1, sub.shift], [4, 5])
            F.add(_signed_field(sub.coefs, sub.precision), sub.precision)
            lay["unsafe"] = (sum(abs(int(c)) for c in sub.coefs) << (SB - 1)) > {8: 0x7FFF, 16: 1 << 30}.get(SB, 1 << 200)
        F.add([sub.method, sub.porder], [2, 4])
        bounds = _part_bounds(sub, bs)
        pk, pesc, phdr = [], [], []
        kmax, escape, kbits = (30, 31, 5) if sub.method else (14, 15, 4)
        for p, (what, val) in enumerate(sub.params):
            a, b = bounds[p], bounds[p + 1]
            r = res[a - o:b - o]
            part[a:b] = p
            if what == "k":
                assert 0 <= val <= kmax
                phdr.append(F.add([val], kbits))
                zz = _zigzag(r)
                q = (zz >> np.uint64(val)).astype(np.int64)
                v = (np.uint64(1) << np.uint64(val)) | (zz & np.uint64((1 << val) - 1))
                for i, (rq, rrem) in (sub.raw or {}).items():
                    if a <= i + o < b:
                        assert 0 <= rrem < (1 << val)
                        q[i + o - a], v[i + o - a] = rq, (1 << val) | rrem
                i0 = F.add(v, q + 1 + val)
                pk.append(val)
                pesc.append(-1)
                n[a:b] = q + 1 + val
            else:
                assert what == "e" and 0 <= val <= 31
                phdr.append(F.add([escape, val], [kbits, 5]))
                i0 = F.add(_signed_field(r, val), val)
                pk.append(-1)
                pesc.append(val)
                n[a:b] = val
            idx[a:b] = i0 + np.arange(b - a)
        lay.update(pk=tuple(pk), pesc=tuple(pesc), pstart=tuple(bounds), phdr=tuple(phdr))
    lay.update(start=first, end=F.count, cpos=idx, clen=n, part=part)
    return vals << w, lay


def write(channels: int, bps: int, bs: int, frames, assignment: str = "indep", rate: int = 44100,
          bs_field: int | str | None = None, *, rate_code: int | None = None, blocking: str = "fixed",
          first_number: int = 0, block_sizes=None) -> Crafted:
    """`frames`: one list of `channels` Subs per frame, every frame `bs` samples (fixed blocking,
    frame numbers from 0). `assignment`: "indep", or for two channels "ls", "sr", "ms": the Subs
    are then the coded channels (left/side, side/right, mid/side). `bs_field`: 8 or 16, the
    width of the header's block-size field (default: 8 bits where the block size allows; a
    block of 256 then puts an FF byte in front of the CRC-8), or "table": the codes 1..5 and
    8..15 where a frame's block size is 192, 576 << k or 1 << k, a field of 8 or 16 bits elsewhere.

    The other header forms (the defaults write what the writer always wrote):
    `rate_code`: any of 0..14 (default 9 for 44,100 Hz, else 0); 1..11 want `rate` to be the
    table's, 12 writes it in 8 bits (in Hz: what zflac reads, src/zflac.zig:369), 13 in 16 bits,
    14 in tens of Hz in 16 bits. STREAMINFO holds `rate` itself.
    `blocking`: "variable" writes 0xF9 and numbers every frame by its first sample.
    `first_number`: the first frame's coded number (the frame number, or the first sample's).
    `block_sizes`: the block size of every frame (default: `bs` each). STREAMINFO's minimum and
    maximum are `bs` where every frame but the last has `bs` samples under fixed blocking, and
    the frames' own extremes elsewhere."""
    assert 1 <= channels <= 8 and 4 <= bps <= 32 and 16 <= bs <= 65535
    sizes_ = [bs] * len(frames) if block_sizes is None else [int(x) for x in block_sizes]
    assert len(sizes_) == len(frames) and all(16 <= x <= 65535 for x in sizes_[:-1]) and 1 <= sizes_[-1] <= 65535
    assert blocking in ("fixed", "variable")
    if bs_field != "table":
        bs_field = bs_field or (8 if max(sizes_) <= 256 else 16)
        assert bs_field == 16 or max(sizes_) <= 256
    rc = rate_code if rate_code is not None else (9 if rate == 44100 else 0)
    assert 0 <= rc <= 14 and 0 < rate < 1 << 20
    if 1 <= rc <= 11:
        assert rate == RATE_TABLE[rc]
    rate_bytes = {12: [rate], 13: [rate >> 8, rate & 0xFF], 14: [rate // 10 >> 8, rate // 10 & 0xFF]}.get(rc, [])
    assert all(0 <= x < 256 for x in rate_bytes) and (rc != 14 or rate % 10 == 0)
    code = ASSIGN[assignment]
    assert code is None or channels == 2
    SB, W = widths(bps)
    F = _Fields()
    marks, pcm, layout = [], [], []
    max_order, mix = 0, False
    number = first_number
    for f, subs in enumerate(frames):
        assert len(subs) == channels
        fbs = sizes_[f]
        bcode, bs_bytes = _bs_code(fbs, bs_field)
        hdr = [0xFF, 0xF8 if blocking == "fixed" else 0xF9, bcode << 4 | rc,
               (channels - 1 if code is None else code) << 4 | _DEPTH_CODE.get(bps, 0) << 1] + _utf8(number)
        hdr += bs_bytes + rate_bytes
        number += 1 if blocking == "fixed" else fbs
        assert F.bits % 8 == 0
        start_byte = F.bits // 8
        F.add(hdr + [0], 8)
        chans, lays = [], []
        for c, sub in enumerate(subs):
            side = code is not None and c == (0 if code == 9 else 1)
            vals, lay = _write_sub(F, sub, fbs, bps, bps + (1 if side else 0), W)
            chans.append(vals)
            lays.append(lay)
            if sub.kind in ("const", "verbatim"):
                mix = True
            else:
                max_order = max(max_order, sub.order)
        F.add([0, 0], [-F.bits % 8, 16])
        marks.append((start_byte, len(hdr), F.bits // 8))
        if code == 8:
            chans = [chans[0], chans[0] - chans[1]]
        elif code == 9:
            chans = [chans[0] + chans[1], chans[1]]
        elif code == 10:
            mid = (chans[0] << 1) | (chans[1] & 1)
            chans = [(mid + chans[1]) >> 1, (mid - chans[1]) >> 1]
        pcm.append(np.stack(chans, axis=1).reshape(-1))
        layout.append(lays)
    body, pos = F.pack()
    starts = np.array([m[0] for m in marks], np.int64)
    hlen = np.array([m[1] for m in marks], np.int64)
    ends = np.array([m[2] for m in marks], np.int64)
    body[starts + hlen] = _crc_rows(body, starts, starts + hlen, _CRC8, 8).astype(np.uint8)
    crc = _crc_rows(body, starts, ends - 2, _CRC16, 16)
    body[ends - 2], body[ends - 1] = (crc >> 8).astype(np.uint8), (crc & 0xFF).astype(np.uint8)
    pcm = np.concatenate(pcm)
    cont = ((pcm + (1 << (SB - 1))) & ((1 << SB) - 1)) - (1 << (SB - 1))  # as the container holds it
    nbytes = (bps + 7) // 8
    msg = cont.astype("<i8").view(np.uint8).reshape(-1, 8)[:, :nbytes]
    total = sum(sizes_)
    sizes = ends - starts
    nominal = blocking == "fixed" and all(x == bs for x in sizes_[:-1]) and sizes_[-1] <= bs
    min_bs, max_bs = (bs, bs) if nominal else (min(sizes_), max(sizes_))
    si = _Fields()
    si.add([min_bs, max_bs, int(sizes.min()), int(sizes.max()), rate, channels - 1, bps - 1, total], [16, 16, 24, 24, 20, 3, 5, 36])
    digest = hashlib.md5(np.ascontiguousarray(msg).tobytes()).digest()
    meta = b"fLaC" + bytes([0x80, 0, 0, 34]) + si.pack()[0].tobytes() + digest
    base = len(meta) * 8
    pos = np.concatenate([pos, [F.bits]]) + base
    out_layout = []
    for lays in layout:
        row = []
        for lay in lays:
            lay["cpos"] = np.where(lay["cpos"] >= 0, pos[np.maximum(lay["cpos"], 0)], -1)
            lay["start"], lay["end"] = int(pos[lay["start"]]), int(pos[lay["end"]])
            lay["phdr"] = tuple(int(pos[i]) for i in lay["phdr"])
            row.append(SubLayout(**lay))
        out_layout.append(row)
    return Crafted(meta + body.tobytes(), pcm.tolist(), [len(meta) + int(s) for s in starts], out_layout, channels, bps,
                   bs, assignment, max_order, mix)


def sync_positions(cr: Crafted, f: int) -> list:
    """Offsets inside frame f, past its own sync code, of a byte-aligned frame sync pattern
    (FF F8 / FF F9): the device frame scan would take each for a candidate header."""
    b = np.frombuffer(cr.frame_bytes(f), np.uint8)
    hit = (b[1:-1] == 0xFF) & ((b[2:] & 0xFE) == 0xF8)
    return (np.flatnonzero(hit) + 1).tolist()


def sync_frames(cr: Crafted) -> list:
    """The frames for which `sync_positions` is not empty, found in one pass over the stream."""
    b = np.frombuffer(cr.flac, np.uint8)
    at = np.flatnonzero((b[:-1] == 0xFF) & ((b[1:] & 0xFE) == 0xF8))
    starts = np.asarray(cr.frame_offsets)
    at = at[at >= starts[0]]
    f = np.searchsorted(starts, at, side="right") - 1
    return sorted(set(f[at != starts[f]].tolist()))


# ---- the precondition model -------------------------------------------------------------------
@dataclasses.dataclass
class ChunkInfo:
    base: int
    active: bool      # the lane has samples in this chunk
    fast: bool        # run_subframe's lane_fast
    why: str          # "" or what keeps the chunk off the fast path
    k: int            # rice parameter at the chunk start, -1 in an escape partition / no residuals
    esc: bool         # the partition at the chunk start is an escape partition
    escw: int
    longest: int      # longest Rice code of the chunk (escape samples not counted)
    longest_at: int   # sample index of it within the chunk
    pair_max: int     # largest total of an aligned pair (samples base + 2j, base + 2j + 1) of Rice codes
    pair_at: int      # its pair slot j
    zero_peeks: int   # codes whose first 32 bits are all zero (quotient >= 32)
    bits: int         # bits the chunk reads: codes, warm-up excluded, partition headers included
    mix: bool         # CONSTANT / VERBATIM: fast only in the MIX kernels


def chunks(cr: Crafted, f: int, c: int) -> list:
    """The lane's chunks as run_subframe sees them."""
    L = cr.layout[f][c]
    out = []
    for base in range(0, L.bs, CHUNK):
        hi = min(base + CHUNK, L.bs)
        full = base + CHUNK <= L.bs and L.bs % 16 == 0
        if L.kind in ("const", "verbatim"):
            ok = full and (L.kind == "const" or L.cbps <= 32)
            out.append(ChunkInfo(base, True, ok, "" if ok else "short or wide", -1, False, 0, 0, 0, 0, 0, 0,
                                 int(L.clen[base:hi].sum()), True))
            continue
        lo = max(base, L.order)
        wu = L.order if base == 0 else 0
        if lo >= hi:  # warm-up only: left + wu >= 32 decides, with the first partition
            lo = hi
        p = int(L.part[lo]) if lo < L.bs else len(L.pk) - 1
        left = L.pstart[p + 1] - lo
        why = ""
        if not full:
            why = "block tail" if base + CHUNK > L.bs else "block size"
        elif left + wu < CHUNK:
            why = "partition ends"
        elif L.unsafe:
            why = "unsafe coefficients"
        sel = np.arange(lo, hi)
        rice = sel[np.asarray([L.pk[int(q)] >= 0 for q in L.part[sel]], dtype=bool)] if sel.size else sel
        n = L.clen
        longest = int(n[rice].max()) if rice.size else 0
        longest_at = int(rice[np.argmax(n[rice])] - base) if rice.size else 0
        pair_max, pair_at = 0, 0
        for j in range((hi - base) // 2):
            a = base + 2 * j
            if a >= lo and L.pk[int(L.part[a])] >= 0 and L.pk[int(L.part[a + 1])] >= 0:
                t = int(n[a] + n[a + 1])
                if t > pair_max:
                    pair_max, pair_at = t, j
        ks = np.asarray([L.pk[int(q)] for q in L.part[rice]], dtype=np.int64)
        zero_peeks = int(((n[rice] - ks - 1) >= 32).sum()) if rice.size else 0
        hdrs = sum((5 if L.method else 4) + (5 if L.pk[q] < 0 else 0) for q in range(len(L.pk)) if lo <= L.pstart[q] < hi
                   and q > 0)
        out.append(ChunkInfo(base, True, not why, why, L.pk[p], L.pk[p] < 0, max(L.pesc[p], 0), longest, longest_at,
                             pair_max, pair_at, zero_peeks, int(n[lo:hi].sum()) + hdrs, False))
    return out


def wave_lanes(cr: Crafted, wave: int = 0) -> list:
    """(frame, channel) of the lanes of wave `wave` of a stream whose frames fill whole waves:
    64 // channels frames, channel 0 of all of them first."""
    per = 64 // cr.channels
    frames = range(wave * per, min((wave + 1) * per, len(cr.layout)))
    return [(f, c) for c in range(cr.channels) for f in frames]


def simulate_wave(cr: Crafted, wave: int = 0, walk: bool = False) -> list:
    """The chunk loop of one wave of k_decode (or, `walk`, of k_walk over channels 0..n-2), ring
    state left out: per chunk a dict with the `form` ("slow", "warm", "esc", "pair", "one"),
    `redo`, the lanes `spoilers` that caused it with their reasons, and the pair back-off state
    (`cool` before the chunk, `fail` after it). Pairs: 16-bit containers (every container under
    the walk), every fast lane's k in 2 (walk: 1)..9, after the first chunk, back-off over."""
    lanes = [(f, c) for f, c in wave_lanes(cr, wave) if not walk or c < cr.channels - 1]
    infos = [chunks(cr, f, c) for f, c in lanes]
    mono = cr.channels == 1
    has_pairs = walk or widths(cr.bps)[0] == 16
    cool = fail = 0
    out = []
    for ci in range(len(infos[0])):
        row = [inf[ci] for inf in infos]
        rec = dict(base=row[0].base, cool=cool, spoilers=[])
        slow = [(lane, x.why) for lane, x in zip(lanes, row) if not x.fast]
        if slow:
            rec.update(form="slow", redo=True, spoilers=slow, fail=fail)
            out.append(rec)
            continue
        pred = [x for x in row if not x.mix]
        pairs = (has_pairs and cool == 0 and ci != 0
                 and all((1 if walk else 2) <= x.k <= PAIR_KMAX and not x.esc for x in pred))
        escs = any(x.esc for x in pred)
        if any(x.mix for x in row):
            form = "mixed"
        elif ci == 0:
            form = "warm"
        elif escs:
            form = "esc"
        else:
            form = "pair" if pairs else "one"
        if form == "pair":
            bad = [(lane, f"pair {x.pair_at} totals {x.pair_max}") for lane, x in zip(lanes, row) if x.pair_max > 32]
        else:
            bad = [(lane, f"code {x.longest_at} has {x.longest} bits") for lane, x in zip(lanes, row)
                   if not x.mix and not x.esc and x.longest > 32]
        redo = bool(bad)
        if has_pairs and pairs and redo:
            cool = (8 << min(fail, 4)) if mono else 8
            fail += 1
        elif mono and has_pairs and pairs:
            fail = 0
        elif cool:
            cool -= 1
        rec.update(form=form, redo=redo, spoilers=bad, fail=fail)
        out.append(rec)
    return out


def predict_probe(cr: Crafted, walk: bool = False) -> dict:
    """What the -DZFLAC_PROBE build's k_decode counters (tools/probe.py) read for this stream if the
    model is right and no ring runs dry: chunks, those with every active lane fast, those of
    them redone, the pair chunks, and those of them redone, summed over the stream's waves.
    `walk`: k_walk's counters for a stereo stream of one wave (channel 0, a lane per frame)."""
    out = dict(chunks=0, fast_chunks=0, redos=0, pair_chunks=0, pair_redos=0)
    for w in range(-(-len(cr.layout) // (64 // cr.channels))):
        for rec in simulate_wave(cr, w, walk):
            out["chunks"] += 1
            out["fast_chunks"] += rec["form"] != "slow"
            out["redos"] += rec["form"] != "slow" and rec["redo"]
            out["pair_chunks"] += rec["form"] == "pair"
            out["pair_redos"] += rec["form"] == "pair" and rec["redo"]
    return out


def segments(cr: Crafted, f: int, c: int, p: int) -> list:
    """k_walk_wave's view of Rice partition p of subframe (f, c): one dict per 4096-bit scan with
    `start` (the first code's bit position), `wbase` (lane 0's segment: the 32-bit word holding
    `start`; segment i is bits wbase + 64 i .. + 64), the codes' `starts` and `ends` inside the
    scan, and `next` (where the following scan, if any, begins: the first code start at or
    past wbase + 4096)."""
    L = cr.layout[f][c]
    a, b = L.pstart[p], L.pstart[p + 1]
    pos, n = L.cpos[a:b], L.clen[a:b]
    out, i = [], 0
    while i < pos.size:
        wbase = int(pos[i]) & ~31
        j = i
        while j < pos.size and pos[j] < wbase + 4096:
            j += 1
        out.append(dict(start=int(pos[i]), wbase=wbase, starts=pos[i:j].copy(), ends=(pos[i:j] + n[i:j]),
                        next=int(pos[j]) if j < pos.size else int(pos[-1] + n[-1])))
        i = j
    return out
