// decode/lane_reader.h -- Rdr: the lane bit reader over a per-lane LDS ring, and the ring's top-up.
#pragma once
#include "config.h"

namespace zflac {

// ----------------------------------------------------------------------------------
// Lane reader (bit_reader.zig semantics: MSB-first; EOF decided against `end`).
// Bit positions are offsets from the lane's 16-byte aligned base.
// ----------------------------------------------------------------------------------
// The window lives in the ring itself: a peek reads the two ring words around the position
// and joins them with one v_alignbit. The position is kept as one register, nb = 96 - pos
// (mod 2^32): its low 5 bits are the alignbit shift ((-pos) & 31), and the ring stores word
// i at slot (3 - i) & (RING_W - 1), so the slot of the peek's low word ceil(pos / 32) is
// (nb >> 5) & (RING_W - 1) and its high word sits one slot up. A consume is one subtraction;
// the two ring addresses are a shift, an add and two v_and_or, with no selects, borrow or
// byte swaps in the step (ring words are stored byte-swapped, MSB first, by the top-ups).
// Slots descend within a 16-byte quad (3 - i for i = 4q..4q+3), so a quad is four word
// slots in a row and never wraps.
constexpr uint32_t NB0 = 96;  // nb at bit position 0: 32 * 3, the slot constant times 32
struct Rdr {
    uint32_t nb;       // 96 - read position (see above)
    uint32_t wr;       // ring holds words < wr (multiple of 4)
    uint4 stg[6];      // quads wr/4.. staged by the last top-up (in flight until the next)
    bool sv;           // the staged quads are real data (the ring had room at issue)
    __amdgpu_buffer_rsrc_t rs;  // wave's input window (wave-uniform)
    uint32_t lofs;     // byte offset of the lane's quad 0 in the window
    uint32_t qa;       // the lane's quad 0, in quads past a 64-byte boundary (0..3)
    uint32_t qmax;     // last loadable quad
    uint32_t lds;      // index of this lane's slot-0 word in g_ring (wave * 4096 + lane)
    uint32_t junk;     // index of this lane's first junk word

    // an = index of the word after the peek's low word: the ring must hold words up to an
    // for the next step (the quantity the top-up and dry() rules are written in)
    __device__ __forceinline__ uint32_t an() const { return 4u - (uint32_t)((int32_t)nb >> 5); }
    __device__ __forceinline__ uint32_t ldsb() const {  // byte address of this lane's slot-0 word
        return (uint32_t)(uintptr_t)g_ring + lds * 4u;
    }
    __device__ __forceinline__ uint32_t lds_word(uint32_t byte_addr) const {
        return *reinterpret_cast<__attribute__((address_space(3))) const uint32_t*>((uintptr_t)byte_addr);
    }

    // word-slot index (in g_ring words, from `lds`) of the quad holding words 4q..4q+3:
    // its first slot holds word 4q + 3
    __device__ __forceinline__ uint32_t quad_slot(uint32_t q) const {
        return lds + ((0u - 4u * q) & (RING_W - 1)) * 64;
    }
    __device__ __forceinline__ void ring_quad(uint32_t q, uint4 v) { ring_store(quad_slot(q), v); }
    // the quad v (words 4q..4q+3 as loaded) at slot index b, byte-swapped, slots descending
    __device__ __forceinline__ void ring_store(uint32_t b, uint4 v) {
        g_ring[b] = bswap32(v.w);
        g_ring[b + 64] = bswap32(v.z);
        g_ring[b + 128] = bswap32(v.y);
        g_ring[b + 192] = bswap32(v.x);
    }
    // Quad q of the lane stream; a lane with `on` false reads out of the window's range,
    // which the buffer unit answers with zeros without touching the caches.
    __device__ __forceinline__ uint4 gload(uint32_t q, bool on = true) const {
        // (the empty asm pins the address computation ahead of the select: sunk into an
        // if / else on `on`, it let the register allocator reuse one quad's destination as
        // the other arm's address, and the top-up then waited for every memory op, vmcnt(0))
        uint32_t a = lofs + min(q, qmax) * 16u;
        asm volatile("" : "+v"(a));
        const uint32_t off = on ? a : 0x80000000u;
        return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
    }

    // (Re)start at bit P: synchronous, per subframe and on rare long skips. Loads 12 quads
    // straight into the ring from the 64-byte boundary (of the input buffer) at or below P's
    // quad, so that the lane's later 4-quad top-ups read aligned 64-byte pieces instead of
    // straddling two (straddling top-ups cost `k_decode` 1.37x the compressed input in
    // reads), with at least 9 quads from P's quad on. Quads before the lane's base (q0
    // "negative") wrap: their loads clamp to qmax and land in ring slots that are never read.
    // The staged sets become stale (stored into the junk slot). A peek at a quad's first bit
    // reads the word before the quad only with shift 0, where alignbit returns the low word.
    __device__ __forceinline__ void init(uint32_t P) {
        const uint32_t q0 = (((P >> 7) + qa) & ~3u) - qa;
        uint4 t[12];
#pragma unroll
        for (int i = 0; i < 12; i++) t[i] = gload(q0 + i);
#pragma unroll
        for (int i = 0; i < 12; i++) ring_quad(q0 + i, t[i]);
        wr = (q0 + 12) * 4;
        sv = false;
        nb = NB0 - P;
    }
    __device__ __forceinline__ uint32_t pos() const { return NB0 - nb; }
    __device__ __forceinline__ uint32_t unread() const { return wr - an() - 1; }
    // the next 32 bits of the stream: ring words ceil(pos / 32) - 1 and ceil(pos / 32),
    // shifted by (-pos) & 31 (a shift of 0 is the low word alone)
    __device__ __forceinline__ uint32_t peek() const {
        uint32_t hi, lo;
        fetch(hi, lo);
        return join(hi, lo);
    }
    // peek in two halves: the ring reads, and (once they have landed) the join, so a fast
    // step can issue the next step's reads before its own samples' arithmetic
    __device__ __forceinline__ void fetch(uint32_t& hi, uint32_t& lo) const {
        const uint32_t t = nb << 3;
        lo = lds_word(ldsb() | (t & RING_SLOT_MASK));
        hi = lds_word(ldsb() | ((t + 256u) & RING_SLOT_MASK));
    }
    __device__ __forceinline__ uint32_t join(uint32_t hi, uint32_t lo) const {
        return __builtin_amdgcn_alignbit(hi, lo, nb);
    }
    // Advance n bits (any n: the position is exact; reads past the stored words are caught
    // by dry() / ensure()).
    __device__ __forceinline__ void consume(uint32_t n) { nb -= n; }
    // Once per chunk, after the chunk-start wait: store the quads staged by the previous
    // top-up (into the junk slot when they were issued without room) and stage the next
    // QN quads (out of range, i.e. no memory traffic, when the ring has no room for them).
    // Writing words wr..wr+4QN-1 reuses the slots of wr-64..: they must be older than
    // an - 2 at issue (an only grows, and a redo rewinds at most to the chunk start).
    // `an_ref`: the position a redo may rewind to (the chunk start): the slots the top-up
    // writes must hold words older than it
    template <int QN>
    __device__ __forceinline__ void topup() { topup<QN>(an()); }
    template <int QN>
    __device__ __forceinline__ void topup(uint32_t an_ref) {
        // Lazy: while every lane of the wave still holds more stored words than a chunk
        // normally reads (4 QN: 16 bits per sample, 24 for 32-bit containers), the staged
        // quads stay in flight. No wait, no stores, no loads: a top-up then runs about once
        // per 4 QN words consumed (every ~2 chunks at C5's ~9 bits per sample) and its loads
        // have that long to land. (A chunk that reads more runs dry and is redone.)
        if (__builtin_amdgcn_ballot_w64(unread() < (uint32_t)(4 * QN + 4)) == 0) return;
        const uint32_t junk_w = junk;
#pragma unroll
        for (int q = 0; q < QN; q++) ring_store(sv ? quad_slot((wr >> 2) + q) : junk_w, stg[q]);
        wr += sv ? 4u * QN : 0u;
        const bool room = wr - an_ref - 1 <= (uint32_t)(RING_W - 3 - 4 * QN);
        sv = room;
        // a wave with no lane that has room issues no loads (the vector-memory pipeline
        // pays per instruction, not per active lane)
        if (__builtin_amdgcn_ballot_w64(room) != 0) {
            // the QN quads from one base offset (instruction offsets 16, 32, ..): quads past
            // the stream read the next stream's bytes or (past the window) zeros, never used
            // (round 5 clamped each quad to the stream's last one: 4 VALU per quad)
            uint32_t base = lofs + (wr >> 2) * 16u;
            asm volatile("" : "+v"(base));  // (as in gload: the select must not sink into the loads)
            base = room ? base : 0x80000000u;
#pragma unroll
            for (int q = 0; q < QN; q++)
                stg[q] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, base + 16u * q, 0, 0));
        }
    }
    // the reads so far (ring[an] at the latest, and the step that may follow: ring[an + 1])
    // lie in stored data
    __device__ __forceinline__ bool dry() const { return an() + 2 > wr; }
    // At least `words` stored words ahead of `an` before the next reads (with margin).
    __device__ __forceinline__ void ensure(uint32_t words) {
        if (unread() < words + 3) init(pos());
    }
    __device__ __forceinline__ uint32_t hi() const { return peek(); }
    __device__ __forceinline__ uint32_t read(uint32_t n) {  // n in [0, 32]
        const uint32_t v = n ? peek() >> (32 - n) : 0u;
        consume(n);
        return v;
    }
    __device__ __forceinline__ int32_t read_signed(uint32_t n) {  // n in [1, 32], src/zflac.zig:188-196
        const uint32_t v = read(n);
        return (int32_t)(v << (32 - n)) >> (32 - n);
    }
    __device__ __forceinline__ int64_t read_signed_wide(uint32_t n) {  // n in [1, 64]
        if (n <= 32) return read_signed(n);
        ensure(3);
        const uint64_t h = read(n - 32);
        const uint64_t l = read(32);
        const uint64_t v = (h << 32) | l;
        return (int64_t)(v << (64 - n)) >> (64 - n);
    }
    __device__ __forceinline__ void skip(uint64_t n) {
        if (n <= 32) {
            consume((uint32_t)n);
        } else {
            const uint64_t np = (uint64_t)pos() + n;
            init(np > 0xFFFFFF00ull ? 0xFFFFFF00u : (uint32_t)np);
        }
    }
    // readUnary (bit_reader.zig:95-120); false on EndOfStream
    __device__ __forceinline__ bool unary(uint32_t end, uint32_t& q) {
        q = 0;
        for (;;) {
            ensure(2);
            const uint32_t h = hi();
            if (h) {
                const uint32_t z = __builtin_clz(h);
                q += z;
                consume(z + 1);
                return pos() <= end;
            }
            q += 32;
            consume(32);
            if (pos() > end) return false;
        }
    }
};

}  // namespace zflac
