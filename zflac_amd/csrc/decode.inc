// decode.inc -- the hot path: subframe decode kernels, lane per subframe.
//
// Included by decode_k{0,1,2}_{stereo,mono,multi}.hip: one translation unit per SampleType
// container (i8 / i16 / i32; src/zflac.zig:255-265) and channel layout; the stereo units
// also instantiate k_walk.
//
// Wave mapping: 64 lanes = F frames x C channels (F = 64 / C): lane = c * F + j.
// Stereo: lanes 0-31 channel 0, lanes 32-63 channel 1 of the same 32 frames, so the
// partner of a lane is lane ^ 32 and stereo decorrelation is one v_permlane32_swap.
//
// Two kernels per frame batch: (1) k_walk, one lane per frame: subframe c+1 starts where
// subframe c ends, so the lane parses subframes 0..C-2 without producing samples and
// records where each later subframe starts (DecodeArgs::sub_start); (2) k_decode, every
// lane decodes its subframe: header, warm-up, Rice / escape residuals (two Rice codes per
// window step while k <= PAIR_KMAX), fixed / LPC rollback in registers (packed i16 LPC via
// v_dot2), wasted bits, decorrelation, left-justify, packed stores.
//
// Lane input: a per-lane 64-word ring in LDS holding the stream byte-swapped (MSB first); a
// peek reads the two ring words around the bit position and joins them with one v_alignbit,
// and the position is one register (Rdr::nb), so a consume is one subtraction. The ring is
// topped up at chunk starts (CHUNK = 32 samples): the buffer loads staged by the previous
// top-up are stored into the ring and the next ones issued, so every load has a chunk or
// more to land and the per-sample work is ALU + LDS reads. A lane that would run its ring
// dry redoes the chunk on the generic path (synchronous refills).
#include "device_common.h"
#include "launch.h"

namespace zflac {

// Ring quads per lane: 16 (64 words, 16 KiB per wave) by default; the 32-bit-container units
// (decode_k2_*.hip) define 32 (128 words, 32 KiB per wave): at 17..32 bits per sample a chunk
// reads up to ~24 words, which a 64-word ring cannot keep stored ahead while the next top-up is
// in flight (the 32-bit row redid 87 % of its chunks on the generic path, dry).
#ifndef ZFLAC_RING_Q
#define ZFLAC_RING_Q 16
#endif
constexpr int RING_Q = ZFLAC_RING_Q;             // 16-byte quads per lane
constexpr int RING_W = RING_Q * 4;               // words per lane
constexpr uint32_t RING_SLOT_MASK = (uint32_t)(RING_W - 1) << 8;  // word slot bits of a pre-shifted index
constexpr int RING_WAVE_WORDS = RING_W * 64;      // per wave, layout [word slot][lane]: a lane's
                                                  // word index is wave * RING_WAVE_WORDS | slot << 6 | lane
constexpr int JUNK_WAVE_WORDS = 4 * 64;           // k_walk: + 4 junk word slots per wave, after all the
                                                  // rings (a top-up with no room writes there); k_decode
                                                  // uses the first 4 word slots of the wave's output
                                                  // stage instead (free at every top-up, see topup_st)
// k_decode: 4 waves per workgroup (80 KiB of LDS), 2 workgroups (8 waves) per CU. Round 5:
// with four runs in flight 681-694k vs 665-669k Msamples/s for 2-wave workgroups (same box,
// alternating; isolated decode the same), as the 4-wave walk workgroups place one wave per
// SIMD of a CU at a time (ZFLAC_DEC_THREADS=128 builds the 2-wave form).
#ifndef ZFLAC_DEC_THREADS
#define ZFLAC_DEC_THREADS 256
#endif
constexpr int DEC_THREADS = ZFLAC_DEC_THREADS;
// k_walk: 4 waves per workgroup (rings only). 2-wave workgroups (34 KiB, which fit beside
// three k_decode workgroups on a CU) measured slower both serially (walk 0.257 vs 0.234 ms)
// and with three shard runs in flight (471k vs 491k Msamples/s).
#ifndef ZFLAC_WALK_THREADS
#define ZFLAC_WALK_THREADS 256
#endif
constexpr int WALK_THREADS = ZFLAC_WALK_THREADS;
// Samples per chunk: 32 (CHUNK for k_walk, DEC_CHUNK for k_decode). The ring is topped up
// at chunk starts, right after the wait for everything issued before: the loads staged then
// are stored into the ring now and the next ones issued, so every load has 32 samples or
// more to land. The output stage holds one chunk (STAGE_SAMPLES). (64-sample decode chunks,
// round 5, spilled 126 VGPRs in the order-8 kernel: DESIGN.md section 10.)
constexpr int CHUNK = 32;
constexpr int DEC_CHUNK = 32;
constexpr int STAGE_SAMPLES = 32;
// Quads staged per top-up: 4 (16 words = 16 bits/sample) for 8- and 16-bit containers, 6
// for 32-bit ones. A lane that reads faster than that runs its ring dry and redoes the
// chunk on the generic path, which refills synchronously.
template <int KIND>
__device__ __forceinline__ constexpr int topup_quads() { return KIND == 2 ? 6 : 4; }
// Largest Rice parameter for which the fast chunk decodes two codes per 32-bit window: a
// pair then spills past the window only when its two quotients sum to more than 30 - 2k.
constexpr uint32_t PAIR_KMAX = 9;
// Word 3 of a raw (stride 0) buffer resource on gfx9-family targets: 32-bit data format.
constexpr int BUFFER_RSRC_WORD3 = 0x00020000;
constexpr int DEC_WAVES = DEC_THREADS / 64;

// Dynamic LDS of both kernels: the rings of the workgroup's waves, [wave][word slot][lane]
// of uint32 (16 KiB per wave), then the junk slots (k_walk, 1 KiB per wave) or one output
// stage per wave (k_decode, 4 KiB: 20 KiB per wave, so four 2-wave workgroups fill a CU's
// 160 KiB and the 256-VGPR decode kernels reach their register limit of 2 waves per SIMD). Declared
// __shared__ so every access is a true LDS (ds_*) instruction, never FLAT.
extern __shared__ uint32_t g_ring[];
// Output staging of the 16-bit stereo fast path: one chunk of a wave's 32 frames, 32 frames
// x 8 pieces of 16 B (4 KiB per wave). Piece p of frame j sits at quad j * 8 + (p ^ (j & 7)):
// the per-group writes (8 consecutive lanes = 8 frames) and the row reads (8 lanes = one
// frame's 128 B) are both free of bank conflicts. Written back as 128-byte runs per frame.
constexpr int STAGE_QUADS = 32 * 8;
// (k_decode only: its workgroup size is the constant DEC_THREADS. blockDim.x is a load from
// the dispatch packet, which the register allocator rematerialised inside the steps.)
__device__ __forceinline__ uint4* stage_base() {
    return reinterpret_cast<uint4*>(g_ring + DEC_WAVES * RING_WAVE_WORDS);
}
constexpr size_t DEC_LDS_BYTES = (size_t)DEC_WAVES * (RING_WAVE_WORDS * 4 + STAGE_QUADS * 16);
static_assert(RING_Q != 16 || (8 / DEC_WAVES) * DEC_LDS_BYTES <= 160 * 1024, "eight k_decode waves per CU");
static_assert(DEC_LDS_BYTES <= 160 * 1024, "a k_decode workgroup fits a CU");
constexpr size_t WALK_LDS_BYTES = (size_t)(WALK_THREADS / 64) * (RING_WAVE_WORDS + JUNK_WAVE_WORDS) * 4;

enum Layout : int { LAY_MONO = 1, LAY_STEREO = 2, LAY_MULTI = 0 };
enum Mode : int { M_NONE = 0, M_CONST = 1, M_VERB = 2, M_PRED = 3 };
enum Decor : int { D_NONE = 0, D_MS = 10, D_GEN = 1 };

template <int KIND>
struct Kind;
template <>
struct Kind<0> {  // 8-bit container, InterType i16
    static constexpr int SB = 8, W = 16, ESZ = 1;
};
template <>
struct Kind<1> {  // 16-bit container, InterType i32
    static constexpr int SB = 16, W = 32, ESZ = 2;
};
template <>
struct Kind<2> {  // 32-bit container (17..32 bps), InterType i64
    static constexpr int SB = 32, W = 64, ESZ = 4;
};

// Compile-time loop: f(std::integral_constant<int, I>) for I in [0, N).
template <typename F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

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

// ----------------------------------------------------------------------------------
// Lane subframe state
// ----------------------------------------------------------------------------------
// Packed PCM quads of the last 8 samples, stored at the next top-up (before its waits):
// every path between two top-ups then carries a store younger than the staged loads,
// so the waitcnt pass can prove vmcnt(1)/(2) instead of draining everything.
struct Pend {
    uint4* p;  // target (the lane's dummy slot when nothing is pending)
    uint4 v0, v1;
    __device__ __forceinline__ void flush(bool two) {
        p[0] = v0;
        if (two) p[1] = v1;
    }
};

// Packed i16 pairs (two samples per register): element-wise, wrapping like the scalar
// path's truncation to the i16 SampleType.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 as_u16x2(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t as_u32(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint32_t pk_shl(uint32_t v, uint32_t n) {
    return as_u32(as_u16x2(v) << (u16x2){(unsigned short)n, (unsigned short)n});
}
__device__ __forceinline__ uint32_t pk_sar1(uint32_t v) {
    return as_u32(__builtin_bit_cast(u16x2, __builtin_bit_cast(s16x2, v) >> (s16x2){1, 1}));
}

// Mid/side decorrelation of two packed sample pairs (src/zflac.zig:553-578): x0 = mid, x1 =
// side, out L / R pairs; R = M - (S >> 1), L = R + S in i16, `ovf` collecting the signed
// overflow bits (15 and 31) of both operations (:573-574 @intCast).
__device__ __forceinline__ void decorrelate2_ms(uint32_t x0, uint32_t x1, uint32_t& Lp, uint32_t& Rp, uint32_t& ovf) {
    const uint32_t d = pk_sar1(x1);
    const uint32_t r = as_u32(as_u16x2(x0) - as_u16x2(d));
    const uint32_t l = as_u32(as_u16x2(r) + as_u16x2(x1));
    Rp = r;
    Lp = l;
    ovf |= ((x0 ^ d) & (x0 ^ r)) | (~(r ^ x1) & (r ^ l));
}

// The 16-bit fast path's staged chunk (g_stage), written back at the next chunk start
// (after that chunk's wait, like Pend), 4 KiB per wave either way:
// * stereo: 32 frames x 8 pieces of 16 B (4 interleaved L/R samples); row t of the write-back
//   covers frames 8t..8t+7, lane L piece L & 7 of frame 8t + (L >> 3): each store
//   instruction writes 8 frames x 128 contiguous bytes;
// * mono: 64 frames x 4 pieces of 16 B (8 samples); row t covers frames 16t..16t+15, lane L
//   piece L & 3 of frame 16t + (L >> 2): 16 frames x 64 contiguous bytes per store, where
//   per-lane stores wrote 64 separate 16-byte pieces.
// The piece swizzles keep both the per-group writes and the row reads free of bank conflicts.
// A global-memory (address space 1) quad pointer: the stage's output base is laundered into
// VGPRs (see run_subframe), after which the compiler can no longer infer its address space.
typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4v guint4;

template <bool MONO>
struct Stage {
    static constexpr uint32_t PIECES = MONO ? 4u : 8u;    // 16-byte pieces per frame and chunk
    static constexpr uint32_t ROW_FRAMES = 64u / PIECES;  // frames per write-back row
    using Mask = std::conditional_t<MONO, uint64_t, uint32_t>;
    guint4* out;     // the output buffer (wave-uniform, held in VGPRs): the pointer write-back
    __amdgpu_buffer_rsrc_t rs;  // the same buffer as a raw resource (SGPRs): the resource write-back
    uint32_t gq[4];  // quad index (from `out`) of this lane's piece of row t at sample 0
    Mask mask;       // frames (bit j) whose staged chunk is valid: fast, not redone, writable
    uint32_t base;   // first sample of the staged chunk
    uint32_t q0;     // this wave's first quad in g_stage
    __device__ __forceinline__ static uint32_t lane() { return threadIdx.x & 63u; }
    __device__ __forceinline__ static uint32_t row_frame(int t) {
        return (uint32_t)t * ROW_FRAMES + (lane() / PIECES);
    }
    // quad of piece p of frame j
    __device__ __forceinline__ uint32_t quad(uint32_t j, uint32_t p) const {
        if constexpr (MONO) return q0 + j * 4u + (p ^ ((j >> 1) & 3u));
        else return q0 + j * 8u + (p ^ (j & 7u));
    }
    __device__ __forceinline__ void put(uint32_t group, uint4 v) {  // group = 8-sample group 0..3
        if constexpr (MONO) {
            stage_base()[quad(lane(), group)] = v;
        } else {
            const uint32_t j = lane() & 31u, c = lane() >> 5;
            stage_base()[quad(j, 2u * group + c)] = v;
        }
    }
    __device__ __forceinline__ void read(uint4 (&v)[4]) const {
#pragma unroll
        for (int t = 0; t < 4; t++) v[t] = stage_base()[quad(row_frame(t), lane() & (PIECES - 1u))];
    }
    __device__ __forceinline__ void store(const uint4 (&v)[4], uint4* dummy) const {
        // quads per sample of the chunk: 4 bytes per stereo sample, 2 per mono one
        const uint32_t bq = MONO ? base / 8u : base / 4u;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const bool ok = (mask >> row_frame(t)) & 1u;
            guint4* dst = ok ? out + (gq[t] + bq) : (guint4*)(dummy + (t & 1));
            *dst = __builtin_bit_cast(u32x4v, v[t]);
        }
    }
    // The same rows through the buffer resource (WB_RSRC launches: the class's output is at most
    // WB_RSRC_MAX bytes). The offset is 32 bits, one v_add_lshl, and a masked row sets its bit 31,
    // which lies past the resource: the buffer unit drops the store, no dummy line is written. The
    // row's bit comes from a scalar shift of ~mask by the row's first frame, then one per-lane
    // shift by the lane's frame within the row; v_lshl_or moves it to bit 31 and drops the rest.
    __device__ __forceinline__ void store_rsrc(const uint4 (&v)[4]) const {
        const uint32_t bq = MONO ? base / 8u : base / 4u;
        const uint32_t fr = lane() / PIECES;  // this lane's frame within a row
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t dead = (uint32_t)((Mask)~mask >> (t * (int)ROW_FRAMES)) >> fr;
            const uint32_t off = ((gq[t] + bq) << 4) | (dead << 31);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v[t]), rs, (int)off, 0, 0);
        }
    }
    template <bool WBR>
    __device__ __forceinline__ void flush(uint4* dummy) {
        uint4 v[4];
        read(v);
        if constexpr (WBR) store_rsrc(v);
        else store(v, dummy);
    }
};
template <int LAY>
using StageOf = Stage<LAY == LAY_MONO>;
// 16-bit containers, stereo or mono: PCM goes through the stage
template <int KIND, int LAY>
__host__ __device__ __forceinline__ constexpr bool staged() { return KIND == 1 && LAY != LAY_MULTI; }

template <int KIND>
__device__ __forceinline__ constexpr bool pend_two() { return KIND == 2; }

// Per-lane dummy slot (2 quads), spread over 64 wave slots so masked stores of different
// waves do not pile onto the same lines. DUMMY_BYTES on the host side.
__device__ __forceinline__ uint32_t dummy_slot() {
    return 2u * ((threadIdx.x & 63u) + 64u * ((blockIdx.x * DEC_WAVES + (threadIdx.x >> 6)) & 63u));
}

// Top-up with the pending store issued first (decode); plain top-up for the walk.
// Chunk-start top-up: pending PCM store first (it then has the whole chunk to complete
// before the next chunk-start wait), then the ring.
// The previous chunk's PCM stores first, then the top-up (its wait for the previous
// top-up's loads, the ring stores, the next loads). (Loads first and stores after measured
// 20 % slower in k_decode: 0.67 vs 0.56 ms on the C5 shard.)
// k_decode's junk slots are the first word slots of the wave's output stage: the flush has
// just read every staged piece into registers (LDS operations of a wave complete in order),
// and the chunk's own pieces are written only after this top-up.
template <int KIND, int LAY, bool WALK, bool WBR>
__device__ __forceinline__ void topup_st(Rdr& rd, Pend& pd, StageOf<LAY>& sg, uint4* dummy) {
    if constexpr (!WALK) {
        if constexpr (staged<KIND, LAY>()) sg.template flush<WBR>(dummy);
        else pd.flush(pend_two<KIND>());
    }
    rd.template topup<topup_quads<KIND>()>();
}

struct LaneCtx {
    uint32_t bs;
    int bps;           // frame bits per sample
    int ubps;          // + 1 on the side channel (src/zflac.zig:436-441)
    uint32_t chan_code;
    uint32_t end;      // stream end, bit offset from the lane base
    int mode;
    int wasted;
    int cbps;          // coded bits of warm-up / verbatim samples
    int order;
    int shift;
    int32_t cval;
    int method;
    uint32_t psize;
    uint32_t parts_left;
    uint32_t left;     // residuals left in the current partition
    uint32_t k;
    uint32_t kp1;      // k + 1
    uint32_t thr;      // a 32-bit peek below thr means the code is longer than 32 bits
    uint32_t escw;
    bool esc;
    int err;
    // Value-range state (Debug zflac traps, reported as OutOfDomain like the oracle's
    // checked build). `dom`: a predicted sample did not fit the SampleType (:494,537 @intCast)
    // or overflowed the InterType; deferred because zflac reads every residual of a subframe
    // before running its predictor, so a residual read error of the same subframe wins.
    // `unsafe`: the coefficients are large enough that a partial LPC sum could overflow the
    // InterType (sum |c| * 2^(SB-1) over the bound), so the lane takes the generic path, which
    // checks every partial sum in zflac's order (:527-532). `dcr`: decorrelation overflow in
    // the SampleType (:558,564,573-574), reported after the frame's subframes and CRC.
    bool dom;
    bool unsafe;
    uint32_t dcr;
};

// Does v fit the SampleType of container KIND (src/zflac.zig:198-201 @intCast)?
template <int KIND>
__device__ __forceinline__ bool fits_sb(int64_t v) {
    if constexpr (Kind<KIND>::SB == 8) return v == (int64_t)(int8_t)v;
    else if constexpr (Kind<KIND>::SB == 16) return v == (int64_t)(int16_t)v;
    else return v == (int64_t)(int32_t)v;
}
// Largest sum |c| * 2^(SB-1) for which no partial LPC sum can leave the InterType (8-bit:
// i16) and the fast path's i32 `r + prediction` cannot wrap (16-bit: |r| <= 2^30 there).
template <int KIND>
__device__ __forceinline__ constexpr uint64_t safe_lpc_bound() {
    return KIND == 0 ? 0x7FFFull : (KIND == 1 ? (1ull << 30) : ~0ull);
}

__device__ __forceinline__ void set_err(LaneCtx& L, const Rdr& rd, int e) {
    if (!L.err) L.err = (rd.pos() > L.end) ? E_END_OF_STREAM : e;
    L.mode = M_NONE;
}

// Partition header (src/zflac.zig:635-654)
template <int KIND>
__device__ __forceinline__ void read_partition_header(LaneCtx& L, Rdr& rd) {
    const uint32_t k = rd.read(L.method ? 5 : 4);
    L.esc = k == (L.method ? 31u : 15u);
    L.k = L.esc ? 0u : k;
    L.kp1 = L.k + 1;
    L.thr = 1u << L.k;  // q = clz(h) <= 31 - k  <=>  h >= 2^k: the whole code is in the peek
    L.escw = 0;
    if (L.esc) {
        L.escw = rd.read(5);
        if (L.escw > (uint32_t)Kind<KIND>::W) set_err(L, rd, E_OUT_OF_DOMAIN);  // read_signed_integer assert
    } else if (k >= (uint32_t)Kind<KIND>::W) {
        set_err(L, rd, E_OUT_OF_DOMAIN);  // :656 unreachable
    }
    L.left = L.psize;
    L.parts_left--;
}

// Residual header (src/zflac.zig:614-633)
template <int KIND>
__device__ __forceinline__ void read_residual_header(LaneCtx& L, Rdr& rd) {
    const uint32_t method = rd.read(2);
    if (method >= 2) { set_err(L, rd, E_INVALID_RESIDUAL_CODING); return; }  // :618
    L.method = (int)method;
    const uint32_t po = rd.read(4);
    L.psize = L.bs >> po;
    // :626 `count -= order` underflow; :623-632 stale residuals when bs % 2^po != 0
    if (L.psize < (uint32_t)L.order || (L.psize << po) != L.bs) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
    L.parts_left = 1u << po;
    read_partition_header<KIND>(L, rd);
    L.left = L.psize - (uint32_t)L.order;
}

template <int KIND>
__device__ __forceinline__ int64_t zigzag(uint64_t zz) {
    if constexpr (Kind<KIND>::W == 64) return (int64_t)((zz >> 1) ^ (0 - (zz & 1)));
    else if constexpr (Kind<KIND>::W == 32) return (int32_t)(((uint32_t)zz >> 1) ^ (0u - ((uint32_t)zz & 1)));
    else {
        const uint32_t z = (uint32_t)zz & 0xFFFFu;
        return (int16_t)((z >> 1) ^ (0u - (z & 1)));
    }
}

// Rice code, any length (src/zflac.zig:657-663)
template <int KIND>
__device__ __forceinline__ int64_t rice_general(LaneCtx& L, Rdr& rd) {
    uint32_t q;
    if (!rd.unary(L.end, q)) { set_err(L, rd, E_END_OF_STREAM); return 0; }
    const uint32_t rem = rd.read(L.k);
    if constexpr (Kind<KIND>::W == 16) {
        if (q > 0xFFFFu) set_err(L, rd, E_OUT_OF_DOMAIN);  // @intCast(readUnary()) to u16
    }
    if constexpr (Kind<KIND>::W == 64) return zigzag<KIND>(((uint64_t)q << L.k) + rem);
    else return zigzag<KIND>((uint64_t)((q << L.k) + rem));  // `<<` discards in u32 / u16
}

// One residual of the current partition, generic path.
template <int KIND>
__device__ __forceinline__ int64_t residual_general(LaneCtx& L, Rdr& rd) {
    if (L.esc) return L.escw ? (int64_t)rd.read_signed(L.escw) : 0;
    const uint32_t h = rd.hi();
    if (h >= L.thr) {
        const uint32_t q = __builtin_clz(h);
        const uint32_t len = q + L.kp1;
        const uint32_t rem = __builtin_amdgcn_ubfe(h, 32 - len, L.k);
        rd.consume(len);
        return zigzag<KIND>((q << L.k) | rem);
    }
    return rice_general<KIND>(L, rd);
}

// ----------------------------------------------------------------------------------
// Predictor state. 16-bit and 8-bit containers: every subframe value fits i16 inside
// zflac's domain (src/zflac.zig:494,537 @intCast), so the order-M sum is M/2
// v_dot2c_i32_i16 over packed sample pairs; pair P[t mod M] = (lo s[t-1], hi s[t]) and
// coefficient pair m = (lo c[2m+1], hi c[2m]) where c[j] multiplies s[i-1-j]. For odd t,
// P[t] is also the little-endian i16 PCM pair (s[t-1], s[t]) the packed stores need.
// 32-bit containers: i64 sums of i32 products (InterType i64).
// ----------------------------------------------------------------------------------
typedef short short2v __attribute__((ext_vector_type(2)));

// History ring length of a bucket: the largest order M rounded up to a power of two that
// divides the chunk, so history slots line up from chunk to chunk (bucket 12: order 9..12,
// a 16-slot ring but 12 products per sample instead of 16).
template <int M>
__host__ __device__ constexpr int hist_len() { return M == 12 ? 16 : M; }

template <int KIND, int M, bool PAIRS = (KIND != 2)>
struct Pred;

template <int KIND, int M>
struct Pred<KIND, M, true> {
    static constexpr int H = hist_len<M>();
    uint32_t P[H];
    uint32_t CP[M / 2];
    int32_t last;
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < H; j++) P[j] = 0;
#pragma unroll
        for (int m = 0; m < M / 2; m++) CP[m] = 0;
        last = 0;
    }
    template <int J>
    __device__ __forceinline__ void set_coef(int32_t c) {
        if constexpr ((J & 1) == 0) CP[J >> 1] = (CP[J >> 1] & 0xFFFFu) | ((uint32_t)c << 16);
        else CP[J >> 1] = (CP[J >> 1] & 0xFFFF0000u) | ((uint32_t)c & 0xFFFFu);
    }
    template <int U>
    __device__ __forceinline__ void push(int32_t s) {
        P[U % H] = __builtin_amdgcn_perm((uint32_t)s, (uint32_t)last, 0x05040100u);  // lo last, hi s
        last = s;
    }
    template <int U>
    __device__ __forceinline__ uint32_t pair() const { return P[U % H]; }
    template <int U>
    __device__ __forceinline__ int32_t value() const {  // s at slot U (prologue warm-up)
        return (int32_t)(int16_t)(P[U % H] >> 16);
    }
    template <int U>
    __device__ __forceinline__ int64_t predict(int shift) const {
        // oldest pairs first: the newest pair (holding s[i-1], just computed) enters last,
        // so the recurrence's dependency chain is one dot2 + shift + add + pack per sample
        // (wrapping i32 / i16 sums: the order does not change the result)
        // the oldest pair starts the sum as v_dot2_i32_i16 with an inline 0 accumulator (the
        // builtin's VOP2 form needs a zeroed register: one v_mov per sample)
        int32_t acc;
        asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(acc) : "v"(P[(((U - 1 - 2 * (M / 2 - 1)) % H) + H) % H]), "v"(CP[M / 2 - 1]));
#pragma unroll
        for (int m = M / 2 - 2; m >= 0; m--) {
            const uint32_t a = P[(((U - 1 - 2 * m) % H) + H) % H];
            acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, CP[m]), acc,
                                         false);
        }
        if constexpr (Kind<KIND>::W == 16) acc = (int16_t)acc;
        return acc >> shift;
    }
    // Every product and partial sum of the prediction of slot U fits the InterType, in
    // zflac's accumulation order: oldest sample first (src/zflac.zig:527-532). Only for
    // `unsafe` lanes (large coefficients); history values fit the SampleType here.
    template <int U>
    __device__ __forceinline__ bool partials_fit(int order) const {
        constexpr int64_t HI = Kind<KIND>::W == 16 ? 0x7FFF : 0x7FFFFFFF;
        int64_t p = 0;
        bool ok = true;
#pragma unroll
        for (int j = M - 1; j >= 0; j--) {
            if (j < order) {
                const int64_t sv = (int16_t)(P[(((U - 1 - j) % H) + H) % H] >> 16);
                const int64_t cv = (j & 1) ? (int16_t)(CP[j >> 1] & 0xFFFFu) : (int16_t)(CP[j >> 1] >> 16);
                const int64_t prod = sv * cv;
                p += prod;
                ok = ok && prod >= -HI - 1 && prod <= HI && p >= -HI - 1 && p <= HI;
            }
        }
        return ok;
    }
};

template <int KIND, int M>
struct Pred<KIND, M, false> {
    static constexpr int H = hist_len<M>();
    int32_t R[H];
    int32_t C[M];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < H; j++) R[j] = 0;
#pragma unroll
        for (int j = 0; j < M; j++) C[j] = 0;
    }
    template <int J>
    __device__ __forceinline__ void set_coef(int32_t c) {
        C[J] = c;
    }
    template <int U>
    __device__ __forceinline__ void push(int32_t s) {
        R[U % H] = s;
    }
    template <int U>
    __device__ __forceinline__ int32_t value() const {
        return R[U % H];
    }
    template <int U>
    __device__ __forceinline__ int64_t predict(int shift) const {
        // ACC independent i64 accumulators over interleaved terms, the newest term (s[i-1])
        // last in accumulator 0: wrapping i64 sums, so any order gives zflac's result; more
        // accumulators shorten the chain of dependent v_mad_i64_i32 per sample
#ifndef ZFLAC_K2_ACC
#define ZFLAC_K2_ACC 1
#endif
        constexpr int ACC = ZFLAC_K2_ACC < M - 1 ? ZFLAC_K2_ACC : M - 1;
        int64_t acc[ACC];
#pragma unroll
        for (int a = 0; a < ACC; a++) acc[a] = 0;
#pragma unroll
        for (int j = M - 1; j >= 1; j--) acc[j % ACC] += (int64_t)C[j] * (int64_t)R[(((U - 1 - j) % H) + H) % H];
#pragma unroll
        for (int a = 1; a < ACC; a++) acc[0] += acc[a];
        acc[0] += (int64_t)C[0] * (int64_t)R[(((U - 1) % H) + H) % H];  // s[i-1] last
        return acc[0] >> shift;
    }
};

template <int KIND>
__device__ __forceinline__ int32_t add_inter(int64_t r, int64_t p) {
    if constexpr (Kind<KIND>::W == 16) return (int16_t)(r + p);
    else if constexpr (Kind<KIND>::W == 32) return (int32_t)((uint32_t)r + (uint32_t)p);
    else return (int32_t)(r + p);
}

template <int KIND>
__device__ __forceinline__ int32_t wrap_st(int64_t v) {
    if constexpr (Kind<KIND>::SB == 8) return (int32_t)(int8_t)v;
    else if constexpr (Kind<KIND>::SB == 16) return (int32_t)(int16_t)v;
    else return (int32_t)v;
}

// Warm-up samples (src/zflac.zig:474,506 read_unencoded_sample): each must fit the
// SampleType, checked as it is read; the first that does not ends the subframe there.
template <int KIND, int M>
__device__ __forceinline__ bool read_warmup(LaneCtx& L, Rdr& rd, Pred<KIND, M>& pr, int order) {
    bool ok = true;
    static_for<M>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        if (J < order && ok) {
            rd.ensure(3);
            const int64_t v = rd.read_signed_wide((uint32_t)L.cbps);
            ok = fits_sb<KIND>(v);
            pr.template push<J>((int32_t)v);
        }
    });
    if (!ok) set_err(L, rd, E_OUT_OF_DOMAIN);
    return ok;
}

// Full subframe header (src/zflac.zig:426-520); warm-up samples are pushed as samples
// 0..order-1 of the predictor history.
template <int KIND, int M>
__device__ __forceinline__ void parse_subframe(LaneCtx& L, Rdr& rd, Pred<KIND, M>& pr) {
    L.mode = M_NONE;
    L.unsafe = false;
    pr.clear();
    const uint32_t h8 = rd.read(8);
    if (h8 >> 7) { set_err(L, rd, E_INVALID_SUBFRAME_HEADER); return; }  // :431
    const uint32_t type = (h8 >> 1) & 63;
    int wasted = 0;
    if (h8 & 1) {  // :433
        uint32_t u;
        if (!rd.unary(L.end, u)) { set_err(L, rd, E_END_OF_STREAM); return; }
        if (u + 1 >= 64) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
        wasted = (int)u + 1;
    }
    L.wasted = wasted;
    if (type == 0) {  // constant: reads bits_per_sample, not the side depth (:447)
        if (L.bps <= wasted || L.bps - wasted > Kind<KIND>::W || wasted >= Kind<KIND>::SB) {
            set_err(L, rd, E_OUT_OF_DOMAIN);
            return;
        }
        const int64_t v = rd.read_signed_wide((uint32_t)(L.bps - wasted));
        if (!fits_sb<KIND>(v)) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }  // rd_unencoded @intCast
        L.cval = wrap_st<KIND>((int64_t)((uint64_t)v << wasted));
        L.mode = M_CONST;
        return;
    }
    if (L.ubps <= wasted || L.ubps - wasted > Kind<KIND>::W || (wasted > 0 && wasted >= Kind<KIND>::SB)) {
        set_err(L, rd, E_OUT_OF_DOMAIN);
        return;
    }
    L.cbps = L.ubps - wasted;
    if (type == 1) {  // verbatim (:455-465)
        L.mode = M_VERB;
        return;
    }
    int order;
    if (type >= 8 && type <= 12) {  // fixed (:466-490) as LPC with shift 0
        order = (int)type - 8;
        L.shift = 0;
        if (!read_warmup<KIND, M>(L, rd, pr, order)) return;
        if (order == 1) pr.template set_coef<0>(1);
        if (order == 2) {
            pr.template set_coef<0>(2);
            pr.template set_coef<1>(-1);
        }
        if (order == 3) {
            pr.template set_coef<0>(3);
            pr.template set_coef<1>(-3);
            pr.template set_coef<2>(1);
        }
        if (order == 4) {
            pr.template set_coef<0>(4);
            pr.template set_coef<1>(-6);
            pr.template set_coef<2>(4);
            pr.template set_coef<3>(-1);
        }
    } else if (type >= 32) {  // LPC (:499-520)
        order = (int)type - 31;
        if (!read_warmup<KIND, M>(L, rd, pr, order)) return;
        rd.ensure(2);
        const uint32_t pc = rd.read(4);
        if (pc == 15) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }  // u4 `+ 1` overflow (:508)
        const uint32_t prec = pc + 1;
        L.shift = (int)rd.read(5);  // unsigned u5 (:510)
        if (L.shift >= Kind<KIND>::W) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
        uint64_t sum_abs = 0;
        static_for<M>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            if (J < order) {
                rd.ensure(2);
                const int32_t cf = rd.read_signed(prec);
                sum_abs += (uint64_t)(cf < 0 ? -(int64_t)cf : cf);
                pr.template set_coef<J>(cf);
            }
        });
        L.unsafe = (sum_abs << (Kind<KIND>::SB - 1)) > safe_lpc_bound<KIND>();
    } else {
        set_err(L, rd, E_INVALID_SUBFRAME_HEADER);  // reserved (:542)
        return;
    }
    L.order = order;
    rd.ensure(2);
    read_residual_header<KIND>(L, rd);
    if (L.err) return;
    L.mode = M_PRED;
}

// Walk: same reads as parse_subframe + residuals, no samples (src/zflac.zig:426-541).
template <int KIND>
__device__ __forceinline__ void walk_subframe(LaneCtx& L, Rdr& rd) {
    const uint32_t h8 = rd.read(8);
    if (h8 >> 7) { set_err(L, rd, E_INVALID_SUBFRAME_HEADER); return; }
    const uint32_t type = (h8 >> 1) & 63;
    int wasted = 0;
    if (h8 & 1) {
        uint32_t u;
        if (!rd.unary(L.end, u)) { set_err(L, rd, E_END_OF_STREAM); return; }
        if (u + 1 >= 64) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
        wasted = (int)u + 1;
    }
    if (type == 0) {
        if (L.bps <= wasted) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
        rd.skip((uint32_t)(L.bps - wasted));
        L.mode = M_NONE;  // done
        return;
    }
    if (L.ubps <= wasted) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
    const uint32_t cb = (uint32_t)(L.ubps - wasted);
    if (type == 1) {
        rd.skip((uint64_t)L.bs * cb);
        L.mode = M_NONE;  // done
        return;
    }
    int order;
    if (type >= 8 && type <= 12) {
        order = (int)type - 8;
        rd.skip((uint64_t)order * cb);
    } else if (type >= 32) {
        order = (int)type - 31;
        rd.skip((uint64_t)order * cb);
        rd.ensure(2);
        const uint32_t pc = rd.read(4);
        if (pc == 15) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
        rd.read(5);
        rd.skip((uint64_t)order * (pc + 1));
    } else {
        set_err(L, rd, E_INVALID_SUBFRAME_HEADER);
        return;
    }
    L.order = order;
    rd.ensure(2);
    read_residual_header<KIND>(L, rd);
    L.mode = L.err ? M_NONE : M_PRED;
}

// ----------------------------------------------------------------------------------
// Output
// ----------------------------------------------------------------------------------
struct FrameCtx {
    uint64_t out_elem;  // absolute output element of sample 0, channel 0
    bool write;
    bool packed;        // aligned for the packed 16-byte stores
    uint32_t justify;
};

template <int KIND>
__device__ __forceinline__ void store_elem(void* out, uint64_t idx, int32_t v) {
    if constexpr (Kind<KIND>::ESZ == 1) reinterpret_cast<int8_t*>(out)[idx] = (int8_t)v;
    else if constexpr (Kind<KIND>::ESZ == 2) reinterpret_cast<int16_t*>(out)[idx] = (int16_t)v;
    else reinterpret_cast<int32_t*>(out)[idx] = v;
}

// lanes l and l^32: x0 = the lane-0..31 side's value, x1 = the lane-32..63 side's value
__device__ __forceinline__ void pair_values(int32_t v, int32_t& x0, int32_t& x1) {
    const auto r = __builtin_amdgcn_permlane32_swap((uint32_t)v, (uint32_t)v, false, false);
    x0 = (int32_t)r[0];
    x1 = (int32_t)r[1];
}

// Stereo decorrelation (src/zflac.zig:553-578) for lane channel c, c1m = c ? -1 : 0.
// mid/side: R = M - (S >> 1), L = R + S (= zflac's ((M<<1 | S&1) +- S) >> 1 exactly).
template <int DECOR>
__device__ __forceinline__ int32_t decorrelate(uint32_t code, int32_t c1m, int32_t x0, int32_t x1) {
    if constexpr (DECOR == D_MS) {
        return x0 - (x1 >> 1) + (x1 & ~c1m);
    } else if constexpr (DECOR == D_NONE) {
        return c1m ? x1 : x0;
    } else {
        // o = (x0 & m0) - ((x1 >> 1) & mh) + (x1 & mp) - (x1 & mn), masks per (code, channel):
        //   LR: c0 x0, c1 x1;  LS(8): c0 x0, c1 x0 - x1;  RS(9): c0 x0 + x1, c1 x1;
        //   MS(10): c0 x0 - (x1 >> 1) + x1, c1 x0 - (x1 >> 1). Arithmetic, not branches.
        const int32_t is_ls = -(int32_t)(code == 8), is_rs = -(int32_t)(code == 9), is_ms = -(int32_t)(code == 10);
        const int32_t is_lr = ~(is_ls | is_rs | is_ms);
        const int32_t m0 = ~(is_lr & c1m) & ~(is_rs & c1m);
        const int32_t mh = is_ms;
        const int32_t mp = (is_lr & c1m) | is_rs | (is_ms & ~c1m);
        const int32_t mn = is_ls & c1m;
        return (x0 & m0) - ((x1 >> 1) & mh) + (x1 & mp) - (x1 & mn);
    }
}

// Does zflac's stereo decorrelation of (x0, x1) overflow the SampleType for output channel
// c (src/zflac.zig:553-578: left/side and side/right in SampleType, mid/side @intCast)?
template <int KIND>
__device__ __forceinline__ bool decor_overflows(uint32_t code, int c, int32_t x0, int32_t x1) {
    int64_t v;
    if (code == 8) {
        if (!c) return false;
        v = (int64_t)x0 - x1;
    } else if (code == 9) {
        if (c) return false;
        v = (int64_t)x0 + x1;
    } else if (code == 10) {
        const int64_t mid = (int64_t)x0 * 2 + (x1 & 1);
        v = c ? (mid - x1) >> 1 : (mid + x1) >> 1;
    } else {
        return false;
    }
    return !fits_sb<KIND>(v);
}

// ----------------------------------------------------------------------------------
// Chunks. A chunk is L_ samples (a multiple of M and of 8) of every lane.
// ----------------------------------------------------------------------------------
// Generic chunk: every mode, warm-up, partition switches and escapes; scalar stores.
template <int KIND, int M, int L_, int LAY, bool WALK>
__device__ __forceinline__ void slow_chunk(LaneCtx& L, Rdr& rd, Pred<KIND, M>& pr, uint32_t base, const FrameCtx& fc,
                                  void* out, int nch, int c, int32_t c1m) {
    // Rolled over blocks of HM samples (the history ring's period): the generic path is
    // rare, and unrolling it over the whole chunk made it too big for the instruction cache
    constexpr int HM = hist_len<M>();
#pragma unroll 1
    for (uint32_t blk = 0; blk < (uint32_t)(L_ / HM); blk++) {
    static_for<HM>([&](auto uc) {
        constexpr int u = decltype(uc)::value;  // history slot: (blk * HM + u) % HM == u
        const uint32_t i = base + blk * HM + u;
        const bool act = L.mode != M_NONE && i < L.bs;
        int32_t val = 0;
        if (act) {
            rd.ensure(3);
            if (L.mode == M_CONST) {
                val = L.cval;
            } else if (L.mode == M_VERB) {
                const int64_t v = rd.read_signed_wide((uint32_t)L.cbps);
                if (!fits_sb<KIND>(v)) set_err(L, rd, E_OUT_OF_DOMAIN);  // rd_unencoded @intCast (:459)
                val = wrap_st<KIND>((int64_t)((uint64_t)v << L.wasted));
            } else {
                int32_t s;
                if (i < (uint32_t)L.order) {
                    s = pr.template value<u>();
                } else {
                    if (L.left == 0) {
                        if (L.parts_left == 0) set_err(L, rd, E_OUT_OF_DOMAIN);
                        else read_partition_header<KIND>(L, rd);
                    }
                    const int64_t r = residual_general<KIND>(L, rd);
                    L.left--;
                    if constexpr (WALK) {
                        s = 0;
                    } else {
                        const int64_t p = pr.template predict<u>(L.shift);
                        // exact r + prediction: InterType overflow (:531 `+=`) or a value
                        // outside the SampleType (:494,537 @intCast) is OutOfDomain
                        const int64_t sx = (int64_t)((uint64_t)r + (uint64_t)p);
                        if constexpr (KIND != 2)
                            if (L.unsafe && !pr.template partials_fit<u>(L.order)) L.dom = true;
                        if (!fits_sb<KIND>(sx)) L.dom = true;
                        s = add_inter<KIND>(r, p);
                        pr.template push<u>(s);
                    }
                }
                val = wrap_st<KIND>((int64_t)((uint64_t)(int64_t)s << L.wasted));
            }
        }
        if constexpr (!WALK) {
            int32_t o = val;
            if constexpr (LAY == LAY_STEREO) {
                int32_t x0, x1;
                pair_values(val, x0, x1);
                o = decorrelate<D_GEN>(L.chan_code, c1m, x0, x1);
                if (act && decor_overflows<KIND>(L.chan_code, c, x0, x1)) L.dcr = 1;
            }
            if (act && fc.write) store_elem<KIND>(out, fc.out_elem + (uint64_t)nch * i + c, o << fc.justify);
        }
    });
    }
}

// Per-lane channel-assignment masks for the packed generic decorrelation.
struct DecMasks {
    uint32_t ms, ls, r1, addl;
    __device__ __forceinline__ void init(uint32_t code) {
        ms = code == 10 ? ~0u : 0u;
        ls = code == 8 ? ~0u : 0u;
        const uint32_t rs = code == 9 ? ~0u : 0u;
        r1 = ~(ms | ls);  // LR and RS: R = x1
        addl = rs | ms;   // RS: L = x0 + x1; MS: L = R + x1
    }
};

// Stereo decorrelation (src/zflac.zig:553-578) of two samples: x0 / x1 = channel 0 / 1
// pairs, out L / R pairs. MS: R = M - (S >> 1), L = R + S; LS: R = L - S; RS: L = S + R.
// Every form is one i16 subtraction R = A - D and one addition L = E + F; `ovf` collects
// their signed-overflow bits (bits 15 and 31), i.e. zflac's SampleType overflow traps
// (:558,564 checked arithmetic, :573-574 @intCast). LR passes D = F = 0: no overflow.
template <int DECOR>
__device__ __forceinline__ void decorrelate2(uint32_t x0, uint32_t x1, const DecMasks& dm, uint32_t& Lp,
                                             uint32_t& Rp, uint32_t& ovf) {
    if constexpr (DECOR == D_MS) {
        decorrelate2_ms(x0, x1, Lp, Rp, ovf);
    } else {
        const uint32_t A = (x0 & ~dm.r1) | (x1 & dm.r1);
        const uint32_t D = (pk_sar1(x1) & dm.ms) | (x1 & dm.ls);
        const uint32_t r = as_u32(as_u16x2(A) - as_u16x2(D));
        const uint32_t E = (r & dm.ms) | (x0 & ~dm.ms);
        const uint32_t F = x1 & dm.addl;
        const uint32_t l = as_u32(as_u16x2(E) + as_u16x2(F));
        Rp = r;
        Lp = l;
        ovf |= ((A ^ D) & (A ^ r)) | (~(E ^ F) & (E ^ l));
    }
}

// v_ffbh_u32 with the hardware's result for 0 (0xFFFFFFFF); __builtin_clz(0) is undefined.
__device__ __forceinline__ uint32_t ffbh_raw(uint32_t x) {
    uint32_t r;
    asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// Rice codes of one bit-window step (src/zflac.zig:657-663). NC = 1: one code from the
// 32-bit peek, `lim` tracks the smallest peek (a peek below 2^k holds no whole code).
// NC = 2: two codes from the same peek, `lim` tracks the largest bit count of a step (more
// than 32 means the pair did not fit). Needs 1 <= k: with k >= 1 a peek of 0 yields a
// count above 32 through ffbh's 0xFFFFFFFF. Returns the bits consumed.
//
// RES (NC = 2, needs 2 <= k): zz receives the residuals themselves, zigzag included. With
// y = h << (q + 1) (the code's remainder at the top), zz >> 1 = (q << (k-1)) | (rem >> 1) is
// one v_alignbit of (q, y) by 33 - k, and -(zz & 1) one v_bfe_i32 of y at 32 - k: the
// residual is their xor, which the caller's add fuses into a v_xad. (k = 1 would need an
// alignbit by 32, which the hardware reads as 0.)
template <int NC, bool WALK, bool ESC, bool RES = false>
__device__ __forceinline__ uint32_t rice_step(uint32_t h, uint32_t k, uint32_t kp1, uint32_t& lim, uint32_t (&zz)[NC],
                                              bool esc, uint32_t escw, int32_t& escv) {
    if constexpr (NC == 1) {
        if constexpr (ESC) {
            // escape partition (src/zflac.zig:646-653): escw-bit signed values, escw = 0 -> zeros
            lim = esc ? lim : min(lim, h);
            const uint32_t q = ffbh_raw(h);
            const uint32_t len = esc ? escw : q + kp1;
            if constexpr (!WALK) {
                zz[0] = (q << k) | __builtin_amdgcn_ubfe(h, 32 - (q + kp1), k);
                escv = escw ? ((int32_t)h >> (32 - escw)) : 0;
            }
            return len;
        } else if constexpr (RES) {  // the residual itself (2 <= k), as in the pair form below
            static_assert(!WALK, "residual values are decode-only");
            lim = min(lim, h);  // a garbage y (q >= 31, h = 0) comes with a flagged peek
            const uint32_t q = ffbh_raw(h);
            const uint32_t y = h << ((q + 1u) & 31u);
            zz[0] = __builtin_amdgcn_alignbit(q, y, 33u - k) ^ (uint32_t)__builtin_amdgcn_sbfe((int)y, 32u - k, 1u);
            return q + kp1;
        } else {
            lim = min(lim, h);
            const uint32_t q = __builtin_clz(h);
            const uint32_t len = q + kp1;
            if constexpr (!WALK) zz[0] = (q << k) | __builtin_amdgcn_ubfe(h, 32 - len, k);
            return len;
        }
    } else if constexpr (RES) {
        static_assert(!WALK, "residual values are decode-only");
        // q >= 31 (or h = 0: q = ~0) makes y garbage, but then tot > 32 flags the step
        const uint32_t q1 = ffbh_raw(h);
        const uint32_t y1 = h << ((q1 + 1u) & 31u);
        const uint32_t g = (y1 << k) | 1u;  // the second code; bit 0 stops ffbh at 31
        const uint32_t q2 = ffbh_raw(g);
        const uint32_t y2 = g << ((q2 + 1u) & 31u);
        const uint32_t tot = q1 + q2 + 2u * kp1;
        lim = max(lim, tot);
        zz[0] = __builtin_amdgcn_alignbit(q1, y1, 33u - k) ^ (uint32_t)__builtin_amdgcn_sbfe((int)y1, 32u - k, 1u);
        zz[1] = __builtin_amdgcn_alignbit(q2, y2, 33u - k) ^ (uint32_t)__builtin_amdgcn_sbfe((int)y2, 32u - k, 1u);
        return tot;
    } else {
        const uint32_t q1 = ffbh_raw(h);
        const uint32_t l1 = q1 + kp1;
        const uint32_t g = (h << l1) | 1u;  // the second code; bit 0 stops ffbh at 31
        const uint32_t q2 = ffbh_raw(g);
        const uint32_t tot = l1 + q2 + kp1;
        lim = max(lim, tot);
        if constexpr (!WALK) {
            zz[0] = (q1 << k) | __builtin_amdgcn_ubfe(h, 32 - l1, k);
            zz[1] = (q2 << k) | __builtin_amdgcn_ubfe(h, 32 - tot, k);
        }
        return tot;
    }
}

// (m & a) | (~m & b) as one v_bfi_b32
__device__ __forceinline__ uint32_t bfi(uint32_t m, uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(a), "v"(b));
    return r;
}

// The walk's steps (k_walk, lengths only): nothing in a walk step can hide the latency of a
// ring read, so the walk keeps the window in registers: (w0, w1) = ring words an-2 and an-1
// at shift sh, wn = word an, wn1 = word an+1, and each step reads word an+2 for the step
// after it (its address does not depend on the step): step s's read is selected in only at
// the end of step s+1, a whole step after its issue. An advance (the sign of sh - n, as a
// mask) shifts the window by one word with v_bfi_b32 selects (v_cndmask on a borrow in VCC
// needs two wait states after the write, which a walk step has no independent work to fill).
// The ring holds the words byte-swapped. nb is rebuilt from the advances at the end. A step
// moves the window by at most one word: a longer (flagged) step leaves a wrong position,
// which the redo discards.
template <int L_, int NC, bool ESC, bool WARM>
__device__ __forceinline__ void walk_steps(Rdr& rd, uint32_t k, uint32_t kp1, uint32_t& lim, bool esc, uint32_t escw,
                                           uint32_t wu) {
    const uint32_t nb0 = rd.nb;
    const uint32_t t0 = nb0 << 3;  // slot bits of word an-1 (see Rdr); an-2 is one slot up
    uint32_t w1 = rd.lds_word(rd.ldsb() | (t0 & RING_SLOT_MASK));
    uint32_t w0 = rd.lds_word(rd.ldsb() | ((t0 + 256u) & RING_SLOT_MASK));
    uint32_t wn = rd.lds_word(rd.ldsb() | ((t0 - 256u) & RING_SLOT_MASK));
    uint32_t wn1 = rd.lds_word(rd.ldsb() | ((t0 - 512u) & RING_SLOT_MASK));
    uint32_t pa = t0 - 768u;  // slot bits of word an+2: 256 lower per advance
    uint32_t sh = nb0 & 31u;
    uint32_t m_prev = 0, nx_prev = 0;
    static_for<L_ / NC>([&](auto sc) {
        constexpr int u0 = decltype(sc)::value * NC;
        const uint32_t nx = rd.lds_word(rd.ldsb() | (pa & RING_SLOT_MASK));  // word an+2
        uint32_t zz[NC];
        int32_t escv = 0;
        uint32_t n = rice_step<NC, true, ESC>(__builtin_amdgcn_alignbit(w0, w1, sh), k, kp1, lim, zz, esc, escw, escv);
        if constexpr (WARM) n = (uint32_t)u0 < wu ? 0u : n;
        const uint32_t tu = sh - n;
        const uint32_t m = (uint32_t)((int32_t)tu >> 31);
        sh = tu & 31u;
        // word an+1 of this step's an (the previous step's read): the empty asm ties the read's
        // first use to this step's position, so its wait comes after this step's own read is
        // issued, a whole step after its own issue (left alone, the scheduler hoists the select
        // into the step that issued the read and waits for it there)
        asm("" : "+v"(nx_prev) : "v"(tu));
        wn1 = bfi(m_prev, nx_prev, wn1);
        w0 = bfi(m, w1, w0);
        w1 = bfi(m, wn, w1);
        wn = bfi(m, wn1, wn);
        // pa -= 256 on an advance: m shifted into place and added in one v_lshl_add_u32
        asm("v_lshl_add_u32 %0, %1, 8, %2" : "=v"(pa) : "v"(m), "v"(pa));
        m_prev = m;
        nx_prev = nx;
    });
    rd.nb = (nb0 & ~31u) - ((t0 - 768u - pa) >> 3) + sh;
}

// Fast chunk: every lane that is `lane_fast` is a predicted subframe with >= L_ Rice codes
// left in its partition, past its warm-up. Straight-line, fully unrolled, no branch: a code
// (or, for NC = 2, a pair of codes) longer than the 32-bit peek only raises `bad` (the
// caller redoes the chunk on the generic path). Lanes that are not fast decode garbage that
// the caller rolls back. 16-bit containers keep samples as the predictor's packed pairs:
// stereo decorrelation, shifts and interleave run once per 8 samples on i16 pairs.
// Value ranges: `vbad` = some sample left the SampleType (or, 32-bit containers, the
// prediction sum left i32); `ovf` = decorrelation overflow bits. The caller keeps both only
// when the chunk is not redone. (Fast lanes are `safe`: no partial LPC sum can overflow and
// |r| <= 2^30, so the 8/16-bit `r + prediction` below is exact in i32.)
// WARM (a subframe's first chunk, NC = 1): samples u < `wu` (= the predictor order) are the
// warm-up samples already in the history; they consume no bits and are only re-emitted.
// MIXED (NC = 1, with ESC): lanes may also be CONSTANT (no bits, the constant) or VERBATIM
// (cbps <= 32 bits per sample, src/zflac.zig:455-465) subframes; a verbatim value outside the
// SampleType sends the chunk back to the generic path (zflac fails at that read).
template <int KIND, int M, int L_, int LAY, int DECOR, bool WALK, int NC, bool ESC = false, bool WARM = false,
          bool MIXED = false, bool RES1 = false, bool WIDE = false>
__device__ __forceinline__ void fast_chunk(LaneCtx& L, Rdr& rd, Pred<KIND, M>& pr, uint32_t base, const FrameCtx& fc,
                                           void* out, int nch, int c, int32_t c1m, bool lane_fast, uint4* dummy,
                                           bool& bad, Pend& pd, StageOf<LAY>& sg, bool& vbad, uint32_t& ovf,
                                           uint32_t wu = 0) {
    static_assert(!WARM || NC == 1, "warm-up chunks decode one code per step");
    static_assert(!MIXED || (NC == 1 && ESC && !WALK), "mixed chunks: one value per step, decode only");
    // decode pairs take their residuals straight from rice_step (every fast lane has k >= 2)
    // (RES1: one-code chunks of the mono kernels in waves where every fast lane has k >= 2)
    static_assert(!RES1 || (NC == 1 && !ESC && !WARM && !MIXED && !WALK), "RES1: plain one-code decode chunks");
    constexpr bool RES = (NC == 2 && !WALK) || RES1;
    const bool is_verb = MIXED && L.mode == M_VERB, is_const = MIXED && L.mode == M_CONST;
    // 32-bit containers, stereo: the decorrelation runs in wrapping i32, which is exact
    // whenever zflac's result fits the SampleType; with 31- or 32-bit decorrelated samples
    // in the wave it can also overflow it (src/zflac.zig:558,564 checked, :573-574
    // @intCast), which the WIDE variant checks per sample. (WIDE is a template argument,
    // chosen once per chunk: a per-sample branch would cut the unrolled chunk into one
    // basic block per sample, and the scheduler could no longer overlap one sample's
    // older-history MACs with the previous sample's chain.)
    static_assert(!WIDE || (KIND == 2 && LAY == LAY_STEREO), "WIDE: 31/32-bit stereo only");
    constexpr bool wide = WIDE;
    const uint32_t vshift = 32u - (uint32_t)L.cbps;  // verbatim: top cbps bits of the peek
    bool vrange = false;                            // a verbatim value outside the SampleType
    const uint32_t k = L.k, kp1 = L.kp1;
    const int shift = L.shift;
    const uint32_t wasted = (uint32_t)L.wasted;
    const uint32_t justify = fc.justify;
#ifdef ZFLAC_ABL_NOSTORE  // timing ablation only: packed PCM stores go to the (coalesced) dummy slots
    const bool do_store = false;
#else
    const bool do_store = lane_fast && fc.write;
#endif
    constexpr bool PACK16 = KIND == 1 && LAY != LAY_MULTI;
    constexpr bool SHIFTS = DECOR != D_MS;  // D_MS is only chosen when no lane shifts
    DecMasks dm;
    if constexpr (DECOR == D_GEN) dm.init(L.chan_code);
    uint32_t pk[KIND == 2 ? 8 : 4];
    uint32_t pb = 0, pb2 = 0;  // 8-bit containers: samples of the dword being packed
    uint32_t lim = NC == 1 ? 0xFFFFFFFFu : 0u;
    int32_t vmax = 0, vmin = 0;  // range of the chunk's samples (8/16-bit containers)
    bool v32 = false;            // 32-bit containers: a sum outside i32
    // packed output of 8 samples: stored at once, except the chunk's last group, which stays
    // pending until after the next chunk-start wait (a store issued just before that wait
    // would expose its whole latency)
    auto emit = [&](auto last, uint4* p, uint4 v0, uint4 v1) {
        if constexpr (decltype(last)::value) {
            pd.p = p;
            pd.v0 = v0;
            pd.v1 = v1;
        } else {
            p[0] = v0;
            if constexpr (pend_two<KIND>()) p[1] = v1;
        }
    };
    // one sample: residual -> prediction -> history -> packed output every 8 samples
    auto sample = [&](auto uc, int64_t r, bool warm, int32_t vv) {
        constexpr int u = decltype(uc)::value;
        const uint32_t i = base + u;
        const int64_t p = pr.template predict<u>(shift);
        // a warm-up sample re-enters the history as itself (its pair's low half, s[-1] for
        // u = 0, only ever meets a zero coefficient); it was range-checked when read
        int32_t s;
        if constexpr (KIND == 2) {
            int64_t sx = (int64_t)((uint64_t)r + (uint64_t)p);
            if constexpr (WARM) sx = warm ? (int64_t)pr.template value<u>() : sx;
            if constexpr (MIXED) sx = (is_verb || is_const) ? (int64_t)vv : sx;
            v32 = v32 || sx != (int64_t)(int32_t)sx;
            s = (int32_t)sx;
        } else {
            int32_t sx = (int32_t)((uint32_t)(int32_t)r + (uint32_t)(int32_t)p);
            if constexpr (WARM) sx = warm ? pr.template value<u>() : sx;
            if constexpr (MIXED) sx = (is_verb || is_const) ? vv : sx;
            vmax = max(vmax, sx);
            vmin = min(vmin, sx);
            s = Kind<KIND>::W == 16 ? (int32_t)(int16_t)sx : sx;  // add_inter's InterType wrap
        }
        pr.template push<u>(s);
        if constexpr (PACK16) {
            if constexpr ((u & 1) == 1) pk[(u & 7) >> 1] = pr.template pair<u>();
            if constexpr ((u & 7) == 7) {
                if constexpr (SHIFTS) {
#pragma unroll
                    for (int j = 0; j < 4; j++) pk[j] = pk_shl(pk[j], wasted);
                }
                if constexpr (LAY == LAY_STEREO) {
                    // lanes 0-31 hold channel 0, lanes 32-63 channel 1 of samples i0..i0+7;
                    // after the swaps lanes 0-31 own samples 0-3, lanes 32-63 samples 4-7,
                    // element [0] channel 0 and [1] channel 1
                    const auto a = __builtin_amdgcn_permlane32_swap(pk[0], pk[2], false, false);
                    const auto b = __builtin_amdgcn_permlane32_swap(pk[1], pk[3], false, false);
                    uint32_t l0, r0, l1, r1;
                    decorrelate2<DECOR>(a[0], a[1], dm, l0, r0, ovf);
                    decorrelate2<DECOR>(b[0], b[1], dm, l1, r1, ovf);
                    if constexpr (SHIFTS) {
                        l0 = pk_shl(l0, justify);
                        r0 = pk_shl(r0, justify);
                        l1 = pk_shl(l1, justify);
                        r1 = pk_shl(r1, justify);
                    }
                    uint4 v;
                    v.x = __builtin_amdgcn_perm(r0, l0, 0x05040100u);
                    v.y = __builtin_amdgcn_perm(r0, l0, 0x07060302u);
                    v.z = __builtin_amdgcn_perm(r1, l1, 0x05040100u);
                    v.w = __builtin_amdgcn_perm(r1, l1, 0x07060302u);
                    // staged in LDS; the chunk is written back as 128-byte runs per frame
                    sg.put((uint32_t)((u >> 3) & 3), v);
                } else {
                    if constexpr (SHIFTS) {
#pragma unroll
                        for (int j = 0; j < 4; j++) pk[j] = pk_shl(pk[j], justify);
                    }
                    sg.put((uint32_t)((u >> 3) & 3), make_uint4(pk[0], pk[1], pk[2], pk[3]));  // mono: staged
                }
            }
        } else if constexpr (KIND == 2 && LAY != LAY_MULTI) {
            int32_t o = (int32_t)((uint32_t)s << wasted);
            if constexpr (LAY == LAY_STEREO) {
                int32_t x0, x1;
                pair_values(o, x0, x1);
                o = decorrelate<DECOR>(L.chan_code, c1m, x0, x1);
                if (wide) ovf |= decor_overflows<KIND>(L.chan_code, c, x0, x1) ? 1u : 0u;
            }
            pk[u & 7] = (uint32_t)o << justify;
            if constexpr ((u & 7) == 7) {
                const uint32_t i0 = i - 7;
                if constexpr (LAY == LAY_STEREO) {
                    // lanes 0-31: L0..L7, lanes 32-63: R0..R7 -> each half owns 4 L/R pairs
                    const auto a0 = __builtin_amdgcn_permlane32_swap(pk[0], pk[4], false, false);
                    const auto a1 = __builtin_amdgcn_permlane32_swap(pk[1], pk[5], false, false);
                    const auto a2 = __builtin_amdgcn_permlane32_swap(pk[2], pk[6], false, false);
                    const auto a3 = __builtin_amdgcn_permlane32_swap(pk[3], pk[7], false, false);
                    int32_t* dst = reinterpret_cast<int32_t*>(out) + fc.out_elem + 2ull * i0 + (c ? 8 : 0);
                    emit(std::integral_constant<bool, u == L_ - 1>{}, do_store ? reinterpret_cast<uint4*>(dst) : dummy,
                         make_uint4(a0[0], a0[1], a1[0], a1[1]), make_uint4(a2[0], a2[1], a3[0], a3[1]));
                } else {
                    int32_t* dst = reinterpret_cast<int32_t*>(out) + fc.out_elem + i0;
                    emit(std::integral_constant<bool, u == L_ - 1>{}, do_store ? reinterpret_cast<uint4*>(dst) : dummy,
                         make_uint4(pk[0], pk[1], pk[2], pk[3]), make_uint4(pk[4], pk[5], pk[6], pk[7]));
                }
            }
        } else if constexpr (KIND == 0 && LAY != LAY_MULTI) {
            // 8-bit containers, mono / stereo: bytes packed four to a dword, one 16-byte store
            // per 16 samples (per-sample byte stores made every sample a separate L2 write:
            // the 8-bit row ran at 0.015 of HBM). 8-bit samples are never justified, and
            // wasted < 8 here (parse_subframe), so the shift is exact in 32 bits.
            int32_t o = (int32_t)(int8_t)((uint32_t)s << wasted);
            if constexpr (LAY == LAY_STEREO) {
                int32_t x0, x1;
                pair_values(o, x0, x1);
                o = decorrelate<D_GEN>(L.chan_code, c1m, x0, x1);
                ovf |= fits_sb<KIND>(o) ? 0u : 1u;  // exact in i32 for 8-bit values
            }
            if constexpr ((u & 3) == 0) {
                pb = (uint32_t)o;
            } else if constexpr ((u & 3) == 1) {
                pb = __builtin_amdgcn_perm((uint32_t)o, pb, 0x0c0c0400u);  // bytes [s0, s1, 0, 0]
            } else if constexpr ((u & 3) == 2) {
                pb2 = (uint32_t)o;
            } else {
                pk[(u & 15) >> 2] = __builtin_amdgcn_perm(__builtin_amdgcn_perm((uint32_t)o, pb2, 0x0c0c0400u), pb,
                                                          0x05040100u);  // [s0, s1, s2, s3]
            }
            if constexpr ((u & 15) == 15) {
                const uint32_t i0 = i - 15;
                if constexpr (LAY == LAY_STEREO) {
                    // lanes 0-31 hold channel 0, lanes 32-63 channel 1 of samples i0..i0+15: after the
                    // swaps lanes 0-31 own samples 0-7, lanes 32-63 samples 8-15 of both channels
                    const auto a = __builtin_amdgcn_permlane32_swap(pk[0], pk[2], false, false);
                    const auto b = __builtin_amdgcn_permlane32_swap(pk[1], pk[3], false, false);
                    uint8_t* dst = reinterpret_cast<uint8_t*>(out) + fc.out_elem + 2ull * i0 + (c ? 16 : 0);
                    emit(std::integral_constant<bool, u == L_ - 1>{}, do_store ? reinterpret_cast<uint4*>(dst) : dummy,
                         make_uint4(__builtin_amdgcn_perm(a[1], a[0], 0x05010400u),
                                    __builtin_amdgcn_perm(a[1], a[0], 0x07030602u),
                                    __builtin_amdgcn_perm(b[1], b[0], 0x05010400u),
                                    __builtin_amdgcn_perm(b[1], b[0], 0x07030602u)),
                         make_uint4(0, 0, 0, 0));
                } else {
                    uint8_t* dst = reinterpret_cast<uint8_t*>(out) + fc.out_elem + i0;
                    emit(std::integral_constant<bool, u == L_ - 1>{}, do_store ? reinterpret_cast<uint4*>(dst) : dummy,
                         make_uint4(pk[0], pk[1], pk[2], pk[3]), make_uint4(0, 0, 0, 0));
                }
            }
        } else {  // 3..8 channels: element stores
            // (wasted < SampleType bits, parse_subframe: a 32-bit shift is exact below 32 bits)
            int32_t o = KIND == 2 ? wrap_st<KIND>((int64_t)((uint64_t)(int64_t)s << wasted))
                                  : wrap_st<KIND>((int64_t)(int32_t)((uint32_t)s << wasted));
            if constexpr (LAY == LAY_STEREO) {
                int32_t x0, x1;
                pair_values(o, x0, x1);
                o = decorrelate<D_GEN>(L.chan_code, c1m, x0, x1);
                ovf |= fits_sb<KIND>(o) ? 0u : 1u;  // exact in i32 for 8-bit values
            }
            if (do_store) store_elem<KIND>(out, fc.out_elem + (uint64_t)nch * i + c, (int32_t)((uint32_t)o << justify));
        }
    };
    // The ring reads of step s+1 are issued right after step s's consume, before step s's
    // samples (the scheduling fence keeps them there): the samples' arithmetic covers their
    // LDS latency, which would otherwise sit on the bit chain of every step.
    if constexpr (WALK) {
        walk_steps<L_, NC, ESC, WARM>(rd, k, kp1, lim, L.esc, L.escw, wu);
        const bool dry = rd.dry();
        if constexpr (NC == 1) bad |= lim < L.thr || dry;
        else bad |= lim > 32u || dry;
        return;
    }
    uint32_t whi, wlo;
    rd.fetch(whi, wlo);
    static_for<L_ / NC>([&](auto sc) {
        constexpr int u0 = decltype(sc)::value * NC;
        uint32_t zz[NC];
        int32_t escv = 0;
        int32_t vv = 0;
        uint32_t n;
        const bool warm = WARM && (uint32_t)u0 < wu;
        const uint32_t h = rd.join(whi, wlo);
        if constexpr (MIXED) {
            const uint32_t lim0 = lim;
            n = rice_step<NC, WALK, ESC>(h, k, kp1, lim, zz, L.esc, L.escw, escv);
            if constexpr (WARM) n = warm ? 0u : n;
            // a constant enters before its wasted-bits shift: pack-out shifts and wraps it back
            // to L.cval exactly (trunc((cval >> w) << w) = trunc(v << w))
            vv = is_const ? (L.cval >> L.wasted) : ((int32_t)h >> vshift);
            n = is_verb ? (uint32_t)L.cbps : (is_const ? 0u : n);
            lim = (is_verb || is_const) ? lim0 : lim;  // no Rice code in these lanes
            vrange = vrange || (is_verb && !fits_sb<KIND>(vv));
        } else {
            n = rice_step<NC, WALK, ESC, RES>(h, k, kp1, lim, zz, L.esc, L.escw, escv);
            if constexpr (WARM) n = warm ? 0u : n;
        }
        rd.consume(n);
        if constexpr (decltype(sc)::value + 1 < L_ / NC) {
            rd.fetch(whi, wlo);
            __builtin_amdgcn_sched_barrier(0x6);  // VALU / SALU may cross, the ring reads may not
        }
        if constexpr (!WALK) {
            int64_t r0 = RES ? (int64_t)(int32_t)zz[0] : zigzag<KIND>(zz[0]);
            if constexpr (ESC) r0 = L.esc ? (int64_t)escv : r0;
            sample(std::integral_constant<int, u0>{}, r0, warm, vv);
            if constexpr (NC == 2)
                sample(std::integral_constant<int, u0 + 1>{}, RES ? (int64_t)(int32_t)zz[1] : zigzag<KIND>(zz[1]), false, 0);
        }
    });
    const bool dry = rd.dry();  // the ring ran out of stored words: stale reads, redo the chunk
    if constexpr (NC == 1) bad |= lim < L.thr || dry || (MIXED && vrange);
    else bad |= lim > 32u || dry;
    if constexpr (KIND == 2) vbad = v32;
    else vbad = vmax > (1 << (Kind<KIND>::SB - 1)) - 1 || vmin < -(1 << (Kind<KIND>::SB - 1));
}

// Decode (WALK = false) or walk (WALK = true) one subframe per lane, chunk by chunk.
// WBR: the staged write-back goes through a buffer resource over `out_bytes` of `out`.
template <int KIND, int M, int LAY, bool WALK, bool MIX = false, bool WBR = false>
__device__ __forceinline__ void run_subframe(LaneCtx& L, Rdr& rd, const FrameCtx& fc, void* out, int nch, int c,
                                    int32_t c1m, uint32_t bs_max, void* dummy_base, uint32_t out_bytes = 0) {
    static_assert(!WBR || (!WALK && staged<KIND, LAY>()), "only the staged write-back has a resource form");
    constexpr int L_ = WALK ? CHUNK : DEC_CHUNK;
    static_assert(L_ % hist_len<M>() == 0 && L_ % 16 == 0, "a chunk holds whole history rings and output groups");
    uint4* const dummy = reinterpret_cast<uint4*>(dummy_base) + dummy_slot();
    Pend pd;
    pd.p = dummy;
    pd.v0 = pd.v1 = make_uint4(0, 0, 0, 0);
    StageOf<LAY> sg;
    sg.mask = 0;
    sg.base = 0;
    sg.q0 = (threadIdx.x >> 6) * STAGE_QUADS;
    // (in VGPRs: as a wave-uniform kernel argument it stayed part of the 16-SGPR tuple of the
    // argument load, which the allocator spilled to VGPR lanes and restored with 16 v_readlane
    // at every chunk start's write-back)
    // (the resource form holds four SGPRs instead: made from values read with v_readfirstlane
    // once per subframe, which the allocator cannot fetch again from the argument tuple)
    if constexpr (WBR) {
        const uint64_t o = reinterpret_cast<uintptr_t>(out);
        // (each half widened as unsigned: the builtin returns int, and a sign-extended low half
        // would set every high bit of a pointer whose bit 31 is set)
        const uint64_t ou = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(o >> 32)) << 32) |
                            (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)o);
        sg.rs = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(ou), (short)0,
                                                  (int)__builtin_amdgcn_readfirstlane(out_bytes), BUFFER_RSRC_WORD3);
    } else {
        uint64_t outv = reinterpret_cast<uintptr_t>(out);
        asm volatile("" : "+v"(outv));
        sg.out = reinterpret_cast<guint4*>(outv);
    }
    if constexpr (!WALK && staged<KIND, LAY>()) {
#pragma unroll
        for (int t = 0; t < 4; t++)  // frame row_frame(t)'s output, in quads (fc.packed: < 2^32)
            sg.gq[t] = (uint32_t)__shfl((int)(uint32_t)(fc.out_elem / 8u), (int)StageOf<LAY>::row_frame(t)) +
                       (StageOf<LAY>::lane() & (StageOf<LAY>::PIECES - 1u));
    }
    Pred<KIND, M> pr;
    if constexpr (WALK) {
        pr.clear();
    } else {
        if (L.mode != M_NONE) parse_subframe<KIND, M>(L, rd, pr);
        else pr.clear();
    }
    const bool need_pack = !WALK && LAY != LAY_MULTI;  // packed 16-byte stores need aligned frames
    // the subframe's fixed fast-path conditions folded into one per-lane bound (a chunk is fast
    // only if it ends by it): packable output, safe coefficients. (As separate lane masks they
    // were spilled to VGPR lanes and read back at every chunk.)
    const uint32_t fast_bs = ((!need_pack || fc.packed) && !L.unsafe) ? L.bs : 0u;
    // Nothing in flight on loop entry (once per subframe): otherwise the entry edge, where
    // the staged loads are the youngest memory ops, forces vmcnt(0) at every top-up.
    __builtin_amdgcn_s_waitcnt(0);
    uint32_t pair_cool = 0;  // wave-uniform: chunks left before pairs are tried again
    // Adaptive pair back-off (mono kernels): 8, 16, .., 128 chunks as pair failures repeat.
    // Long residual tails (e.g. C2's k = 4 partitions) put a too-long pair in nearly every
    // 64-lane chunk, and each redo on the generic path costs ~6 fast chunks. The stereo
    // kernels keep a fixed 8: the extra wave-uniform state measured 1-3 % slower there.
    constexpr bool BACKOFF = LAY == LAY_MONO;
    uint32_t pair_fail = 0;  // wave-uniform: pair chunks redone since the last good one
#ifdef ZFLAC_PROBE  // timing-probe build (tools/probe.sh): cycles per chunk phase, per kernel
    unsigned long long* const probe =
        reinterpret_cast<unsigned long long*>(reinterpret_cast<uint8_t*>(dummy_base) + DUMMY_BYTES) + (WALK ? 0 : 8);
    uint64_t pr_top = 0, pr_fast = 0, pr_slow = 0, pr_n = 0, pr_nfast = 0, pr_redo = 0, pr_pair = 0, pr_pair_redo = 0;
#endif
    auto chunk = [&](uint32_t base, auto set) __attribute__((always_inline)) {
#ifdef ZFLAC_PROBE
        const uint64_t p0 = __builtin_amdgcn_s_memtime();
#endif
        topup_st<KIND, LAY, WALK, WBR>(rd, pd, sg, dummy);
        sg.mask = 0;  // flushed
#ifdef ZFLAC_PROBE
        const uint64_t p1 = __builtin_amdgcn_s_memtime();
#endif
        if (L.mode == M_PRED && base < L.bs && base >= (uint32_t)L.order && L.left == 0 && L.parts_left > 0)
            read_partition_header<KIND>(L, rd);
        if (L.mode != M_NONE && rd.pos() > L.end) set_err(L, rd, E_END_OF_STREAM);
        const bool active = L.mode != M_NONE && base < L.bs;
        // The first chunk is fast too: its warm-up samples are re-emitted from the history.
        uint32_t wu;  // warm-up samples in this chunk
        bool lane_fast;
        if constexpr (MIX) {  // constant / verbatim lanes ride along in the mixed variant
            wu = base == 0 && L.mode == M_PRED ? (uint32_t)L.order : 0u;
            const bool pred_ok = L.mode == M_PRED && L.left + wu >= (uint32_t)L_ && !L.unsafe;
            const bool cv_ok = L.mode == M_CONST || (L.mode == M_VERB && L.cbps <= 32);
            lane_fast = active && base + L_ <= L.bs && (pred_ok || cv_ok) && (!need_pack || fc.packed);
        } else {
            wu = base == 0 ? (uint32_t)L.order : 0u;
            lane_fast = active && base + L_ <= fast_bs && L.mode == M_PRED && L.left + wu >= (uint32_t)L_;
        }
        const bool need_slow = active && !lane_fast;
        bool redo = __builtin_amdgcn_ballot_w64(need_slow) != 0;
#ifdef ZFLAC_PROBE
        bool was_pair = false;
#endif
        if (!redo) {
            // snapshot of the lane's bit position and predictor history: idle lanes get their
            // position back; a long code anywhere sends the whole wave back to redo the chunk
            const uint32_t k_nb = rd.nb;
            const Pred<KIND, M> k_pr = pr;
            if constexpr (!WALK) {
                // frames whose staged output goes back to memory at the next chunk start;
                // cleared again if the chunk is redone
                sg.mask = (typename StageOf<LAY>::Mask)__builtin_amdgcn_ballot_w64(lane_fast && fc.write);
                sg.base = base;
            }
            bool bad = false;
            bool vbad = false;
            uint32_t ovf = 0;
            // two Rice codes per bit-window step when every fast lane has 1 <= k <= PAIR_KMAX
            constexpr bool PAIRS = WALK || KIND == 1;
            // (decode: k >= 2, for rice_step's residual form; the walk takes k = 1 too)
            const bool pairs = PAIRS && pair_cool == 0 && base != 0 &&
                               __builtin_amdgcn_ballot_w64(lane_fast && (L.k < (WALK ? 1u : 2u) || L.k > PAIR_KMAX ||
                                                                         L.esc)) == 0;
            const bool escs = __builtin_amdgcn_ballot_w64(lane_fast && L.esc) != 0;
            // 31/32-bit stereo with decorrelation: the per-sample overflow-checking variant
            // (the generic one-code form), see fast_chunk
            bool wide = false;
            if constexpr (KIND == 2 && LAY == LAY_STEREO)
                wide = __builtin_amdgcn_ballot_w64(lane_fast && L.bps > 30 && L.chan_code >= 8) != 0;
            auto fast = [&](auto decor, auto nc, auto esc) {
                fast_chunk<KIND, M, L_, LAY, decltype(decor)::value, WALK, decltype(nc)::value, decltype(esc)::value>(
                    L, rd, pr, base, fc, out, nch, c, c1m, lane_fast, dummy, bad, pd, sg, vbad, ovf);
            };
            using DGen = std::integral_constant<int, D_GEN>;
            using DMs = std::integral_constant<int, D_MS>;
            using One = std::integral_constant<int, 1>;
            using Two = std::integral_constant<int, PAIRS ? 2 : 1>;
            using Esc = std::true_type;
            using NoEsc = std::false_type;
            bool mixed = false;
            if constexpr (MIX) {
                mixed = __builtin_amdgcn_ballot_w64(lane_fast && L.mode != M_PRED) != 0;
                if (mixed) {  // constant / verbatim lanes: one value per step, generic forms
                    auto mixed_chunk = [&](auto widec) {
                        constexpr bool W = decltype(widec)::value;
                        if (base == 0)
                            fast_chunk<KIND, M, L_, LAY, D_GEN, WALK, 1, true, true, true, false, W>(
                                L, rd, pr, base, fc, out, nch, c, c1m, lane_fast, dummy, bad, pd, sg, vbad, ovf, wu);
                        else
                            fast_chunk<KIND, M, L_, LAY, D_GEN, WALK, 1, true, false, true, false, W>(
                                L, rd, pr, base, fc, out, nch, c, c1m, lane_fast, dummy, bad, pd, sg, vbad, ovf, wu);
                    };
                    if constexpr (KIND == 2 && LAY == LAY_STEREO) {
                        if (wide) mixed_chunk(std::true_type{});
                        else mixed_chunk(std::false_type{});
                    } else {
                        mixed_chunk(std::false_type{});
                    }
                }
            }
            if (MIX && mixed) {
            } else if (KIND == 2 && LAY == LAY_STEREO && wide) {
                // (the generic one-code form, escapes and warm-up included, with the checks)
                if constexpr (KIND == 2 && LAY == LAY_STEREO) {
                    if (base == 0)
                        fast_chunk<KIND, M, L_, LAY, D_GEN, WALK, 1, true, true, false, false, true>(
                            L, rd, pr, base, fc, out, nch, c, c1m, lane_fast, dummy, bad, pd, sg, vbad, ovf, wu);
                    else
                        fast_chunk<KIND, M, L_, LAY, D_GEN, WALK, 1, true, false, false, false, true>(
                            L, rd, pr, base, fc, out, nch, c, c1m, lane_fast, dummy, bad, pd, sg, vbad, ovf, wu);
                }
            } else if (base == 0) {  // warm-up chunk: one code per step, generic forms
                fast_chunk<KIND, M, L_, LAY, D_GEN, WALK, 1, true, true>(L, rd, pr, base, fc, out, nch, c, c1m,
                                                                        lane_fast, dummy, bad, pd, sg, vbad, ovf, wu);
            } else if (escs) {
                fast(DGen{}, One{}, Esc{});  // escape partitions: one value per step
            } else if constexpr (WALK || LAY == LAY_MULTI || KIND == 0 || (KIND == 2 && LAY == LAY_MONO)) {
                if (PAIRS && pairs) fast(DGen{}, Two{}, NoEsc{});
                else fast(DGen{}, One{}, NoEsc{});
            } else {
                // D_MS: mid/side everywhere (16-bit: and no wasted / justify shifts)
                bool ms = true;
                if constexpr (LAY == LAY_STEREO) ms = __builtin_amdgcn_ballot_w64(lane_fast && L.chan_code != 10) == 0;
                if constexpr (KIND == 1)
                    ms = ms && __builtin_amdgcn_ballot_w64(lane_fast && (L.wasted != 0 || fc.justify != 0)) == 0;
                if (ms) {
                    if (PAIRS && pairs) {
                        fast(DMs{}, Two{}, NoEsc{});
                    } else if constexpr (LAY == LAY_MONO) {
                        // mono one-code chunks (C2 after its pair back-off): the residual form
                        if (__builtin_amdgcn_ballot_w64(lane_fast && L.k < 2u) == 0)
                            fast_chunk<KIND, M, L_, LAY, D_MS, WALK, 1, false, false, false, true>(
                                L, rd, pr, base, fc, out, nch, c, c1m, lane_fast, dummy, bad, pd, sg, vbad, ovf);
                        else
                            fast(DMs{}, One{}, NoEsc{});
                    } else {
                        fast(DMs{}, One{}, NoEsc{});
                    }
                } else {
                    if (PAIRS && pairs) fast(DGen{}, Two{}, NoEsc{});
                    else fast(DGen{}, One{}, NoEsc{});
                }
            }
            redo = __builtin_amdgcn_ballot_w64(bad && lane_fast) != 0;
            // a pair chunk that had to be redone (codes too long for two per window): one code
            // per step for the next chunks of this subframe (BACKOFF above)
            if (PAIRS && pairs && redo) {
                pair_cool = BACKOFF ? 8u << (pair_fail < 4u ? pair_fail : 4u) : 8u;
                pair_fail++;
            } else if (BACKOFF && PAIRS && pairs) {
                pair_fail = 0;
            } else if (pair_cool) {
                pair_cool--;
            }
            // (wave-uniform: in SGPRs, not a VGPR updated with v_cndmask every chunk)
            pair_cool = __builtin_amdgcn_readfirstlane(pair_cool);
            if constexpr (BACKOFF) pair_fail = __builtin_amdgcn_readfirstlane(pair_fail);
#ifdef ZFLAC_PROBE
            was_pair = PAIRS && pairs && !escs && base != 0;
#endif
            if (redo || !lane_fast) {
                rd.nb = k_nb;
            }
            if (redo) {
                pr = k_pr;
                pd.p = dummy;  // the redo rewrites the chunk: drop its pending quads
                sg.mask = 0;   // ... and its staged chunk
            }
            if (!redo && lane_fast) {
                if (!MIX || L.mode == M_PRED) L.left -= L_ - wu;
                L.dom = L.dom || vbad;
                L.dcr |= ovf & (KIND == 1 ? 0x80008000u : 1u);
            }
        }
#ifdef ZFLAC_PROBE
        const uint64_t p2 = __builtin_amdgcn_s_memtime();
        const bool was_fast = !__builtin_amdgcn_ballot_w64(active && !lane_fast);
#endif
        if (redo) slow_chunk<KIND, M, L_, LAY, WALK>(L, rd, pr, base, fc, out, nch, c, c1m);
#ifdef ZFLAC_PROBE
        const uint64_t p3 = __builtin_amdgcn_s_memtime();
        pr_top += p1 - p0;
        pr_fast += p2 - p1;
        pr_slow += p3 - p2;
        pr_n += 1;
        pr_nfast += was_fast ? 1 : 0;
        pr_redo += (was_fast && redo) ? 1 : 0;
        pr_pair += was_pair ? 1 : 0;
        pr_pair_redo += (was_pair && redo) ? 1 : 0;
#endif
    };
    for (uint32_t base = 0; base < bs_max; base += L_) chunk(base, std::integral_constant<int, 0>{});
#ifdef ZFLAC_PROBE
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(probe + 0, (unsigned long long)pr_top);
        atomicAdd(probe + 1, (unsigned long long)pr_fast);
        atomicAdd(probe + 2, (unsigned long long)pr_slow);
        atomicAdd(probe + 3, (unsigned long long)pr_n);
        atomicAdd(probe + 4, (unsigned long long)pr_nfast);
        atomicAdd(probe + 5, (unsigned long long)pr_redo);
        atomicAdd(probe + 6, (unsigned long long)pr_pair);
        atomicAdd(probe + 7, (unsigned long long)pr_pair_redo);
    }
#endif
    if constexpr (!WALK) {
        if constexpr (staged<KIND, LAY>()) {
            sg.template flush<WBR>(dummy);
        } else {
            pd.flush(pend_two<KIND>());
        }
    }
    if (L.mode != M_NONE && rd.pos() > L.end) set_err(L, rd, E_END_OF_STREAM);
}

// Per-lane frame setup shared by k_walk and k_decode: the wave's input window, the frame
// header (exact zflac semantics, src/zflac.zig:343-405), the lane reader's base and the
// output placement. `L.ubps` is left to the caller (it depends on the channel).
struct FrameSetup {
    LaneCtx L;
    FrameCtx fc;
    uint64_t pos;
    uint32_t hdr_info, rate, start;
    bool frame_ok;
};

__device__ __forceinline__ bool is_side_channel(uint32_t code, int c) {  // src/zflac.zig:436-441
    return (code == 8 && c == 1) || (code == 9 && c == 0) || (code == 10 && c == 1);
}

// `dec`: k_decode's LDS layout (junk slots in the wave's output stage), else k_walk's.
__device__ __forceinline__ void setup_frame(const DecodeArgs& a, uint32_t f, bool fvalid, int nch, uint32_t lds_lane,
                                            int esz, Rdr& rd, FrameSetup& s, bool dec) {
    s.L = LaneCtx{};
    s.fc = FrameCtx{};
    s.pos = 0;
    s.hdr_info = s.rate = s.start = 0;
    s.frame_ok = false;
    rd.nb = NB0;
    rd.wr = 0;
#pragma unroll
    for (int q = 0; q < 6; q++) rd.stg[q] = make_uint4(0, 0, 0, 0);
    rd.sv = false;
    // The wave's input window starts at its lowest frame position; lanes address it
    // with 32-bit offsets (buffer loads: out-of-range offsets read zeros, no traffic).
    uint64_t wmin = fvalid ? (a.c_pos[f] & ~(uint64_t)15) : ~0ull;
    for (int o = 32; o > 0; o >>= 1) wmin = min(wmin, (uint64_t)__shfl_xor((unsigned long long)wmin, o));
    const uint64_t wbase = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(wmin >> 32)) << 32) |
                           __builtin_amdgcn_readfirstlane((uint32_t)wmin);
    const uint64_t wlen = a.in_size > wbase ? a.in_size - wbase : 0;
    rd.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.in) + wbase, (short)0,
                                              (int)(wlen > 0x7FFFFFF0ull ? 0x7FFFFFF0ull : wlen), BUFFER_RSRC_WORD3);
    rd.lofs = 0x80000000u;
    rd.qa = 0;
    rd.qmax = 0;
    rd.lds = lds_lane;
    rd.junk = (blockDim.x >> 6) * RING_WAVE_WORDS + (lds_lane / RING_WAVE_WORDS) * (dec ? STAGE_QUADS * 4 : JUNK_WAVE_WORDS) +
              (lds_lane & 63u);
    if (!fvalid) return;
    LaneCtx& L = s.L;
    s.pos = a.c_pos[f];
    const uint64_t pos = s.pos;
    const StreamDesc S = a.streams[a.c_stream[f]];
    const FrameHdr h = parse_frame_fields(a.in + pos, S.in_end > pos ? S.in_end - pos : 0, S.si_rate);
    s.rate = h.rate;
    s.hdr_info = ((h.bs - 1) & 0xFFFFu) | (h.chan_code << 16) | (h.dcode << 20);
    L.bs = h.bs;
    L.chan_code = h.chan_code;
    L.bps = depth_bits(h.dcode, S.si_bps);
    if (h.err) {
        L.err = h.err;
        s.hdr_info |= INFO_PRE_ERR;
    } else if (h.crc_eof) {
        L.err = E_END_OF_STREAM;
        s.hdr_info |= INFO_CRC_EOF;
    } else if (channels_count(h.chan_code) != nch) {
        L.err = E_INCONSISTENT_PARAMETERS;
    } else if (L.bps < 0) {
        L.err = E_OUT_OF_DOMAIN;  // reserved depth code: `unreachable` (:143)
    } else {
        s.frame_ok = true;
    }
    const uint64_t abase = pos & ~(uint64_t)15;
    const uint64_t end_bytes = S.in_end > abase ? S.in_end - abase : 0;
    L.end = end_bytes * 8 > 0xFFFF0000ull ? 0xFFFF0000u : (uint32_t)(end_bytes * 8);
    const uint64_t quads = (S.in_end + INPUT_PAD - abase) / 16;
    // a frame beyond the 2 GiB window reads zeros: its chain check then fails and
    // the stream goes to the sequential planner, whose probes are one frame each
    rd.lofs = abase - wbase < 0x7FFFFFF0ull ? (uint32_t)(abase - wbase) : 0x80000000u;
    rd.qmax = quads > 0x3FFFFFFull ? 0x3FFFFFFu : (uint32_t)quads - 1;
    rd.qa = (uint32_t)(abase >> 4) & 3u;  // (`in` itself is 256-byte aligned)
    s.start = ((uint32_t)(pos & 15) + h.hdr_len) * 8;
    const uint64_t rel = a.c_out[f] - S.out_base;
    const bool in_range = !S.valid_total || rel < S.total;
    s.fc.out_elem = a.c_out[f];
    s.fc.write = a.write && in_range && s.frame_ok && rel + (uint64_t)h.bs * nch <= S.out_cap;
    // packed 16-byte stores need the frame's first output byte 16-byte aligned (absolute
    // address: the sequential path decodes into a sub-range or an override buffer)
    // (and within the first 2^36 bytes of the buffer: the staged write-back of the stereo
    // fast path addresses 16-byte quads with 32-bit indices)
    s.fc.packed = ((reinterpret_cast<uintptr_t>(a.out) + s.fc.out_elem * (uint64_t)esz) & 15) == 0 &&
                  (s.fc.out_elem + 0x20000u) * (uint64_t)esz < (1ull << 36);
    s.fc.justify = S.justify;
}

// ----------------------------------------------------------------------------------
// k_walk: subframe c+1 starts where subframe c ends (src/zflac.zig:425-541 read order), so
// before any lane can decode subframe c >= 1 the bit length of subframes 0..c-1 must be
// known. One lane per frame (64 frames per wave) reads subframes 0..nch-2 without
// producing samples (header, warm-up / coefficient skips, Rice lengths only) and records
// where each following subframe starts, as a bit offset from the frame's 16-byte base.
// ----------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(WALK_THREADS, 2) void k_walk(DecodeArgs a) {
#ifdef ZFLAC_DEC_PRIO
    __builtin_amdgcn_s_setprio(ZFLAC_DEC_PRIO);
#endif
    const int lane = threadIdx.x & 63;
    const int wave_in_block = threadIdx.x >> 6;
    const uint32_t wave = (blockIdx.x * WALK_THREADS + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * WALK_THREADS) >> 6;
    const int nch = a.nch;
    uint32_t nframes = a.n_frames ? *a.n_frames : a.n_frames_host;
    if (nframes > a.cap) nframes = a.cap;
    const uint32_t lds_lane = (uint32_t)(wave_in_block * RING_WAVE_WORDS + lane);
    for (uint32_t g0 = wave * 64u; g0 < nframes; g0 += nwaves * 64u) {
        const uint32_t f = g0 + (uint32_t)lane;
        const bool fvalid = f < nframes;
        Rdr rd;
        FrameSetup s;
        setup_frame(a, f, fvalid, nch, lds_lane, Kind<KIND>::ESZ, rd, s, false);
        uint32_t start = s.start;
        for (int r = 0; r + 1 < nch; r++) {
            LaneCtx W = s.L;
            W.ubps = W.bps + (is_side_channel(W.chan_code, r) ? 1 : 0);
            W.mode = M_NONE;
            if (s.frame_ok) {
                W.mode = M_PRED;
                rd.init(start);
                walk_subframe<KIND>(W, rd);
            }
            uint32_t wbs = W.mode != M_NONE ? W.bs : 0;
            for (int o = 32; o > 0; o >>= 1) wbs = max(wbs, (uint32_t)__shfl_xor((int)wbs, o));
            if (wbs) run_subframe<KIND, 4, LAY_MULTI, true>(W, rd, s.fc, a.out, nch, r, 0, wbs, a.dummy);
            start = s.frame_ok ? rd.pos() : 0u;
            if (fvalid) a.sub_start[(uint64_t)f * MAX_CH + r + 1] = start;
        }
    }
}

// ----------------------------------------------------------------------------------
// k_decode
// ----------------------------------------------------------------------------------
// One kernel per history bucket MB (4, 8, 16, 32 >= the largest predictor order of the
// wave's subframes), launched back to back: a wave decodes its frames only in the launch
// of its bucket. Register allocation is per kernel, so the order-8 code (C3/C5) is not
// sized for the order-32 history. Waves with CONSTANT or VERBATIM subframes among their
// lanes go to the MIX kernels (MB 8 or 32), whose fast path also carries those lanes; the
// pure kernels keep their registers for the predicted-only fast path.
// (Waves per SIMD the register allocation must allow: two for the 16-bit kernels and the small
// 8-bit / 32-bit stereo ones, which fit in 256 VGPRs; one for MB = 32 and MIX, and (round 6) for
// the 3..8-channel kernels and the larger 8-bit and 32-bit stereo buckets, which spilled 18-88
// VGPRs to scratch at two waves per SIMD (tools/kmeta.sh). A single-stream launch of 32k
// frames holds about one wave per SIMD anyway.)
template <int KIND, int LAY, int MB, bool MIX>
__host__ __device__ constexpr int dec_min_waves() {
    if (MB == 32 || MIX || LAY == LAY_MULTI) return 1;
    if (KIND == 0 && MB > 8) return 1;
    if (KIND == 2 && LAY == LAY_STEREO && MB > 4) return 1;
    return 2;
}
// WBR (16-bit stereo / mono only): the staged PCM goes back through a buffer resource
// (Stage::store_rsrc); chosen per launch by the host (DecodeArgs::wb_bytes).
template <int KIND, int LAY, int MB, bool MIX, bool WBR = false>
__global__ __launch_bounds__(DEC_THREADS, (dec_min_waves<KIND, LAY, MB, MIX>())) void k_decode(DecodeArgs a) {
#ifdef ZFLAC_DEC_PRIO
    // (experiment) decode waves ahead of the md5 hub's waves on a shared SIMD
    __builtin_amdgcn_s_setprio(ZFLAC_DEC_PRIO);
#endif
    const int lane = threadIdx.x & 63;
    const int wave_in_block = threadIdx.x >> 6;
    const uint32_t wave = (blockIdx.x * DEC_THREADS + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * DEC_THREADS) >> 6;
    const int nch = LAY == LAY_STEREO ? 2 : (LAY == LAY_MONO ? 1 : a.nch);
    const int F = 64 / nch;
    const int c = lane / F;
    const int j = lane - c * F;
    const bool lane_ok = c < nch;
    const int32_t c1m = c ? -1 : 0;
    uint32_t nframes = a.n_frames ? *a.n_frames : a.n_frames_host;
    if (nframes > a.cap) nframes = a.cap;
    const uint32_t lds_lane = (uint32_t)(wave_in_block * RING_WAVE_WORDS + lane);

    constexpr bool FIRST = MB == 8 && !MIX;  // launched first: finds every group's bucket
    constexpr uint32_t MIX_BIT = 64;
    // the `rest` launch (only of k_decode<*, *, 32, true>): every group whose bucket has no
    // launch of its own (a bucket the host did not predict)
    const bool rest = MB == 32 && MIX && a.rest;
    for (uint32_t g0 = wave * (uint32_t)F; g0 < nframes; g0 += nwaves * (uint32_t)F) {
        if constexpr (!FIRST) {  // wave-uniform, one scalar load
            const uint32_t gmb = a.group_mb[g0 / (uint32_t)F];
            if (rest) {
                if (gmb == 8u || (a.full_mask & bucket_bit(gmb & ~MIX_BIT, (gmb & MIX_BIT) != 0))) continue;
            } else if (gmb != (uint32_t)MB + (MIX ? MIX_BIT : 0u)) {
                continue;
            }
        }
        const uint32_t f = g0 + (uint32_t)j;
        const bool fvalid = lane_ok && f < nframes;
        Rdr rd;
        FrameSetup s;
        setup_frame(a, f, fvalid, nch, lds_lane, Kind<KIND>::ESZ, rd, s, true);
        LaneCtx& L = s.L;
        const FrameCtx& fc = s.fc;
        L.ubps = L.bps + (is_side_channel(L.chan_code, c) ? 1 : 0);
        // subframe c >= 1 starts where k_walk found subframe c-1 to end
        uint32_t start = s.start;
        if (c > 0 && s.frame_ok) start = a.sub_start[(uint64_t)f * MAX_CH + c];
        // ---- decode --------------------------------------------------------------------
        if (s.frame_ok) {
            L.mode = M_PRED;  // active marker until the subframe header is parsed
            rd.init(start);
        }
        uint32_t ord = 0, bs_act = 0;
        bool cv = false;
        if (L.mode != M_NONE) {  // peek the subframe type (header bits 1..6) to size the history
            const uint32_t t = (rd.hi() >> 25) & 63;
            ord = (t >= 32) ? t - 31 : ((t >= 8 && t <= 12) ? t - 8 : 0);
            cv = t <= 1;  // CONSTANT / VERBATIM
            bs_act = L.bs;
        }
        for (int o = 32; o > 0; o >>= 1) {
            ord = max(ord, (uint32_t)__shfl_xor((int)ord, o));
            bs_act = max(bs_act, (uint32_t)__shfl_xor((int)bs_act, o));
        }
        const bool mix = __builtin_amdgcn_ballot_w64(cv) != 0;
        const uint32_t mb = mix ? (ord <= 8 ? 8u + MIX_BIT : 32u + MIX_BIT)
                                : (ord <= 4 ? 4u : (ord <= 8 ? 8u : (ord <= 12 ? 12u : (ord <= 16 ? 16u : 32u))));
        if constexpr (FIRST) {
            if (lane == 0) {
                a.group_mb[g0 / (uint32_t)F] = mb;
                if (a.bucket_used) atomicOr(a.bucket_used, bucket_bit(mb & ~MIX_BIT, (mb & MIX_BIT) != 0));
            }
        }
        if (!rest && mb != (uint32_t)MB + (MIX ? MIX_BIT : 0u)) continue;  // another launch decodes this wave's frames
        run_subframe<KIND, MB, LAY, false, MIX, WBR>(L, rd, fc, a.out, nch, c, c1m, bs_act, a.dummy, a.wb_bytes);

        // ---- frame end and record -----------------------------------------------------
        uint32_t endbits = (rd.pos() + 7) & ~7u;  // alignToByte (:546)
        // the subframe's error: a read error first, else a value out of range (zflac reads
        // all residuals before it predicts)
        int lerr = L.err ? L.err : (L.dom ? (int)E_OUT_OF_DOMAIN : 0);
        if (s.frame_ok && !lerr && c == nch - 1 && endbits + 16 > L.end) lerr = E_END_OF_STREAM;  // CRC-16 (:548)
        int ferr = 0;  // first error in channel order
        uint32_t dcr = 0;
        for (int cc = nch - 1; cc >= 0; cc--) {
            const int e = __shfl(lerr, cc * F + j);
            if (e) ferr = e;
            dcr |= (uint32_t)__shfl((int)L.dcr, cc * F + j);
        }
        if (LAY == LAY_STEREO && !ferr && dcr) ferr = E_OUT_OF_DOMAIN;  // decorrelation, after the CRC (:553)
        const uint32_t last_end = (uint32_t)__shfl((int)endbits, (nch - 1) * F + j);
        if (fvalid && c == 0) {
            a.c_err[f] = ferr;
            a.c_info[f] = s.hdr_info;
            a.c_rate[f] = s.rate;
            a.c_end[f] = (s.pos & ~(uint64_t)15) + last_end / 8 + 2;
        }
    }
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) of one kernel, once per device: the
// attribute belongs to the kernel's instance on the current device, so a process that
// decodes on several devices sets it on each (`done`: one bit per device already set).
__host__ inline hipError_t set_lds_limit(std::atomic<uint64_t>& done, const void* fn, size_t bytes) {
    int dev = 0;
    if (const hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_acq_rel);
    return e;
}

template <int KIND>
hipError_t launch_walk_kind(const DecodeArgs& a, uint32_t max_frames, hipStream_t st) {
    static std::atomic<uint64_t> lds_set{0};
    if (const hipError_t e = set_lds_limit(lds_set, reinterpret_cast<const void*>(&k_walk<KIND>), WALK_LDS_BYTES);
        e != hipSuccess)
        return e;
    uint32_t waves = (max_frames + 63) / 64;
    uint32_t blocks = (waves + WALK_THREADS / 64 - 1) / (WALK_THREADS / 64);
    if (blocks > 8192) blocks = 8192;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL((k_walk<KIND>), dim3(blocks), dim3(WALK_THREADS), WALK_LDS_BYTES, st, a);
    return hipGetLastError();
}

template <int KIND, int LAY>
__host__ __forceinline__ dim3 decode_grid(const DecodeArgs& a, uint32_t max_frames) {
    const uint32_t F = 64 / (uint32_t)a.nch;
    uint32_t waves = (max_frames + F - 1) / F;
    uint32_t blocks = (waves + DEC_WAVES - 1) / DEC_WAVES;
    if (blocks > 8192) blocks = 8192;
    if (blocks == 0) blocks = 1;
    return dim3(blocks);
}

// Does bucket (mb, mix) get a launch of its own? Always for order 8 (it classifies every
// frame group), else when the host predicts it (DecodeArgs::full_mask; 0 = every bucket).
__host__ __forceinline__ bool bucket_launched(const DecodeArgs& a, uint32_t mb, bool mix) {
    return a.full_mask == 0 || (a.full_mask & bucket_bit(mb, mix)) || (mb == 8 && !mix);
}

// Pure (predicted-only) bucket kernels. Bucket 8 first: it records every frame group's
// bucket in a.group_mb for the others. The MIX kernels (launch_decode_mix) live in their own
// translation unit (decode_k*_*_mix.hip), so this code object holds only the pure kernels.
// A bucket the host does not predict costs no launch: its groups (if any) are decoded by
// the `rest` launch (launch_decode_mix with rest_only), which the host issues only after a
// run that needed it (each empty launch costs ~5 us of a ~0.55 ms step, and far more with
// several runs in flight, where it waits for LDS to dispatch).
// The staged write-back of a launch: through the buffer resource when the host offers one
// (DecodeArgs::wb_bytes != 0) and the kernel stages its PCM, else through the pointer.
template <int KIND, int LAY>
__host__ __forceinline__ bool wb_rsrc(const DecodeArgs& a) {
    return staged<KIND, LAY>() && a.wb_bytes != 0;
}

// One bucket kernel, either write-back form. Dynamic LDS above 64 KiB (four waves' rings and
// stages; the 32-bit-container units' larger rings) must be allowed per kernel.
template <int KIND, int LAY, int MB, bool MIX, bool WBR>
__host__ hipError_t launch_bucket_wb(const DecodeArgs& a, dim3 g, hipStream_t st) {
    if constexpr (DEC_LDS_BYTES > 64 * 1024) {
        static std::atomic<uint64_t> lds_set{0};
        if (const hipError_t e = set_lds_limit(lds_set, reinterpret_cast<const void*>(&k_decode<KIND, LAY, MB, MIX, WBR>),
                                               DEC_LDS_BYTES);
            e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL((k_decode<KIND, LAY, MB, MIX, WBR>), g, dim3(DEC_THREADS), DEC_LDS_BYTES, st, a);
    return hipSuccess;
}
template <int KIND, int LAY, int MB, bool MIX>
__host__ hipError_t launch_bucket(const DecodeArgs& a, dim3 g, hipStream_t st) {
    if constexpr (staged<KIND, LAY>()) {
        if (wb_rsrc<KIND, LAY>(a)) return launch_bucket_wb<KIND, LAY, MB, MIX, true>(a, g, st);
    }
    return launch_bucket_wb<KIND, LAY, MB, MIX, false>(a, g, st);
}

template <int KIND, int LAY>
hipError_t launch_decode_layout(const DecodeArgs& a, uint32_t max_frames, hipStream_t st) {
    if (a.rest_only) return hipSuccess;
    const dim3 g = decode_grid<KIND, LAY>(a, max_frames);
    hipError_t e = launch_bucket<KIND, LAY, 8, false>(a, g, st);
    if (e == hipSuccess && bucket_launched(a, 4, false)) e = launch_bucket<KIND, LAY, 4, false>(a, g, st);
    if (e == hipSuccess && bucket_launched(a, 12, false)) e = launch_bucket<KIND, LAY, 12, false>(a, g, st);
    if (e == hipSuccess && bucket_launched(a, 16, false)) e = launch_bucket<KIND, LAY, 16, false>(a, g, st);
    if (e == hipSuccess && bucket_launched(a, 32, false)) e = launch_bucket<KIND, LAY, 32, false>(a, g, st);
    return e != hipSuccess ? e : hipGetLastError();
}

// Waves with CONSTANT / VERBATIM lanes (bucket 8 or 32 + MIX_BIT), after the pure kernels.
// With rest_only: just the `rest` launch of the most general kernel (order 32, constant /
// verbatim lanes) on a small grid, for the groups of buckets without a launch of their own.
template <int KIND, int LAY>
hipError_t launch_decode_mix(const DecodeArgs& a, uint32_t max_frames, hipStream_t st) {
    const dim3 g = decode_grid<KIND, LAY>(a, max_frames);
    if (a.rest_only) {
        DecodeArgs r = a;
        r.rest = 1;
        const dim3 gr(g.x < SPARSE_DECODE_BLOCKS ? g.x : SPARSE_DECODE_BLOCKS);
        const hipError_t e = launch_bucket<KIND, LAY, 32, true>(r, gr, st);
        return e != hipSuccess ? e : hipGetLastError();
    }
    hipError_t e = hipSuccess;
    if (bucket_launched(a, 8, true)) e = launch_bucket<KIND, LAY, 8, true>(a, g, st);
    if (e == hipSuccess && bucket_launched(a, 32, true)) e = launch_bucket<KIND, LAY, 32, true>(a, g, st);
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace zflac
