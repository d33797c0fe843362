// decode/pcm_stage.h -- the PCM output stage: pending packed stores, packed i16 helpers, stereo
// decorrelation, the staged write-back of the 16-bit kernels, and the chunk-start top-up.
#pragma once
#include "lane_reader.h"
#include "row_mask.h"

namespace zflac {

// ----------------------------------------------------------------------------------
// Output
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
    uint32_t rw[3];  // the resource write-back: the buffer's address (low, high) and bytes, wave-uniform
                     // but held in VGPRs on purpose (see store_rsrc)
    uint32_t gq[4];  // quad index (from `out`) of this lane's piece of row t at sample 0 (the resource
                     // form: its byte offset)
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
    // WB_RSRC_MAX = 2^31 bytes). gq[t] is then the byte offset of the lane's piece at sample 0
    // (< 2^31, fixed for the subframe) and goes in as the store's vector offset unchanged; the
    // chunk's own offset is wave-uniform, at most 4 * 65535 bytes, and is the store's scalar
    // offset: their sum stays below 2^32. A lane whose frame is masked takes the offset 2^31
    // instead, which lies past the resource with or without the scalar offset: the buffer unit
    // drops its store, no dummy line is written. The choice is one v_cndmask per row on the row's
    // lane mask (row_lane_mask: scalar instructions on the wave-uniform frame mask), and nothing
    // else per lane is left in the chunk.
    // (The four stores stay unconditional, in straight-line code. Stored under their lane masks
    // in branches of their own (s_and_saveexec, s_cbranch_execz) they saved the four v_cndmask,
    // but the top-up's waits for its staged loads can then no longer count on the stores as
    // younger operations: vmcnt(7..4) became vmcnt(3..0), every chunk start waited for its own
    // write-back to finish, and k_decode ran 4 % longer with 4 % fewer vector instructions.)
    // The resource's four words are made here, at every write-back, from three v_readfirstlane of
    // rw[] and a constant: held in SGPRs across the chunk they were spilled to VGPR lanes, and each
    // of the four stores read them back and wrote them out again (8 v_readlane / v_writelane per
    // store). The empty asm makes rw[] a new value at every write-back, so the reads stay here.
    // `sbase`: `base` as a value the compiler knows to be wave-uniform (see flush).
    __device__ __forceinline__ void store_rsrc(const uint4 (&v)[4], uint32_t sbase) {
        const uint32_t so = MONO ? sbase * 2u : sbase * 4u;  // bytes per sample: 2 mono, 4 stereo
        asm volatile("" : "+v"(rw[0]), "+v"(rw[1]), "+v"(rw[2]));
        // (each half widened as unsigned: the builtin returns int, and a sign-extended low half
        // would set every high bit of a pointer whose bit 31 is set)
        const uint64_t o = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(rw[1]) << 32) |
                           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(rw[0]);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<void*>(o), (short)0, (int)__builtin_amdgcn_readfirstlane(rw[2]), BUFFER_RSRC_WORD3);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t off = __builtin_amdgcn_inverse_ballot_w64(row_lane_mask<MONO>(mask, t)) ? gq[t] : 0x80000000u;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v[t]), rs, (int)off, (int)so, 0);
        }
    }
    // `sbase`: the staged chunk's first sample again, for the resource form's scalar offset. `base`
    // itself is carried round the chunk loop, whose trip count is per-lane to the compiler, so it
    // counts as divergent and a store with it as scalar offset is wrapped in a waterfall loop.
    template <bool WBR>
    __device__ __forceinline__ void flush(uint4* dummy, uint32_t sbase) {
        uint4 v[4];
        read(v);
        if constexpr (WBR) store_rsrc(v, sbase);
        else store(v, dummy);
    }
};
template <int LAY>
using StageOf = Stage<LAY == LAY_MONO>;

// Per-lane dummy slot (2 quads), spread over 64 wave slots so masked stores of different
// waves do not pile onto the same lines. DUMMY_BYTES on the host side.
__device__ __forceinline__ uint32_t dummy_slot() {
    return 2u * ((threadIdx.x & 63u) + 64u * ((blockIdx.x * DEC_WAVES + (threadIdx.x >> 6)) & 63u));
}

// Chunk-start top-up. Decode: the previous chunk's pending PCM stores first (they then have the
// whole chunk to complete before the next chunk-start wait), then the ring's top-up (its wait for
// the previous top-up's loads, the ring stores, the next loads); loads first and stores after
// measured 20 % slower in k_decode (0.67 vs 0.56 ms on the C5 shard). The walk: the ring alone.
// k_decode's junk slots are the first word slots of the wave's output stage: the flush has
// just read every staged piece into registers (LDS operations of a wave complete in order),
// and the chunk's own pieces are written only after this top-up.
template <int KIND, int LAY, bool WALK, bool WBR>
__device__ __forceinline__ void topup_st(Rdr& rd, Pend& pd, StageOf<LAY>& sg, uint4* dummy, uint32_t sbase) {
    if constexpr (!WALK) {
        if constexpr (staged<KIND, LAY>()) sg.template flush<WBR>(dummy, sbase);
        else pd.flush(pend_two<KIND>());
    }
    rd.template topup<topup_quads<KIND>()>();
}

}  // namespace zflac
