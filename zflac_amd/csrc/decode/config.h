// decode/config.h -- ring, chunk and LDS constants of k_walk / k_decode, the layout, mode and
// decorrelation enums, and small compile-time helpers.
#pragma once
#include "../device_common.h"

#ifndef ZFLAC_RING_Q
#error "include decode.inc: it sets the ring size of the unit"
#endif

namespace zflac {

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
// Samples per chunk: 32, for k_walk and k_decode alike. The ring is topped up
// at chunk starts, right after the wait for everything issued before: the loads staged then
// are stored into the ring now and the next ones issued, so every load has 32 samples or
// more to land. The output stage holds one chunk. (64-sample decode chunks,
// round 5, spilled 126 VGPRs in the order-8 kernel: DESIGN.md section 10.)
constexpr int CHUNK = 32;
// Quads staged per top-up: 4 (16 words = 16 bits/sample) for 8- and 16-bit containers, 6
// for 32-bit ones. A lane that reads faster than that runs its ring dry and redoes the
// chunk on the generic path, which refills synchronously.
template <int KIND>
__device__ __forceinline__ constexpr int topup_quads() { return KIND == 2 ? 6 : 4; }
// Largest Rice parameter for which the fast chunk decodes two codes per 32-bit window: a
// pair then spills past the window only when its two quotients sum to more than 30 - 2k.
constexpr uint32_t PAIR_KMAX = 9;
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
enum Decor : int { D_MS = 10, D_GEN = 1 };

// Compile-time loop: f(std::integral_constant<int, I>) for I in [0, N).
template <typename F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// 16-bit containers, stereo or mono: PCM goes through the stage
template <int KIND, int LAY>
__host__ __device__ __forceinline__ constexpr bool staged() { return KIND == 1 && LAY != LAY_MULTI; }

template <int KIND>
__device__ __forceinline__ constexpr bool pend_two() { return KIND == 2; }

}  // namespace zflac
