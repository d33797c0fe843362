// decode/row_mask.h -- which lanes of a write-back row store: the stage's frame mask to the lane
// mask of one row. Plain C++ (host and device), so the CPU test of the lane layout
// (tests/c/row_mask_probe.cpp) calls the very function the kernels run.
#pragma once
#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace zflac {

#if defined(__HIP_DEVICE_COMPILE__)
// s_bitreplicate_b64_b32 (no clang builtin of its own): bit i of x to bits 2i and 2i + 1
__device__ uint64_t s_bitreplicate(uint32_t x) __asm("llvm.amdgcn.s.bitreplicate");
#endif

// every bit of x doubled: bit i to bits 2i and 2i + 1. One scalar instruction on the device.
__host__ __device__ constexpr uint64_t double_bits(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (!__builtin_is_constant_evaluated()) return s_bitreplicate(x);
#endif
    uint64_t r = 0;
    for (int i = 0; i < 32; i++) r |= (uint64_t)((x >> i) & 1u) * 3u << (2 * i);
    return r;
}

// Lane mask of write-back row t (0..3) of the output stage (Stage in pcm_stage.h), from the
// frame mask (bit j: frame j's staged chunk goes to memory). A row is 64 lanes of 16 bytes:
// * stereo: frames 8t..8t+7, lane L holds a piece of frame 8t + (L >> 3): 8 lanes per frame;
// * mono: frames 16t..16t+15, lane L a piece of frame 16t + (L >> 2): 4 lanes per frame.
// The row's frame bits, each doubled log2(lanes per frame) times: scalar instructions only when
// `frames` is wave-uniform (s_bfe, then s_bitreplicate three or two times).
template <bool MONO>
__host__ __device__ constexpr uint64_t row_lane_mask(uint64_t frames, int t) {
    constexpr int ROW_FRAMES = MONO ? 16 : 8;
    const uint32_t row = (uint32_t)(frames >> (t * ROW_FRAMES)) & ((1u << ROW_FRAMES) - 1u);
    if constexpr (MONO) return double_bits((uint32_t)double_bits(row));
    else return double_bits((uint32_t)double_bits((uint32_t)double_bits(row)));
}

}  // namespace zflac
