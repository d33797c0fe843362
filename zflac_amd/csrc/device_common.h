// device_common.h -- device helpers shared by the scan and decode translation units: the
// frame-header parser of frame_header.h bound to device memory and small utils.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <utility>

#include "common.h"
#include "frame_header.h"

namespace zflac {

// ----------------------------------------------------------------------------------
// small helpers
// ----------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// Word 3 of a raw (stride 0) buffer resource on gfx9-family targets: 32-bit data format.
constexpr int BUFFER_RSRC_WORD3 = 0x00020000;

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

static __constant__ Crc8Table CRC8 = make_crc8_table();

__device__ __forceinline__ FrameHdr parse_frame_header(const uint8_t* p, uint64_t avail, uint32_t si_rate) {
    return parse_frame_header_t<1>([p](uint32_t i) -> uint32_t { return p[i]; }, avail, si_rate, CRC8.t);
}
__device__ __forceinline__ FrameHdr parse_frame_fields(const uint8_t* p, uint64_t avail, uint32_t si_rate) {
    return parse_frame_header_t<0>([p](uint32_t i) -> uint32_t { return p[i]; }, avail, si_rate, nullptr);
}

// (the sync-code masks ff_mask, sync_mask, sync_any and the candidate filter candidate_ok:
// frame_header.h, plain C++, so a host probe runs the text the kernels compile)

}  // namespace zflac
