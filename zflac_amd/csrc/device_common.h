// device_common.h -- device helpers shared by the scan and decode translation units: the
// frame-header parser of frame_header.h bound to device memory, the candidate filter and
// small utils.
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

static __constant__ Crc8Table CRC8 = make_crc8_table();

__device__ __forceinline__ FrameHdr parse_frame_header(const uint8_t* p, uint64_t avail, uint32_t si_rate) {
    return parse_frame_header_t<1>([p](uint32_t i) -> uint32_t { return p[i]; }, avail, si_rate, CRC8.t);
}
__device__ __forceinline__ FrameHdr parse_frame_fields(const uint8_t* p, uint64_t avail, uint32_t si_rate) {
    return parse_frame_header_t<0>([p](uint32_t i) -> uint32_t { return p[i]; }, avail, si_rate, nullptr);
}

// Filter for sync candidates: a well-formed header consistent with the stream's first
// frame. Anything it rejects that zflac would still decode breaks the verified chain and
// sends the stream to the sequential planner, so the filter affects speed only.
__device__ __forceinline__ bool candidate_ok(const FrameHdr& h, const StreamDesc& S) {
    return h.err == 0 && !h.crc_eof && h.crc_ok && h.zero_bit == 0 && h.byte1 == S.byte1 &&
           channels_count(h.chan_code) == S.nch && h.dcode == S.dcode && h.rate == S.rate_hz;
}

}  // namespace zflac
