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

// ----------------------------------------------------------------------------------
// frame sync codes in registers (k_scan, k_hop)
// ----------------------------------------------------------------------------------
__device__ inline uint32_t ff_mask(uint32_t d) { return ((d & 0x7F7F7F7Fu) + 0x01010101u) & d & 0x80808080u; }

// Bit 7 of byte i set where byte i of d is 0xFF and the byte after it (byte i + 1, or the
// first byte of dn for i = 3) is 0xF8 or 0xF9: a frame sync code (src/zflac.zig:351-352).
// Exact per byte (no borrow between bytes).
__device__ __forceinline__ uint32_t sync_mask(uint32_t d, uint32_t dn) {
    const uint32_t nxt = __builtin_amdgcn_alignbyte(dn, d, 1);  // byte i = the byte after byte i of d
    const uint32_t y = (nxt & 0xFEFEFEFEu) ^ 0xF8F8F8F8u;        // zero bytes: next is 0xF8 / 0xF9
    const uint32_t zero = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
    return ff_mask(d) & zero;
}

// Nonzero iff some byte i of d is 0xFF and the byte after it 0xF8 / 0xF9: the same test as
// sync_mask, as an existence test only. Byte i of t is zero exactly at a sync code, and
// (t - 0x01..01) & ~t & 0x80..80 is nonzero iff t has a zero byte (the borrows can mark a
// byte above a zero one, never create a mark without one). ~5 VALU per dword against
// sync_mask's ~10: k_scan runs it on every window and the exact masks only where it fires
// (a sync code, or a 0xFF 0xF8|F9 pair in the coded bits: ~1 in 7 wave-windows of 1 KiB).
__device__ __forceinline__ uint32_t sync_any(uint32_t d, uint32_t dn) {
    const uint32_t nxt = __builtin_amdgcn_alignbyte(dn, d, 1);
    const uint32_t t = ~d | ((nxt & 0xFEFEFEFEu) ^ 0xF8F8F8F8u);
    return (t - 0x01010101u) & ~t & 0x80808080u;
}

// Filter for sync candidates: a well-formed header consistent with the stream's first
// frame. Anything it rejects that zflac would still decode breaks the verified chain and
// sends the stream to the sequential planner, so the filter affects speed only.
__device__ __forceinline__ bool candidate_ok(const FrameHdr& h, const StreamDesc& S) {
    return h.err == 0 && !h.crc_eof && h.crc_ok && h.zero_bit == 0 && h.byte1 == S.byte1 &&
           channels_count(h.chan_code) == S.nch && h.dcode == S.dcode && h.rate == S.rate_hz;
}

}  // namespace zflac
