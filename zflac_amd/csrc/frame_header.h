// frame_header.h -- the exact frame-header parser (src/zflac.zig:343-407), its format tables,
// the register CRC-8, the candidate filter and the SWAR sync-code masks of the frame scan. Plain
// C++20 with no HIP header: the kernels include it through device_common.h, the host planner
// (stream_plan.cpp) and the scan probe (tests/c/scan_probe.cpp) directly, so both sides run one text.
#pragma once
#include <cstdint>

#include "common.h"

// (what HIP's __forceinline__ expands to; the kernels' inlining must not depend on the includer)
#define ZFLAC_HDI ZFLAC_HD inline __attribute__((always_inline))
#ifdef __clang__
#define ZFLAC_UNROLL _Pragma("unroll")
#else
#define ZFLAC_UNROLL _Pragma("GCC unroll 8")
#endif

namespace zflac {

ZFLAC_HDI int channels_count(uint32_t code) {  // Channels.count, src/zflac.zig:107-122
    return code <= 7 ? (int)code + 1 : (code <= 10 ? 2 : 0);
}
ZFLAC_HDI uint32_t rate_table(uint32_t code) {  // SampleRate.hz, src/zflac.zig:75-90
    switch (code) {
        case 1: return 88200;
        case 2: return 176400;
        case 3: return 192000;
        case 4: return 8000;
        case 5: return 16000;
        case 6: return 22050;
        case 7: return 24000;
        case 8: return 32000;
        case 9: return 44100;
        case 10: return 48000;
        default: return 96000;
    }
}
ZFLAC_HDI int depth_bits(uint32_t dcode, int si_bps) {  // BitDepth.bps, src/zflac.zig:135-145
    switch (dcode) {
        case 0: return si_bps;
        case 1: return 8;
        case 2: return 12;
        case 4: return 16;
        case 5: return 20;
        case 6: return 24;
        case 7: return 32;
        default: return -1;  // reserved: `unreachable` in zflac
    }
}

struct Crc8Table {
    uint8_t t[256];
};
constexpr Crc8Table make_crc8_table() {  // x^8 + x^2 + x + 1, init 0 (RFC 9639 frame header CRC)
    Crc8Table r{};
    for (int i = 0; i < 256; i++) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; k++) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xFF : (c << 1) & 0xFF;
        r.t[i] = (uint8_t)c;
    }
    return r;
}

// a (a polynomial of degree < 32 over GF(2)) mod x^8 + x^2 + x + 1. With x^8 = x^2 + x + 1,
// a = t x^8 + l reduces to t (x^2 + x + 1) + l: one fold lowers the degree by 6, four take
// 31 down to 7. Register-only: a table lookup is an LDS round trip per byte, and the bytes of
// a header are a dependent chain.
constexpr uint32_t crc8_reduce(uint32_t a) {
    for (int i = 0; i < 4; i++) {
        const uint32_t t = a >> 8;
        a = (t ^ (t << 1) ^ (t << 2)) ^ (a & 0xFFu);
    }
    return a;
}
// CRC-8 (init 0, MSB first) after three more bytes b0 b1 b2 (w = b0 << 16 | b1 << 8 | b2):
// the message (b0 ^ crc) x^16 + b1 x^8 + b2, times x^8, mod the polynomial
constexpr uint32_t crc8_3(uint32_t crc, uint32_t w) { return crc8_reduce((w ^ (crc << 16)) << 8); }
constexpr uint32_t crc8_1(uint32_t crc, uint32_t b) { return crc8_reduce((crc ^ b) << 8); }
constexpr bool crc8_fold_matches_table() {
    const Crc8Table t = make_crc8_table();
    for (uint32_t i = 0; i < 256; i++)
        if (crc8_1(0, i) != t.t[i]) return false;
    uint32_t a = 0, b = 0, x = 12345;  // 3-byte steps against byte steps over a pseudo-random message
    for (int k = 0; k < 300; k++) {
        uint32_t w = 0;
        for (int j = 0; j < 3; j++) {
            x = x * 1103515245u + 12345u;
            const uint32_t by = (x >> 16) & 0xFFu;
            a = t.t[a ^ by];
            w = (w << 8) | by;
        }
        b = crc8_3(b, w);
        if (a != b) return false;
    }
    return true;
}
static_assert(crc8_fold_matches_table(), "register CRC-8 = table CRC-8");

// Does a header of n bytes (6..16, its CRC-8 byte last) carry the right CRC-8? h0..h3 hold
// header bytes 0..15 in memory order (byte 0 in the low bits of h0), whatever follows the
// header in the bytes from n on. With init 0 and no final xor, the CRC-8 of a message followed
// by its own CRC-8 is 0, and zero bytes after that leave it 0 (x is invertible modulo the
// polynomial), while a wrong CRC-8 leaves a nonzero remainder that zeros never clear. So the
// bytes from n on are zeroed and the 16 go through 3-byte steps at constant byte positions (two,
// then one more per three bytes the header reaches), where a loop over the header's own length
// picks every byte with a computed index and ends with one or two single-byte steps (k_hop).
constexpr uint32_t crc8_keep_bytes(uint32_t be_word, int bytes) {  // the first `bytes` (<= 0: none, >= 4: all)
    const int s = bytes < 0 ? 0 : (bytes > 4 ? 32 : 8 * bytes);
    return be_word & (uint32_t)(0xFFFFFFFF00000000ull >> s);
}
constexpr bool crc8_header_ok(uint32_t h0, uint32_t h1, uint32_t h2, uint32_t h3, uint32_t n) {
    const uint32_t w0 = __builtin_bswap32(h0);  // n >= 6: whole
    const uint32_t w1 = crc8_keep_bytes(__builtin_bswap32(h1), (int)n - 4);
    // (crc8_3 shifts its 24-bit group up by 8: whatever a group carries above bit 23 falls out)
    uint32_t crc = crc8_3(0, w0 >> 8);
    crc = crc8_3(crc, (w0 << 16) | (w1 >> 16));
    // the groups from byte 6 on only where the header reaches them (all zero otherwise): most
    // headers are 6 or 7 bytes long
    if (n > 6) {
        const uint32_t w2 = crc8_keep_bytes(__builtin_bswap32(h2), (int)n - 8);
        crc = crc8_3(crc, (w1 << 8) | (w2 >> 24));
        if (n > 9) {
            const uint32_t w3 = crc8_keep_bytes(__builtin_bswap32(h3), (int)n - 12);
            crc = crc8_3(crc, w2);
            if (n > 12) crc = crc8_1(crc8_3(crc, w3 >> 8), w3 & 0xFFu);
        }
    }
    return crc == 0;
}
constexpr bool crc8_header_ok_matches_table() {
    const Crc8Table t = make_crc8_table();
    uint32_t x = 2463534242u;
    for (int k = 0; k < 64; k++) {
        for (uint32_t n = 6; n <= 16; n++) {
            uint8_t b[16] = {};
            for (int i = 0; i < 16; i++) {
                x = x * 1103515245u + 12345u;
                b[i] = (uint8_t)(x >> 16);
            }
            uint32_t crc = 0;
            for (uint32_t i = 0; i + 1 < n; i++) crc = t.t[crc ^ b[i]];
            for (int bad = 0; bad < 2; bad++) {  // the right CRC-8 byte, then a wrong one
                b[n - 1] = (uint8_t)(crc ^ (bad ? 1u + (x >> 24) % 255u : 0u));
                uint32_t h[4] = {};
                for (int i = 0; i < 16; i++) h[i / 4] |= (uint32_t)b[i] << (8 * (i % 4));
                if (crc8_header_ok(h[0], h[1], h[2], h[3], n) != (bad == 0)) return false;
            }
        }
    }
    return true;
}
static_assert(crc8_header_ok_matches_table(), "fixed-length header CRC-8 = table CRC-8, lengths 6..16");

// ----------------------------------------------------------------------------------
// Frame header, exact zflac semantics (src/zflac.zig:343-375, 203-214, 407).
// `err` holds errors raised before the first-frame / consistency checks; a missing
// CRC-8 byte is reported separately because zflac reads it after those checks.
// ----------------------------------------------------------------------------------
struct FrameHdr {
    uint32_t bs, rate, hdr_len;  // hdr_len: header bytes, CRC-8 included (when err == 0)
    uint32_t chan_code, dcode, byte1, zero_bit, bs_code;
    int err;
    bool crc_eof;
    bool crc_ok;
};

// `at(i)` returns header byte i (global memory, an LDS copy, registers or host memory). CRC:
// 0 skips the CRC-8 (the decode kernels and the host planner only need the fields), 1 looks
// it up in `crc_tab` (global memory, or an LDS copy), 2 computes it in registers (k_scan).
template <int CRC, typename At>
ZFLAC_HDI FrameHdr parse_frame_header_t(At&& at, uint64_t avail, uint32_t si_rate, const uint8_t* crc_tab) {
    FrameHdr h;
    h.bs = h.rate = h.hdr_len = 0;
    h.chan_code = h.dcode = h.byte1 = h.zero_bit = h.bs_code = 0;
    h.err = 0;
    h.crc_eof = false;
    h.crc_ok = false;
    if (avail < 4) { h.err = E_END_OF_STREAM; return h; }
    const uint32_t b0 = at(0), b1 = at(1), b2 = at(2), b3 = at(3);
    h.byte1 = b1;
    h.chan_code = b3 >> 4;
    h.dcode = (b3 >> 1) & 7;
    h.zero_bit = b3 & 1;
    h.bs_code = b2 >> 4;
    if (((b0 << 7) | (b1 >> 1)) != 0x7FFC) { h.err = E_INVALID_FRAME_HEADER; return h; }  // :351-352
    uint32_t idx = 4;
    // read_coded_number (:203-214)
    if (avail <= idx) { h.err = E_END_OF_STREAM; return h; }
    const uint32_t first = at(idx++);
#ifdef __HIP_DEVICE_COMPILE__
    const uint32_t ones = __clz((~first & 0xFFu) << 24) > 8 ? 8 : __clz((~first & 0xFFu) << 24);
#else
    uint32_t ones = 0;
    while (ones < 8 && (first & (0x80u >> ones))) ones++;
#endif
    if (first == 0xFF || ones == 1) { h.err = E_INVALID_CODED_NUMBER; return h; }
    if (ones >= 2) {
        if (avail < (uint64_t)idx + (ones - 1)) { h.err = E_END_OF_STREAM; return h; }
        idx += ones - 1;
    }
    // block size (:356-365)
    const uint32_t bc = b2 >> 4;
    if (bc == 0) { h.err = E_INVALID_FRAME_HEADER; return h; }
    if (bc == 6) {
        if (avail <= idx) { h.err = E_END_OF_STREAM; return h; }
        h.bs = (uint32_t)at(idx++) + 1;
    } else if (bc == 7) {
        if (avail < (uint64_t)idx + 2) { h.err = E_END_OF_STREAM; return h; }
        const uint32_t v = ((uint32_t)at(idx) << 8) | at(idx + 1);
        idx += 2;
        if (v == 0xFFFF) { h.err = E_INVALID_FRAME_HEADER; return h; }
        h.bs = v + 1;
    } else if (bc == 1) {
        h.bs = 192;
    } else if (bc <= 5) {
        h.bs = 144u << bc;
    } else {
        h.bs = 1u << bc;
    }
    // sample rate (:367-374); uncommon 8-bit rate is taken in Hz as zflac does (:369)
    const uint32_t rc = b2 & 15;
    if (rc == 0) {
        h.rate = si_rate;
    } else if (rc == 12) {
        if (avail <= idx) { h.err = E_END_OF_STREAM; return h; }
        h.rate = at(idx++);
    } else if (rc == 13 || rc == 14) {
        if (avail < (uint64_t)idx + 2) { h.err = E_END_OF_STREAM; return h; }
        h.rate = ((uint32_t)at(idx) << 8) | at(idx + 1);
        if (rc == 14) h.rate *= 10;
        idx += 2;
    } else if (rc == 15) {
        h.err = E_INVALID_FRAME_HEADER;
        return h;
    } else {
        h.rate = rate_table(rc);
    }
    // CRC-8 byte (:407): read, never checked by zflac; checked here only to filter
    // sync candidates.
    h.hdr_len = idx + 1;
    if (avail <= idx) {
        h.crc_eof = true;
        return h;
    }
    if constexpr (CRC == 1) {
        uint32_t crc = 0;
        for (uint32_t i = 0; i < idx; i++) crc = crc_tab[crc ^ at(i)];
        h.crc_ok = crc == at(idx);
    } else if constexpr (CRC == 2) {
        uint32_t crc = 0, i = 0;  // idx <= 15: up to five 3-byte steps, then up to two bytes
        ZFLAC_UNROLL
        for (int g = 0; g < 5; g++) {
            if (i + 3 <= idx) {
                crc = crc8_3(crc, (at(i) << 16) | (at(i + 1) << 8) | at(i + 2));
                i += 3;
            }
        }
        ZFLAC_UNROLL
        for (int g = 0; g < 2; g++) {
            if (i < idx) {
                crc = crc8_1(crc, at(i));
                i++;
            }
        }
        h.crc_ok = crc == at(idx);
    }
    return h;
}

// Filter for sync candidates: a well-formed header consistent with the stream's first
// frame. Anything it rejects that zflac would still decode breaks the verified chain and
// sends the stream to the sequential planner, so the filter affects speed only.
ZFLAC_HDI bool candidate_ok(const FrameHdr& h, const StreamDesc& S) {
    return h.err == 0 && !h.crc_eof && h.crc_ok && h.zero_bit == 0 && h.byte1 == S.byte1 &&
           channels_count(h.chan_code) == S.nch && h.dcode == S.dcode && h.rate == S.rate_hz;
}

// ----------------------------------------------------------------------------------
// frame sync codes in registers (k_scan, k_hop; on the host: tests/c/scan_probe.cpp)
// ----------------------------------------------------------------------------------
ZFLAC_HD inline uint32_t ff_mask(uint32_t d) { return ((d & 0x7F7F7F7Fu) + 0x01010101u) & d & 0x80808080u; }

// Byte i = the byte after byte i of d (byte 0 of dn for i = 3): v_alignbyte on the device.
ZFLAC_HDI uint32_t bytes_after(uint32_t d, uint32_t dn) {
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_alignbyte(dn, d, 1);
#else
    return (d >> 8) | (dn << 24);
#endif
}

// Bit 7 of byte i set where byte i of d is 0xFF and the byte after it (byte i + 1, or the
// first byte of dn for i = 3) is 0xF8 or 0xF9: a frame sync code (src/zflac.zig:351-352).
// Exact per byte (no borrow between bytes).
ZFLAC_HDI uint32_t sync_mask(uint32_t d, uint32_t dn) {
    const uint32_t nxt = bytes_after(d, dn);
    const uint32_t y = (nxt & 0xFEFEFEFEu) ^ 0xF8F8F8F8u;  // zero bytes: next is 0xF8 / 0xF9
    const uint32_t zero = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
    return ff_mask(d) & zero;
}

// Nonzero iff some byte i of d is 0xFF and the byte after it 0xF8 / 0xF9: the same test as
// sync_mask, as an existence test only. Byte i of t is zero exactly at a sync code, and
// (t - 0x01..01) & ~t & 0x80..80 is nonzero iff t has a zero byte (the borrows can mark a
// byte above a zero one, never create a mark without one). ~5 VALU per dword against
// sync_mask's ~10: k_scan runs it on every window and the exact masks only where it fires
// (a sync code, or a 0xFF 0xF8|F9 pair in the coded bits: ~1 in 7 wave-windows of 1 KiB).
ZFLAC_HDI uint32_t sync_any(uint32_t d, uint32_t dn) {
    const uint32_t nxt = bytes_after(d, dn);
    const uint32_t t = ~d | ((nxt & 0xFEFEFEFEu) ^ 0xF8F8F8F8u);
    return (t - 0x01010101u) & ~t & 0x80808080u;
}

// The value of the header's coded number (read_coded_number, src/zflac.zig:203-214; header
// byte 4 onwards), which parse_frame_header_t only skips: the frame number of a fixed-blocking
// stream, the first sample's number of a variable-blocking one. False where zflac's reader
// fails (InvalidCodedNumber, or fewer than `avail` bytes). `at` as for parse_frame_header_t.
template <typename At>
ZFLAC_HDI bool coded_number_value(At&& at, uint64_t avail, uint64_t& value) {
    value = 0;
    if (avail <= 4) return false;
    const uint32_t first = at(4);
    uint32_t ones = 0;
    ZFLAC_UNROLL
    for (int k = 0; k < 8; k++)
        if (ones == (uint32_t)k && (first & (0x80u >> k))) ones++;
    if (first == 0xFF || ones == 1) return false;
    if (ones == 0) {
        value = first;
        return true;
    }
    if (avail < (uint64_t)4 + ones) return false;
    uint64_t v = first & (0x7Fu >> ones);
    ZFLAC_UNROLL
    for (uint32_t k = 1; k < 7; k++)
        if (k < ones) v = (v << 6) | (at(4 + k) & 0x3Fu);
    value = v;
    return true;
}

}  // namespace zflac
