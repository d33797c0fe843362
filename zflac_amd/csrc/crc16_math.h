// crc16_math.h -- the arithmetic of FLAC's frame CRC-16 as plain C++20: no HIP header, so the
// kernel (crc16.hip) and a host-only probe (tests/c/crc16_probe.cpp) compile the same text.
//
// CRC-16 of FLAC frames: x^16 + x^15 + x^2 + 1, MSB first, init 0 (RFC 9639 9.1.8). With init 0
// the CRC is linear: CRC(A || B) = CRC(A) * x^(8|B|) mod P xor CRC(B). k_crc16 leans on that:
// each lane hashes a piece with the slice-by-4 tables, multiplies its remainder by
// x^(8 * bytes after the piece) out of the table of squares, and the wave xor-reduces.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZFLAC_CRC16_HD __host__ __device__
#else
#define ZFLAC_CRC16_HD
#endif

namespace zflac {

constexpr uint32_t CRC16_P = 0x18005;  // x^16 + x^15 + x^2 + 1

struct Crc16Tabs {
    uint16_t t[4][256];  // t[k][v] = v(x) * x^(8k + 16) mod P
};
constexpr Crc16Tabs make_crc16_tabs() {
    Crc16Tabs r{};
    for (uint32_t v = 0; v < 256; v++) {
        uint32_t c = v << 8;
        for (int i = 0; i < 8; i++) c = (c & 0x8000) ? ((c << 1) ^ CRC16_P) : (c << 1);
        r.t[0][v] = (uint16_t)c;
    }
    for (int k = 1; k < 4; k++)
        for (uint32_t v = 0; v < 256; v++) {
            const uint32_t c = r.t[k - 1][v];  // one more zero byte
            r.t[k][v] = (uint16_t)(r.t[0][c >> 8] ^ ((c << 8) & 0xFFFF));
        }
    return r;
}

// a(x) * b(x) mod P for 16-bit remainders (Horner over b's bits, most significant first)
ZFLAC_CRC16_HD constexpr uint32_t crc16_mulmod(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r <<= 1;
        if (r & 0x10000) r ^= CRC16_P;
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}

struct Crc16Pow {
    uint16_t p[40];  // p[k] = x^(8 * 2^k) mod P
};
constexpr Crc16Pow make_crc16_pow() {
    Crc16Pow r{};
    r.p[0] = 0x100;  // x^8
    for (int k = 1; k < 40; k++) r.p[k] = (uint16_t)crc16_mulmod(r.p[k - 1], r.p[k - 1]);
    return r;
}

// ---- compile-time checks: the three identities k_crc16 is built on, each against the bitwise
// CRC (one message bit at a time), which shares nothing with the tables but the polynomial
constexpr uint32_t crc16_bitwise(uint32_t crc, uint32_t byte) {
    crc ^= byte << 8;
    for (int i = 0; i < 8; i++) crc = (crc & 0x8000) ? ((crc << 1) ^ CRC16_P) & 0xFFFFu : (crc << 1) & 0xFFFFu;
    return crc;
}
// one slice-by-4 step as k_crc16 does it: four message bytes b0..b3 in memory order
constexpr uint32_t crc16_slice4(const Crc16Tabs& t, uint32_t crc, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
    return (uint32_t)(t.t[3][(crc >> 8) ^ b0] ^ t.t[2][(crc & 255u) ^ b1] ^ t.t[1][b2] ^ t.t[0][b3]);
}
// crc * x^(8 * rem) mod P by the table of squares, as k_crc16's shift loop does it
constexpr uint32_t crc16_shift(const Crc16Pow& p, uint32_t crc, uint64_t rem) {
    for (int k = 0; rem && k < 40; k++, rem >>= 1)
        if (rem & 1) crc = crc16_mulmod(crc, p.p[k]);
    return crc;
}

constexpr bool crc16_slice4_matches_bitwise() {
    const Crc16Tabs t = make_crc16_tabs();
    uint32_t a = 0, b = 0, x = 12345;  // 4-byte steps against bit steps over a pseudo-random message
    for (int k = 0; k < 300; k++) {
        uint32_t by[4] = {};
        for (int j = 0; j < 4; j++) {
            x = x * 1103515245u + 12345u;
            by[j] = (x >> 16) & 0xFFu;
            a = crc16_bitwise(a, by[j]);
        }
        b = crc16_slice4(t, b, by[0], by[1], by[2], by[3]);
        if (a != b) return false;
    }
    return true;
}
static_assert(crc16_slice4_matches_bitwise(), "slice-by-4 CRC-16 = bitwise CRC-16");

constexpr bool crc16_pow_matches_byte_shifts() {
    const Crc16Pow p = make_crc16_pow();
    uint32_t r = 1;  // x^0; one zero byte more per step: r * x^8 mod P
    uint32_t n = 0;
    for (int k = 0; k <= 10; k++) {  // 2^10 single-byte shifts: cheap in a constant expression
        for (; n < (1u << k); n++) r = crc16_mulmod(r, 0x100);
        if (p.p[k] != r) return false;
    }
    // the single-byte shift itself against the bitwise CRC: CRC(v || 00) = CRC(v) * x^8
    for (uint32_t v = 0; v < 256; v++)
        if (crc16_mulmod(crc16_bitwise(0, v), 0x100) != crc16_bitwise(crc16_bitwise(0, v), 0)) return false;
    return true;
}
static_assert(crc16_pow_matches_byte_shifts(), "p[k] = x^(8 * 2^k) mod P, k = 0..10");

constexpr bool crc16_split_matches_whole() {
    const Crc16Pow p = make_crc16_pow();
    uint8_t msg[160] = {};
    uint32_t x = 2463534242u;
    for (int i = 0; i < 160; i++) {
        x = x * 1103515245u + 12345u;
        msg[i] = (uint8_t)(x >> 16);
    }
    uint32_t whole = 0;
    for (int i = 0; i < 160; i++) whole = crc16_bitwise(whole, msg[i]);
    for (int cut = 0; cut <= 160; cut += (cut < 8 || cut >= 152) ? 1 : 13) {  // empty pieces included
        uint32_t a = 0, b = 0;
        for (int i = 0; i < cut; i++) a = crc16_bitwise(a, msg[i]);
        for (int i = cut; i < 160; i++) b = crc16_bitwise(b, msg[i]);
        if ((crc16_shift(p, a, (uint64_t)(160 - cut)) ^ b) != whole) return false;
    }
    return true;
}
static_assert(crc16_split_matches_whole(), "CRC(A || B) = CRC(A) * x^(8|B|) xor CRC(B)");

}  // namespace zflac
