// scan_probe.cpp -- test shim (tests/test_scan_edges.py): the frame scan's integer logic on the
// host. Built with plain g++ against zflac_amd/csrc/frame_header.h and common.h alone: the sync-code
// masks, the header parser with its register CRC-8 and the candidate filter are the text k_scan,
// k_compact and k_hop compile. As a shared library for the tests; with -DSCAN_PROBE_MAIN a program
// of its own (also built with -fsanitize=address,undefined) that walks the streams named on its
// command line and prints one line per stream.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "common.h"
#include "frame_header.h"

namespace {

using namespace zflac;

constexpr Crc8Table CRC8 = make_crc8_table();
constexpr uint8_t FILL[6] = {0x00, 0x01, 0x7F, 0x80, 0xF8, 0xFF};

uint32_t mask_by_bytes(uint32_t d, uint32_t dn) {
    uint32_t out = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t by = (d >> (8 * i)) & 0xFFu;
        const uint32_t nx = i < 3 ? (d >> (8 * (i + 1))) & 0xFFu : dn & 0xFFu;
        out |= (uint32_t)((by == 0xFFu) & ((nx & 0xFEu) == 0xF8u)) << (8 * i + 7);  // (no branch: the loop vectorises)
    }
    return out;
}

// Fillings [f0, f1) of the six bytes around the pair (base 6 digits of f), every pair of bytes at
// every position: the number of (d, dn) at which a mask is wrong.
uint64_t masks_range(uint32_t f0, uint32_t f1) {
    uint64_t bad = 0;
    for (uint32_t f = f0; f < f1; f++) {
        for (int pos = 0; pos < 4; pos++) {
            uint64_t base = 0;
            uint32_t digits = f;
            for (int slot = 0; slot < 8; slot++) {
                if (slot == pos || slot == pos + 1) continue;
                base |= (uint64_t)FILL[digits % 6] << (8 * slot);
                digits /= 6;
            }
            for (uint32_t x = 0; x < 256; x++) {
                const uint64_t bx = base | (uint64_t)x << (8 * pos);
                uint32_t wrong = 0;
                for (uint32_t y = 0; y < 256; y++) {
                    const uint64_t v = bx | (uint64_t)y << (8 * (pos + 1));
                    const uint32_t d = (uint32_t)v, dn = (uint32_t)(v >> 32);
                    const uint32_t want = mask_by_bytes(d, dn), got = sync_mask(d, dn);
                    wrong += (got != want) | ((sync_any(d, dn) != 0) != (want != 0));
                }
                bad += wrong;
            }
        }
    }
    return bad;
}

uint64_t ff_mask_wrong() {  // ff_mask alone: every byte value in every position among every filling
    uint64_t bad = 0;
    for (uint32_t f = 0; f < 216; f++)
        for (int pos = 0; pos < 4; pos++)
            for (uint32_t x = 0; x < 256; x++) {
                uint32_t d = 0, digits = f;
                for (int slot = 0; slot < 4; slot++) {
                    if (slot == pos) continue;
                    d |= (uint32_t)FILL[digits % 6] << (8 * slot);
                    digits /= 6;
                }
                d |= x << (8 * pos);
                uint32_t want = 0;
                for (int i = 0; i < 4; i++)
                    if (((d >> (8 * i)) & 0xFFu) == 0xFFu) want |= 0x80u << (8 * i);
                bad += ff_mask(d) != want;
            }
    return bad;
}

struct Found {
    std::vector<uint64_t> pos;
    std::vector<uint32_t> bs, hdr_len;
};

// CRC form 2 (k_scan's): sync codes from sync_mask over 16-byte windows of the stream's grid, the
// header read out of four little-endian words. CRC form 1 (k_compact's rescan): a byte loop and the
// table. Bytes past the stream's end read as zero in both (the parser asks for none of them).
Found walk(const uint8_t* data, uint64_t len, uint64_t frames_begin, const StreamDesc& S, int form) {
    Found out;
    auto byte = [&](uint64_t i) -> uint32_t { return i < len ? data[i] : 0u; };
    auto word = [&](uint64_t i) -> uint32_t { return byte(i) | byte(i + 1) << 8 | byte(i + 2) << 16 | byte(i + 3) << 24; };
    auto take = [&](uint64_t p) {
        FrameHdr h;
        if (form == 2) {
            const uint32_t w[4] = {word(p), word(p + 4), word(p + 8), word(p + 12)};
            h = parse_frame_header_t<2>([&w](uint32_t i) -> uint32_t { return (w[(i >> 2) & 3u] >> (8 * (i & 3u))) & 0xFFu; },
                                        len - p, S.si_rate, nullptr);
        } else {
            h = parse_frame_header_t<1>([&](uint32_t i) -> uint32_t { return byte(p + i); }, len - p, S.si_rate, CRC8.t);
        }
        if (!candidate_ok(h, S)) return;
        out.pos.push_back(p);
        out.bs.push_back(h.bs);
        out.hdr_len.push_back(h.hdr_len);
    };
    if (form == 2) {
        for (uint64_t ws = frames_begin & ~(uint64_t)15; ws < len; ws += 16)
            for (int k = 0; k < 4; k++) {
                const uint32_t m = sync_mask(word(ws + 4 * k), word(ws + 4 * k + 4));
                for (int i = 0; i < 4; i++) {
                    const uint64_t p = ws + 4 * k + i;
                    if ((m >> (8 * i + 7) & 1u) && p >= frames_begin && p + 1 < len) take(p);
                }
            }
    } else {
        for (uint64_t p = frames_begin; p + 1 < len; p++)
            if (data[p] == 0xFF && (data[p + 1] & 0xFE) == 0xF8) take(p);
    }
    return out;
}

}  // namespace

extern "C" {

void scan_probe_constants(uint64_t* out) {
    out[0] = CHUNK_BYTES;
    out[1] = SCAN_THREADS;
    out[2] = SCAN_BYTES_PER_THREAD;
    out[3] = CHUNK_CAP;
}

// The number of (d, dn) at which ff_mask, sync_mask or sync_any is wrong, over every pair of bytes
// at each of the four positions of d among the first `fillings` (of 6^6) fillings of the six other
// bytes, on `threads` threads.
uint64_t scan_probe_masks(uint32_t fillings, uint32_t threads) {
    if (threads < 1) threads = 1;
    std::vector<uint64_t> bad(threads, 0);
    std::vector<std::thread> ts;
    for (uint32_t t = 0; t < threads; t++)
        ts.emplace_back([&, t] {
            bad[t] = masks_range((uint32_t)((uint64_t)fillings * t / threads), (uint32_t)((uint64_t)fillings * (t + 1) / threads));
        });
    uint64_t total = ff_mask_wrong();
    for (auto& t : ts) t.join();
    for (uint64_t b : bad) total += b;
    return total;
}

// Candidates from frames_begin on, in order: returns their count (the first `cap` are stored).
uint64_t scan_probe_candidates(const uint8_t* data, uint64_t len, uint64_t frames_begin, uint32_t byte1, uint32_t nch,
                               uint32_t dcode, uint32_t rate_hz, uint32_t si_rate, int form, uint64_t* pos, uint32_t* bs,
                               uint32_t* hdr_len, uint64_t cap) {
    StreamDesc S;
    std::memset(&S, 0, sizeof(S));
    S.in_begin = frames_begin;
    S.in_end = len;
    S.byte1 = (uint8_t)byte1;
    S.nch = (uint8_t)nch;
    S.dcode = (uint8_t)dcode;
    S.rate_hz = rate_hz;
    S.si_rate = si_rate;
    const Found f = walk(data, len, frames_begin, S, form);
    for (uint64_t i = 0; i < f.pos.size() && i < cap; i++) {
        pos[i] = f.pos[i];
        bs[i] = f.bs[i];
        hdr_len[i] = f.hdr_len[i];
    }
    return f.pos.size();
}

// k_hop's fixed-length CRC-8 over a header of n bytes (6..16) held in 16 bytes.
int scan_probe_crc8_header_ok(const uint8_t* b, uint32_t n) {
    uint32_t h[4] = {};
    for (int i = 0; i < 16; i++) h[i / 4] |= (uint32_t)b[i] << (8 * (i % 4));
    return crc8_header_ok(h[0], h[1], h[2], h[3], n) ? 1 : 0;
}

}  // extern "C"

#ifdef SCAN_PROBE_MAIN
// scan_probe <fillings> <stream file>...: "masks <wrong>", then per stream "<candidates of form 2>
// <candidates of form 1> <1 if the two lists are equal> <headers whose fixed-length CRC-8 disagrees>".
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::printf("masks %llu\n", (unsigned long long)scan_probe_masks((uint32_t)std::strtoul(argv[1], nullptr, 10), 2));
    for (int a = 2; a < argc; a++) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) return 3;
        std::vector<uint8_t> d;
        uint8_t buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + n);
        std::fclose(f);
        uint64_t p = 4;  // metadata blocks (the streams are the tests' own: well formed)
        for (;;) {
            if (p + 4 > d.size()) return 4;
            const bool last = d[p] & 0x80;
            p += 4 + ((uint64_t)d[p + 1] << 16 | (uint64_t)d[p + 2] << 8 | d[p + 3]);
            if (last) break;
        }
        if (p >= d.size()) return 4;
        const uint32_t si_rate = ((uint32_t)d[18] << 16 | (uint32_t)d[19] << 8 | d[20]) >> 4;
        const uint8_t* q = d.data() + p;
        const FrameHdr h0 = parse_frame_header_t<1>([q](uint32_t i) -> uint32_t { return q[i]; }, d.size() - p, si_rate, CRC8.t);
        StreamDesc S;
        std::memset(&S, 0, sizeof(S));
        S.byte1 = (uint8_t)h0.byte1;
        S.nch = (uint8_t)channels_count(h0.chan_code);
        S.dcode = (uint8_t)h0.dcode;
        S.rate_hz = h0.rate;
        S.si_rate = si_rate;
        const Found r = walk(d.data(), d.size(), p, S, 2), t = walk(d.data(), d.size(), p, S, 1);
        unsigned crc_wrong = 0;
        for (size_t i = 0; i < t.pos.size(); i++) {
            uint8_t b[16] = {};
            for (uint32_t k = 0; k < 16 && t.pos[i] + k < d.size(); k++) b[k] = d[t.pos[i] + k];
            crc_wrong += scan_probe_crc8_header_ok(b, t.hdr_len[i]) != 1;
        }
        std::printf("%zu %zu %d %u\n", r.pos.size(), t.pos.size(), (int)(r.pos == t.pos && r.bs == t.bs && r.hdr_len == t.hdr_len),
                    crc_wrong);
    }
    return 0;
}
#endif
