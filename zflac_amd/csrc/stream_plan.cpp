// stream_plan.cpp -- host-side parsing with zflac semantics (see stream_plan.h).
//
// Reference: Senryoku/zflac src/zflac.zig (decode :217-310).
#include "stream_plan.h"

#include <cstring>

namespace zflac {

namespace {
struct ByteReader {
    const uint8_t* d;
    size_t n;
    size_t pos = 0;
    bool get(size_t k, uint64_t& v) {  // readInt(uK*8, .big)
        if (n - pos < k) return false;
        v = 0;
        for (size_t i = 0; i < k; i++) v = (v << 8) | d[pos + i];
        pos += k;
        return true;
    }
};
}  // namespace

int parse_metadata(const uint8_t* d, size_t n, StreamInfoH& si, size_t& frames_begin) {
    ByteReader r{d, n};
    uint64_t v;
    if (!r.get(4, v)) return E_END_OF_STREAM;
    if (v != 0x664C6143) return E_INVALID_SIGNATURE;  // :218-220
    bool have = false;
    for (;;) {
        uint64_t h;
        if (!r.get(4, h)) return E_END_OF_STREAM;
        const unsigned info = (unsigned)(h >> 24) & 0x7F;
        const bool last = (h >> 31) & 1;
        const uint64_t length = h & 0xFFFFFF;
        if (info == 0) {  // STREAMINFO, always 34 bytes (:228-240)
            if (r.n - r.pos < 34) return E_END_OF_STREAM;
            const uint8_t* p = d + r.pos;
            si.min_block = (uint16_t)((p[0] << 8) | p[1]);
            si.max_block = (uint16_t)((p[2] << 8) | p[3]);
            si.sample_rate = ((uint32_t)p[10] << 12) | ((uint32_t)p[11] << 4) | (p[12] >> 4);
            si.channels = ((p[12] >> 1) & 7) + 1;
            si.bps = (((p[12] & 1) << 4) | (p[13] >> 4)) + 1;
            si.total = ((uint64_t)(p[13] & 15) << 32) | ((uint64_t)p[14] << 24) | ((uint64_t)p[15] << 16) |
                       ((uint64_t)p[16] << 8) | p[17];
            std::memcpy(si.md5, p + 18, 16);
            r.pos += 34;
            have = true;
        } else if (info >= 1 && info <= 6) {  // skipped (:243-247)
            if (r.n - r.pos < length) return E_END_OF_STREAM;
            r.pos += length;
        } else {
            return E_INVALID_METADATA_HEADER;  // :248
        }
        if (last) break;
    }
    if (!have) return E_MISSING_STREAMINFO;  // :309
    frames_begin = r.pos;
    return E_OK;
}

int kind_of_bps(uint32_t bps) {
    const uint32_t aligned = (bps + 7) / 8 * 8;  // src/zflac.zig:256-264
    if (aligned == 8) return 0;
    if (aligned == 16) return 1;
    return 2;
}
int esz_of_kind(int kind) { return kind == 0 ? 1 : (kind == 1 ? 2 : 4); }
uint8_t justify_of(uint32_t bps) {  // src/zflac.zig:287-306
    if (bps >= 9 && bps <= 15) return (uint8_t)(16 - bps);
    if (bps >= 17 && bps <= 31) return (uint8_t)(32 - bps);
    return 0;
}

void plan_stream(StreamPlan& s, const uint8_t* d, size_t n) {
    s.len = n;
    s.host_err = parse_metadata(d, n, s.si, s.frames_begin);
    if (s.host_err) return;
    s.kind = kind_of_bps(s.si.bps);
    s.nch = (int)s.si.channels;
    const bool valid_total = s.si.total > 0;
    const uint64_t avail = n - s.frames_begin;
    if (avail < 4) {  // readInt(u32) of the first frame header fails (:343-350)
        if (valid_total) s.host_err = E_END_OF_STREAM;
        else s.no_frames = true;
        return;
    }
    const uint8_t* p = d + s.frames_begin;
    s.first = parse_frame_header_t<0>([p](uint32_t i) -> uint32_t { return p[i]; }, avail, s.si.sample_rate, nullptr);
    if (s.first.err) { s.host_err = s.first.err; return; }
    if (depth_bits(s.first.dcode, (int)s.si.bps) < 0) { s.host_err = E_OUT_OF_DOMAIN; return; }  // :143
    if (channels_count(s.first.chan_code) != s.nch) { s.host_err = E_INCONSISTENT_PARAMETERS; return; }  // :386
}

uint32_t hop_frames(const StreamPlan& s) {
    const uint64_t bs = s.si.min_block;
    return bs ? (uint32_t)((s.si.total + bs - 1) / bs) : 0;
}

bool hop_stream_ok(const StreamPlan& s, uint32_t max_frames) {
    if (s.host_err || s.no_frames || s.si.total == 0) return false;
    if (s.si.min_block != s.si.max_block || s.si.min_block < 16 || s.first.byte1 != 0xF8) return false;
    if ((s.si.total + s.si.min_block - 1) / s.si.min_block > max_frames) return false;
    return s.len - s.frames_begin < (1ull << 31);
}

Front plan_hop(const StreamPlan* const* streams, size_t n, FrontMode mode, const HopLimits& lim, HopDesc* out,
               uint64_t* total_frames) {
    if (total_frames) *total_frames = 0;
    if (mode == FRONT_FORCE_SCAN || n == 0) return FRONT_SCAN;
    if (mode == FRONT_AUTO && n < lim.min_streams) return FRONT_SCAN;
    uint64_t f0 = 0;
    for (size_t i = 0; i < n; i++) {
        const StreamPlan& s = *streams[i];
        if (!hop_stream_ok(s, lim.max_frames)) return FRONT_SCAN;
        const uint32_t nf = hop_frames(s);
        if (f0 + nf > 0x7FFFFFFFull) return FRONT_SCAN;
        if (out) {
            out[i].n_frames = nf;
            out[i].f0 = (uint32_t)f0;
            out[i].units = (uint32_t)s.si.min_block * (uint32_t)s.nch;
            out[i].guess = (uint32_t)((s.len - s.frames_begin) / nf);
        }
        f0 += nf;
    }
    if (total_frames) *total_frames = f0;
    return FRONT_HOP;
}

}  // namespace zflac
