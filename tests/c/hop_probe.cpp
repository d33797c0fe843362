// hop_probe.cpp -- test shim (tests/test_hop_plan.py): the host side of the hop front without a
// GPU: the coded-number value and the header fields of frame_header.h, and the choice of front
// and per-stream hop descriptors of stream_plan.cpp. Built with plain g++.
#include <vector>

#include "stream_plan.h"

extern "C" {

struct hop_hdr {
    unsigned bs, rate, hdr_len, chan_code, dcode, byte1, zero_bit, bs_code;
    int err, crc_eof, crc_ok;
    int num_ok;                // coded_number_value succeeded
    unsigned long long number;
};

// The header at `p` (`avail` bytes left in the stream), CRC-8 computed in registers as k_hop does.
void hop_probe_header(const unsigned char* p, size_t avail, unsigned si_rate, hop_hdr* out) {
    auto at = [p](uint32_t i) -> uint32_t { return p[i]; };
    const zflac::FrameHdr h = zflac::parse_frame_header_t<2>(at, avail, si_rate, nullptr);
    out->bs = h.bs;
    out->rate = h.rate;
    out->hdr_len = h.hdr_len;
    out->chan_code = h.chan_code;
    out->dcode = h.dcode;
    out->byte1 = h.byte1;
    out->zero_bit = h.zero_bit;
    out->bs_code = h.bs_code;
    out->err = h.err;
    out->crc_eof = h.crc_eof ? 1 : 0;
    out->crc_ok = h.crc_ok ? 1 : 0;
    uint64_t v = 0;
    out->num_ok = zflac::coded_number_value(at, avail, v) ? 1 : 0;
    out->number = v;
}

struct hop_desc {
    unsigned n_frames, f0, units, guess;
};

// plan_hop over `n` whole streams. Returns the front (1 scan, 2 hop); for hop, out[i] and *total.
int hop_probe_plan(const unsigned char* const* data, const size_t* len, size_t n, int mode, unsigned max_frames,
                   unsigned min_streams, hop_desc* out, unsigned long long* total) {
    std::vector<zflac::StreamPlan> plans(n);
    std::vector<const zflac::StreamPlan*> ptr(n);
    for (size_t i = 0; i < n; i++) {
        zflac::plan_stream(plans[i], data[i], len[i]);
        ptr[i] = &plans[i];
    }
    zflac::HopLimits lim;
    lim.max_frames = max_frames;
    lim.min_streams = min_streams;
    std::vector<zflac::HopDesc> d(n);
    uint64_t t = 0;
    const zflac::Front f = zflac::plan_hop(ptr.data(), n, (zflac::FrontMode)mode, lim, d.data(), &t);
    for (size_t i = 0; i < n && f == zflac::FRONT_HOP; i++) out[i] = {d[i].n_frames, d[i].f0, d[i].units, d[i].guess};
    *total = t;
    return (int)f;
}

unsigned hop_probe_default_max_frames() { return zflac::HOP_MAX_FRAMES; }
unsigned hop_probe_default_min_streams() { return zflac::HOP_MIN_STREAMS; }

}  // extern "C"
