// stream_plan.h -- host planning of one stream with zflac semantics: the metadata blocks and
// the first frame header, everything a stream's verdict or class needs before the GPU sees
// it. No HIP: this and stream_plan.cpp compile as plain C++20.
#pragma once
#include <cstddef>
#include <cstdint>

#include "common.h"
#include "frame_header.h"

namespace zflac {

struct StreamInfoH {
    uint16_t min_block = 0, max_block = 0;
    uint32_t sample_rate = 0;
    uint32_t channels = 0;  // count
    uint32_t bps = 0;       // bits
    uint64_t total = 0;     // per channel
    uint8_t md5[16] = {};
};

// What plan_stream learns about a stream (StreamState, batch.h, extends it).
struct StreamPlan {
    int host_err = 0;  // error known without the GPU (metadata / first frame header)
    StreamInfoH si;
    size_t len = 0;
    size_t frames_begin = 0;
    int kind = 1;
    int nch = 0;
    FrameHdr first = {};
    bool no_frames = false;  // empty frame section, total unknown: zero samples, no error
};

// decode() up to the first frame (src/zflac.zig:217-253)
int parse_metadata(const uint8_t* d, size_t n, StreamInfoH& si, size_t& frames_begin);

int kind_of_bps(uint32_t bps);     // container kind of a bit depth (src/zflac.zig:256-264)
int esz_of_kind(int kind);         // its element size in bytes
uint8_t justify_of(uint32_t bps);  // left-justify shift (src/zflac.zig:287-306)

// Host planning of one stream: metadata and the first frame header.
void plan_stream(StreamPlan& s, const uint8_t* d, size_t n);

}  // namespace zflac
