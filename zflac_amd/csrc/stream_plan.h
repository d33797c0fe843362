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

// ---- the choice of front (k_scan or k_hop, hop.hip) ----------------------------------
enum Front : int { FRONT_SCAN = 1, FRONT_HOP = 2 };  // ZFLAC_FRONT_* of zflac_hip.h
enum FrontMode : int { FRONT_AUTO = 0, FRONT_FORCE_SCAN = 1, FRONT_FORCE_HOP = 2 };

struct HopLimits {
    uint32_t max_frames = HOP_MAX_FRAMES;    // frames per stream, at most
    uint32_t min_streams = HOP_MIN_STREAMS;  // streams per class, at least (not applied when forced)
};

// Can k_hop follow this stream? A STREAMINFO total, fixed blocking (first frame 0xF8 and
// STREAMINFO min block == max block >= 16: frame i carries the coded number i and zflac reads
// exactly ceil(total / block) frames), at most max_frames of them, and under 2 GiB of frames
// (k_hop's positions are 32-bit).
bool hop_stream_ok(const StreamPlan& s, uint32_t max_frames);
// Frames of a hop-eligible stream: ceil(total / block).
uint32_t hop_frames(const StreamPlan& s);
// The front of a class of `n` streams, and for FRONT_HOP its per-stream descriptors (f0 the
// running sum of n_frames, guess = frame bytes / n_frames) and their frame total.
// FRONT_FORCE_HOP still needs every stream to pass hop_stream_ok; it only drops min_streams.
Front plan_hop(const StreamPlan* const* streams, size_t n, FrontMode mode, const HopLimits& lim, HopDesc* out,
               uint64_t* total_frames);

}  // namespace zflac
