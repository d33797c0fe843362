// hop.hip -- k_hop: the frame table of a batch of many short fixed-blocking streams, built by
// hopping from one frame header to the next instead of scanning every input byte.
//
// zflac itself never scans for sync codes: it reads one frame after another
// (src/zflac.zig:340-581). k_scan reads every byte because a lone long stream offers no other
// parallelism; a batch of many streams does, across the streams. A stream with fixed blocking
// (first frame 0xF8, STREAMINFO min block == max block) and a STREAMINFO total has exactly
// ceil(total / block) frames, and frame i carries the coded number i. So from a known header at
// p the next one is found by reading one 1 KiB window around p + (the previous frame's size)
// and taking the header whose number is i + 1. A stream is a chain of n_frames dependent small
// reads, the streams of the class run side by side, and nothing waits for anything else.
//
// A candidate is accepted by the same filter as k_scan's (exact header parse, CRC-8, the first
// frame's parameters) plus its number, and the table goes through k_verify as the scan's does,
// so a wrong hop can only send a stream to the sequential planner, never change its samples. A
// stream the hop cannot follow (no header with the right number within the probe budget) marks
// the run `hop_failed`: the host redoes the class with the scan front and keeps it there.
#include "device_common.h"
#include "launch.h"

namespace zflac {

constexpr int HOP_LANES = 16;        // lanes per stream: a quarter wave
constexpr int HOP_LANE_BYTES = 64;   // bytes of the window a lane searches (it loads 16 more: a header's tail)
constexpr int HOP_WINDOW = HOP_LANES * HOP_LANE_BYTES;  // 1 KiB
constexpr int HOP_PROBES = 16;       // windows per hop, at most
constexpr int HOP_THREADS = 64;      // one wave: four streams

__device__ __forceinline__ uint32_t hop_group_min(uint32_t v) {
#pragma unroll
    for (int m = HOP_LANES / 2; m; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m, HOP_LANES));
    return v;
}

// One lane's share of a probe: the lowest position (relative to `abase`) in [lo, end) of its
// 64 bytes at `off` that holds an acceptable header numbered `want` whose block size x channels
// is `want_units` (~0u: none), and whether it holds one with a higher number. The table's output
// offsets are i x (STREAMINFO block x channels), which k_verify does not check against the
// headers (under the scan front k_compact derives them from the headers themselves): a frame
// with the right number and another block size is therefore no hit, the hop is lost there and
// the class goes back to the scan front, which places every frame by its own header as zflac does.
struct HopHit {
    uint32_t pos, higher;
};

__device__ __forceinline__ HopHit hop_probe_lane(const __amdgpu_buffer_rsrc_t rs, const StreamDesc& S, uint64_t abase,
                                                 int64_t off, uint32_t lo, uint32_t end, uint64_t want,
                                                 uint64_t want_units) {
    HopHit hit{~0u, 0u};
    if (off < 0 || off >= (int64_t)end) return hit;
    // 80 bytes: the lane's 64 and the 16 after them, so that a header (at most 16 bytes) that
    // starts in its last byte is whole; past the stream the buffer unit answers with zeros
    uint32_t d[20];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint4 v = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, (uint32_t)off, j * 16, 0));
        d[4 * j] = v.x;
        d[4 * j + 1] = v.y;
        d[4 * j + 2] = v.z;
        d[4 * j + 3] = v.w;
    }
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) any |= sync_any(d[i], d[i + 1]);
    if (!any) return hit;
    uint64_t cand = 0;  // bit b: a sync code at byte b of the lane's 64
#pragma unroll
    for (int i = 0; i < 16; i++)
        cand |= (uint64_t)((sync_mask(d[i], d[i + 1]) * 0x00204081u) >> 28 & 15u) << (4 * i);
    while (cand) {
        const uint32_t b = (uint32_t)__ffsll((unsigned long long)cand) - 1u;
        cand &= cand - 1;
        const uint64_t rel = (uint64_t)off + b;
        if (rel < lo || rel >= end) continue;
        // dwords b/4 .. b/4 + 4 picked with constant indices (80 v_cndmask per candidate; an
        // indexed register array, or a select tree the compiler folds into one, becomes scratch
        // stores on every probe), then v_alignbyte by b & 3: header bytes 0..15 in four registers
        const uint32_t dw = b >> 2, sb = b & 3u;
        uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0, w4 = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const bool here = dw == (uint32_t)i;
            w0 = here ? d[i] : w0;
            w1 = here ? d[i + 1] : w1;
            w2 = here ? d[i + 2] : w2;
            w3 = here ? d[i + 3] : w3;
            w4 = here ? d[i + 4] : w4;
        }
        const uint32_t h0 = __builtin_amdgcn_alignbyte(w1, w0, sb), h1 = __builtin_amdgcn_alignbyte(w2, w1, sb),
                       h2 = __builtin_amdgcn_alignbyte(w3, w2, sb), h3 = __builtin_amdgcn_alignbyte(w4, w3, sb);
        auto at = [h0, h1, h2, h3](uint32_t i) -> uint32_t {  // byte i: v_perm from 8 bytes, zeros above
            const uint32_t sel = (i & 7u) | 0x0C0C0C00u;
            return (i & 8u) ? __builtin_amdgcn_perm(h3, h2, sel) : __builtin_amdgcn_perm(h1, h0, sel);
        };
        const uint64_t avail = S.in_end - (abase + rel);
        const FrameHdr h = parse_frame_header_t<2>(at, avail, S.si_rate, nullptr);
        if (!candidate_ok(h, S)) continue;
        uint64_t num;
        if (!coded_number_value(at, avail, num)) continue;
        if (num == want) {
            // (ascending: the first is the lowest)
            if (hit.pos == ~0u && (uint64_t)h.bs * S.nch == want_units) hit.pos = (uint32_t)rel;
        } else if (num > want) {
            hit.higher = 1;
        }
    }
    return hit;
}

// One 16-lane group per stream; see the file header. Every loop is bounded (n_frames x
// HOP_PROBES probes per stream), every read goes through a buffer resource over the stream's
// own bytes, and no lane or workgroup waits for another.
__global__ __launch_bounds__(HOP_THREADS) void k_hop(HopArgs a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the run's counters (k_scan's zero_run_words)
        a.misc[0] = a.total_frames;             // the frame count: known before the run
        a.misc[1] = 0;
        a.misc[2] = 0;
    }
    const uint32_t s = (blockIdx.x * HOP_THREADS + threadIdx.x) / HOP_LANES;
    if (s >= a.n_streams) return;  // (whole groups: HOP_THREADS is a multiple of HOP_LANES)
    const uint32_t ln = threadIdx.x & (HOP_LANES - 1);
    const StreamDesc S = a.streams[s];
    const HopDesc H = a.hop[s];
    const uint64_t abase = S.in_begin & ~(uint64_t)15;
    // positions below are relative to abase; the host only plans the hop for streams under 2 GiB
    const uint32_t end = (uint32_t)(S.in_end - abase);
    const uint32_t begin = (uint32_t)(S.in_begin - abase);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(a.in) + abase, (short)0, (int)((end + 15u) & ~15u), 0x00020000);
    auto put = [&](uint32_t i, uint64_t pos) {  // table entry of the stream's frame i
        if (ln == 0 && H.f0 + i < a.cap) {
            a.c_pos[H.f0 + i] = pos;
            a.c_stream[H.f0 + i] = s;
            a.c_out[H.f0 + i] = S.out_base + (uint64_t)i * H.units;
        }
    };
    // frame 0 lies at in_begin and is validated like any other candidate
    uint32_t cur;
    {
        const HopHit hit = hop_probe_lane(rs, S, abase, (int64_t)ln * HOP_LANE_BYTES, begin, end, 0,
                                          H.n_frames > 1 ? (uint64_t)H.units : S.total);
        cur = hop_group_min(hit.pos);
    }
    bool failed = cur != begin;
    uint32_t done = 0;  // frames found
    if (!failed) {
        put(0, S.in_begin);
        done = 1;
        uint32_t guess = H.guess;
        for (uint32_t f = 0; f + 1 < H.n_frames; f++) {  // group-uniform
            // windows ws0 + k * HOP_WINDOW, k = 0 first, centred on the guess and never before
            // the current header; then outwards, alternating, until a window tells the side
            // (a header with a higher number: the wanted one lies before it)
            const int64_t lo_ws = (int64_t)((cur + 1u) & ~15u);
            int64_t ws0 = ((int64_t)cur + guess - HOP_WINDOW / 2) & ~(int64_t)15;
            if (ws0 < lo_ws) ws0 = lo_ws;
            // every frame holds a full block but the last, which holds the rest of the total
            const uint64_t want_units = f + 2 < H.n_frames ? (uint64_t)H.units : S.total - (uint64_t)(f + 1) * H.units;
            int fwd = 0, back = -1, dir = 0;
            uint32_t found = ~0u;
#pragma unroll 1
            for (int pr = 0; pr < HOP_PROBES; pr++) {
                const bool back_ok = ws0 + (int64_t)(back + 1) * HOP_WINDOW > lo_ws;
                const bool fwd_ok = ws0 + (int64_t)fwd * HOP_WINDOW < (int64_t)end;
                bool go_back = dir < 0 || (dir == 0 && (pr & 1));
                if (go_back && !back_ok) {
                    if (dir < 0) break;
                    go_back = false;
                }
                if (!go_back && !fwd_ok) {
                    if (dir > 0 || !back_ok) break;
                    go_back = true;
                }
                const int k = go_back ? back-- : fwd++;
                const int64_t ws = ws0 + (int64_t)k * HOP_WINDOW;
                const HopHit hit = hop_probe_lane(rs, S, abase, ws + (int64_t)ln * HOP_LANE_BYTES, cur + 1u, end,
                                                  (uint64_t)f + 1, want_units);
                found = hop_group_min(hit.pos);
                if (found != ~0u) break;
                if (hop_group_min(hit.higher ? 0u : 1u) == 0u) dir = -1;
                else if (!back_ok) dir = 1;
            }
            if (found == ~0u) {
                failed = true;
                break;
            }
            guess = found - cur;  // the size just found
            cur = found;
            put(f + 1, abase + cur);
            done = f + 2;
        }
    }
    // a stream the hop lost: its other frames at the stream's end, where the decode kernels
    // read no header and write nothing (the host redoes the class with the scan front)
    for (uint32_t i = done; i < H.n_frames; i++) put(i, S.in_end);
    if (ln == 0) {
        a.chunk_off[S.first_chunk] = H.f0;  // the two entries k_verify reads per stream
        a.chunk_off[S.end_chunk] = H.f0 + H.n_frames;
        a.status[s] = failed ? 2u : 0u;
        if (failed) a.misc[3] = a.epoch;  // hop_failed: this run's own mark (nothing zeroes it, so no race)
    }
}

hipError_t launch_hop(const HopArgs& a, hipStream_t st) {
    if (a.n_streams == 0) return hipSuccess;
    const uint32_t per = HOP_THREADS / HOP_LANES;
    hipLaunchKernelGGL(k_hop, dim3((a.n_streams + per - 1) / per), dim3(HOP_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace zflac
