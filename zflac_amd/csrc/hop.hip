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

// Minimum over the 16 lanes of a stream's group. A group is one DPP row, so the four steps are
// v_min_u32 with a DPP operand (the lane's quad neighbours, then the row rotated by 4 and by 8)
// and no LDS permute. Lanes of a group are active together wherever this is called.
__device__ __forceinline__ uint32_t hop_group_min(uint32_t v) {
    static_assert(HOP_LANES == 16, "a group is one DPP row");
    auto step = [](uint32_t x, auto ctrl) {
        return min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, decltype(ctrl)::value, 0xF, 0xF, false));
    };
    v = step(v, std::integral_constant<int, 0xB1>{});   // quad_perm:[1,0,3,2]
    v = step(v, std::integral_constant<int, 0x4E>{});   // quad_perm:[2,3,0,1]
    v = step(v, std::integral_constant<int, 0x124>{});  // row_ror:4
    v = step(v, std::integral_constant<int, 0x128>{});  // row_ror:8
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
    // (Twenty named registers, not an array: an array indexed inside an unrolled loop or a lambda is
    // still memory when the optimiser first meets a select between two of its elements, which it
    // folds into one load at a selected address, and that ends as scratch stores on every probe.)
#define HOP_LOAD(j, a, b, c, e)                                                                                    \
    uint32_t a, b, c, e;                                                                                           \
    {                                                                                                              \
        const uint4 v = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, (uint32_t)off, (j) * 16, 0)); \
        a = v.x, b = v.y, c = v.z, e = v.w;                                                                        \
    }
    HOP_LOAD(0, d0, d1, d2, d3)
    HOP_LOAD(1, d4, d5, d6, d7)
    HOP_LOAD(2, d8, d9, d10, d11)
    HOP_LOAD(3, d12, d13, d14, d15)
    HOP_LOAD(4, d16, d17, d18, d19)
#undef HOP_LOAD
    // The sync codes of the lane's 64 bytes, found once (the cheaper existence test that k_scan
    // runs first is no saving here: the wanted header makes it fire in every probe of every
    // group). Two registers of 8 dwords each: bit 8 y + x of c0 is byte y of dword x, of c1 byte y
    // of dword 8 + x, so a dword's four marks (bits 7, 15, 23, 31) go in with one shift and one or.
    const uint32_t c0_all = sync_mask(d0, d1) >> 7 | sync_mask(d1, d2) >> 6 | sync_mask(d2, d3) >> 5 |
                            sync_mask(d3, d4) >> 4 | sync_mask(d4, d5) >> 3 | sync_mask(d5, d6) >> 2 |
                            sync_mask(d6, d7) >> 1 | sync_mask(d7, d8);
    const uint32_t c1_all = sync_mask(d8, d9) >> 7 | sync_mask(d9, d10) >> 6 | sync_mask(d10, d11) >> 5 |
                            sync_mask(d11, d12) >> 4 | sync_mask(d12, d13) >> 3 | sync_mask(d13, d14) >> 2 |
                            sync_mask(d14, d15) >> 1 | sync_mask(d15, d16);
    uint32_t c0 = c0_all, c1 = c1_all;
    while (c0 | c1) {  // (in no order of position: the lowest hit is kept by a minimum below)
        const bool first = c0 != 0;
        const uint32_t cc = first ? c0 : c1;
        const uint32_t bit = (uint32_t)__ffs((int)cc) - 1u;
        c0 = first ? cc & (cc - 1u) : c0;
        c1 = first ? c1 : cc & (cc - 1u);
        const uint32_t dw = (bit & 7u) + (first ? 0u : 8u), sb = bit >> 3;
        const uint64_t rel = (uint64_t)off + 4u * dw + sb;
        if (rel < lo || rel >= end) continue;
        // dwords dw .. dw + 4 in two levels of selects: the eight dwords from quad dw / 4 on (3
        // v_cndmask each), then five of those from dword dw % 4 on (3 each): 39 v_cndmask, where one
        // level over the 16 positions took 80. Then v_alignbyte by sb: header bytes 0..15 in four
        // registers
        const bool q1 = (dw >> 2) == 1u, q2 = (dw >> 2) == 2u, q3 = (dw >> 2) == 3u;
#define HOP_QUAD(a, b, c, e) (q3 ? (e) : (q2 ? (c) : (q1 ? (b) : (a))))
        const uint32_t e0 = HOP_QUAD(d0, d4, d8, d12), e1 = HOP_QUAD(d1, d5, d9, d13), e2 = HOP_QUAD(d2, d6, d10, d14),
                       e3 = HOP_QUAD(d3, d7, d11, d15), e4 = HOP_QUAD(d4, d8, d12, d16), e5 = HOP_QUAD(d5, d9, d13, d17),
                       e6 = HOP_QUAD(d6, d10, d14, d18), e7 = HOP_QUAD(d7, d11, d15, d19);
#undef HOP_QUAD
        const bool r1 = (dw & 3u) == 1u, r2 = (dw & 3u) == 2u, r3 = (dw & 3u) == 3u;
#define HOP_WORD(a, b, c, e) (r3 ? (e) : (r2 ? (c) : (r1 ? (b) : (a))))
        const uint32_t w0 = HOP_WORD(e0, e1, e2, e3), w1 = HOP_WORD(e1, e2, e3, e4), w2 = HOP_WORD(e2, e3, e4, e5),
                       w3 = HOP_WORD(e3, e4, e5, e6), w4 = HOP_WORD(e4, e5, e6, e7);
#undef HOP_WORD
        const uint32_t h0 = __builtin_amdgcn_alignbyte(w1, w0, sb), h1 = __builtin_amdgcn_alignbyte(w2, w1, sb),
                       h2 = __builtin_amdgcn_alignbyte(w3, w2, sb), h3 = __builtin_amdgcn_alignbyte(w4, w3, sb);
        auto at = [h0, h1, h2, h3](uint32_t i) -> uint32_t {  // byte i: v_perm from 8 bytes, zeros above
            const uint32_t sel = (i & 7u) | 0x0C0C0C00u;
            return (i & 8u) ? __builtin_amdgcn_perm(h3, h2, sel) : __builtin_amdgcn_perm(h1, h0, sel);
        };
        const uint64_t avail = S.in_end - (abase + rel);
        // the fields, then the CRC-8 over the header's own length in a fixed number of steps
        // (crc8_header_ok; read only where the header is whole: hdr_len is 6..16 there)
        FrameHdr h = parse_frame_header_t<0>(at, avail, S.si_rate, nullptr);
        h.crc_ok = h.err == 0 && !h.crc_eof && crc8_header_ok(h0, h1, h2, h3, h.hdr_len);
        if (!candidate_ok(h, S)) continue;
        uint64_t num;
        if (!coded_number_value(at, avail, num)) continue;
        if (num == want) {
            if ((uint64_t)h.bs * S.nch == want_units) hit.pos = min(hit.pos, (uint32_t)rel);  // the lowest
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
