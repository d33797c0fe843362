// decode/kernels.h -- frame setup, k_walk, k_decode and their host launches.
#pragma once
#include <atomic>

#include "../launch.h"
#include "run_subframe.h"

namespace zflac {

// Per-lane frame setup shared by k_walk and k_decode: the wave's input window, the frame
// header (exact zflac semantics, src/zflac.zig:343-405), the lane reader's base and the
// output placement. `L.ubps` is left to the caller (it depends on the channel).
struct FrameSetup {
    LaneCtx L;
    FrameCtx fc;
    uint64_t pos;
    uint32_t hdr_info, rate, start;
    bool frame_ok;
};

__device__ __forceinline__ bool is_side_channel(uint32_t code, int c) {  // src/zflac.zig:436-441
    return (code == 8 && c == 1) || (code == 9 && c == 0) || (code == 10 && c == 1);
}

// `dec`: k_decode's LDS layout (junk slots in the wave's output stage), else k_walk's.
__device__ __forceinline__ void setup_frame(const DecodeArgs& a, uint32_t f, bool fvalid, int nch, uint32_t lds_lane,
                                            int esz, Rdr& rd, FrameSetup& s, bool dec) {
    s.L = LaneCtx{};
    s.fc = FrameCtx{};
    s.pos = 0;
    s.hdr_info = s.rate = s.start = 0;
    s.frame_ok = false;
    rd.nb = NB0;
    rd.wr = 0;
#pragma unroll
    for (int q = 0; q < 6; q++) rd.stg[q] = make_uint4(0, 0, 0, 0);
    rd.sv = false;
    // The wave's input window starts at its lowest frame position; lanes address it
    // with 32-bit offsets (buffer loads: out-of-range offsets read zeros, no traffic).
    uint64_t wmin = fvalid ? (a.c_pos[f] & ~(uint64_t)15) : ~0ull;
    for (int o = 32; o > 0; o >>= 1) wmin = min(wmin, (uint64_t)__shfl_xor((unsigned long long)wmin, o));
    const uint64_t wbase = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(wmin >> 32)) << 32) |
                           __builtin_amdgcn_readfirstlane((uint32_t)wmin);
    const uint64_t wlen = a.in_size > wbase ? a.in_size - wbase : 0;
    rd.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.in) + wbase, (short)0,
                                              (int)(wlen > 0x7FFFFFF0ull ? 0x7FFFFFF0ull : wlen), BUFFER_RSRC_WORD3);
    rd.lofs = 0x80000000u;
    rd.qa = 0;
    rd.qmax = 0;
    rd.lds = lds_lane;
    rd.junk = (blockDim.x >> 6) * RING_WAVE_WORDS + (lds_lane / RING_WAVE_WORDS) * (dec ? STAGE_QUADS * 4 : JUNK_WAVE_WORDS) +
              (lds_lane & 63u);
    if (!fvalid) return;
    LaneCtx& L = s.L;
    s.pos = a.c_pos[f];
    const uint64_t pos = s.pos;
    const StreamDesc S = a.streams[a.c_stream[f]];
    const FrameHdr h = parse_frame_fields(a.in + pos, S.in_end > pos ? S.in_end - pos : 0, S.si_rate);
    s.rate = h.rate;
    s.hdr_info = ((h.bs - 1) & 0xFFFFu) | (h.chan_code << 16) | (h.dcode << 20);
    L.bs = h.bs;
    L.chan_code = h.chan_code;
    L.bps = depth_bits(h.dcode, S.si_bps);
    if (h.err) {
        L.err = h.err;
        s.hdr_info |= INFO_PRE_ERR;
    } else if (h.crc_eof) {
        L.err = E_END_OF_STREAM;
        s.hdr_info |= INFO_CRC_EOF;
    } else if (channels_count(h.chan_code) != nch) {
        L.err = E_INCONSISTENT_PARAMETERS;
    } else if (L.bps < 0) {
        L.err = E_OUT_OF_DOMAIN;  // reserved depth code: `unreachable` (:143)
    } else {
        s.frame_ok = true;
    }
    const uint64_t abase = pos & ~(uint64_t)15;
    const uint64_t end_bytes = S.in_end > abase ? S.in_end - abase : 0;
    L.end = end_bytes * 8 > 0xFFFF0000ull ? 0xFFFF0000u : (uint32_t)(end_bytes * 8);
    const uint64_t quads = (S.in_end + INPUT_PAD - abase) / 16;
    // a frame beyond the 2 GiB window reads zeros: its chain check then fails and
    // the stream goes to the sequential planner, whose probes are one frame each
    rd.lofs = abase - wbase < 0x7FFFFFF0ull ? (uint32_t)(abase - wbase) : 0x80000000u;
    rd.qmax = quads > 0x3FFFFFFull ? 0x3FFFFFFu : (uint32_t)quads - 1;
    rd.qa = (uint32_t)(abase >> 4) & 3u;  // (`in` itself is 256-byte aligned)
    s.start = ((uint32_t)(pos & 15) + h.hdr_len) * 8;
    const uint64_t rel = a.c_out[f] - S.out_base;
    const bool in_range = !S.valid_total || rel < S.total;
    s.fc.out_elem = a.c_out[f];
    s.fc.write = a.write && in_range && s.frame_ok && rel + (uint64_t)h.bs * nch <= S.out_cap;
    // packed 16-byte stores need the frame's first output byte 16-byte aligned (absolute
    // address: the sequential path decodes into a sub-range or an override buffer)
    // (and within the first 2^36 bytes of the buffer: the staged write-back of the stereo
    // fast path addresses 16-byte quads with 32-bit indices)
    s.fc.packed = ((reinterpret_cast<uintptr_t>(a.out) + s.fc.out_elem * (uint64_t)esz) & 15) == 0 &&
                  (s.fc.out_elem + 0x20000u) * (uint64_t)esz < (1ull << 36);
    s.fc.justify = S.justify;
}

// ----------------------------------------------------------------------------------
// k_walk: subframe c+1 starts where subframe c ends (src/zflac.zig:425-541 read order), so
// before any lane can decode subframe c >= 1 the bit length of subframes 0..c-1 must be
// known. One lane per frame (64 frames per wave) reads subframes 0..nch-2 without
// producing samples (header, warm-up / coefficient skips, Rice lengths only) and records
// where each following subframe starts, as a bit offset from the frame's 16-byte base.
// ----------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(WALK_THREADS, 2) void k_walk(DecodeArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave_in_block = threadIdx.x >> 6;
    const uint32_t wave = (blockIdx.x * WALK_THREADS + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * WALK_THREADS) >> 6;
    const int nch = a.nch;
    uint32_t nframes = a.n_frames ? *a.n_frames : a.n_frames_host;
    if (nframes > a.cap) nframes = a.cap;
    const uint32_t lds_lane = (uint32_t)(wave_in_block * RING_WAVE_WORDS + lane);
    for (uint32_t g0 = wave * 64u; g0 < nframes; g0 += nwaves * 64u) {
        const uint32_t f = g0 + (uint32_t)lane;
        const bool fvalid = f < nframes;
        Rdr rd;
        FrameSetup s;
        setup_frame(a, f, fvalid, nch, lds_lane, Kind<KIND>::ESZ, rd, s, false);
        uint32_t start = s.start;
        for (int r = 0; r + 1 < nch; r++) {
            LaneCtx W = s.L;
            W.ubps = W.bps + (is_side_channel(W.chan_code, r) ? 1 : 0);
            W.mode = M_NONE;
            if (s.frame_ok) {
                W.mode = M_PRED;
                rd.init(start);
                walk_subframe<KIND>(W, rd);
            }
            uint32_t wbs = W.mode != M_NONE ? W.bs : 0;
            for (int o = 32; o > 0; o >>= 1) wbs = max(wbs, (uint32_t)__shfl_xor((int)wbs, o));
            if (wbs) run_subframe<KIND, 4, LAY_MULTI, true>(W, rd, s.fc, a.out, nch, r, 0, wbs, a.dummy);
            start = s.frame_ok ? rd.pos() : 0u;
            if (fvalid) a.sub_start[(uint64_t)f * MAX_CH + r + 1] = start;
        }
    }
}

// ----------------------------------------------------------------------------------
// k_decode
// ----------------------------------------------------------------------------------
// One kernel per history bucket MB (4, 8, 16, 32 >= the largest predictor order of the
// wave's subframes), launched back to back: a wave decodes its frames only in the launch
// of its bucket. Register allocation is per kernel, so the order-8 code (C3/C5) is not
// sized for the order-32 history. Waves with CONSTANT or VERBATIM subframes among their
// lanes go to the MIX kernels (MB 8 or 32), whose fast path also carries those lanes; the
// pure kernels keep their registers for the predicted-only fast path.
// (Waves per SIMD the register allocation must allow: two for the 16-bit kernels and the small
// 8-bit / 32-bit stereo ones, which fit in 256 VGPRs; one for MB = 32 and MIX, and (round 6) for
// the 3..8-channel kernels and the larger 8-bit and 32-bit stereo buckets, which spilled 18-88
// VGPRs to scratch at two waves per SIMD (tools/kmeta.sh). A single-stream launch of 32k
// frames holds about one wave per SIMD anyway.)
template <int KIND, int LAY, int MB, bool MIX>
__host__ __device__ constexpr int dec_min_waves() {
    if (MB == 32 || MIX || LAY == LAY_MULTI) return 1;
    if (KIND == 0 && MB > 8) return 1;
    if (KIND == 2 && LAY == LAY_STEREO && MB > 4) return 1;
    return 2;
}
// WBR (16-bit stereo / mono only): the staged PCM goes back through a buffer resource
// (Stage::store_rsrc); chosen per launch by the host (DecodeArgs::wb_bytes).
template <int KIND, int LAY, int MB, bool MIX, bool WBR = false>
__global__ __launch_bounds__(DEC_THREADS, (dec_min_waves<KIND, LAY, MB, MIX>())) void k_decode(DecodeArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave_in_block = threadIdx.x >> 6;
    const uint32_t wave = (blockIdx.x * DEC_THREADS + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * DEC_THREADS) >> 6;
    const int nch = LAY == LAY_STEREO ? 2 : (LAY == LAY_MONO ? 1 : a.nch);
    const int F = 64 / nch;
    const int c = lane / F;
    const int j = lane - c * F;
    const bool lane_ok = c < nch;
    const int32_t c1m = c ? -1 : 0;
    uint32_t nframes = a.n_frames ? *a.n_frames : a.n_frames_host;
    if (nframes > a.cap) nframes = a.cap;
    const uint32_t lds_lane = (uint32_t)(wave_in_block * RING_WAVE_WORDS + lane);

    constexpr bool FIRST = MB == 8 && !MIX;  // launched first: finds every group's bucket
    constexpr uint32_t MIX_BIT = 64;
    // the `rest` launch (only of k_decode<*, *, 32, true>): every group whose bucket has no
    // launch of its own (a bucket the host did not predict)
    const bool rest = MB == 32 && MIX && a.rest;
    for (uint32_t g0 = wave * (uint32_t)F; g0 < nframes; g0 += nwaves * (uint32_t)F) {
        if constexpr (!FIRST) {  // wave-uniform, one scalar load
            const uint32_t gmb = a.group_mb[g0 / (uint32_t)F];
            if (rest) {
                if (gmb == 8u || (a.full_mask & bucket_bit(gmb & ~MIX_BIT, (gmb & MIX_BIT) != 0))) continue;
            } else if (gmb != (uint32_t)MB + (MIX ? MIX_BIT : 0u)) {
                continue;
            }
        }
        const uint32_t f = g0 + (uint32_t)j;
        const bool fvalid = lane_ok && f < nframes;
        Rdr rd;
        FrameSetup s;
        setup_frame(a, f, fvalid, nch, lds_lane, Kind<KIND>::ESZ, rd, s, true);
        LaneCtx& L = s.L;
        const FrameCtx& fc = s.fc;
        L.ubps = L.bps + (is_side_channel(L.chan_code, c) ? 1 : 0);
        // subframe c >= 1 starts where k_walk found subframe c-1 to end
        uint32_t start = s.start;
        if (c > 0 && s.frame_ok) start = a.sub_start[(uint64_t)f * MAX_CH + c];
        // ---- decode --------------------------------------------------------------------
        if (s.frame_ok) {
            L.mode = M_PRED;  // active marker until the subframe header is parsed
            rd.init(start);
        }
        uint32_t ord = 0, bs_act = 0;
        bool cv = false;
        if (L.mode != M_NONE) {  // peek the subframe type (header bits 1..6) to size the history
            const uint32_t t = (rd.hi() >> 25) & 63;
            ord = (t >= 32) ? t - 31 : ((t >= 8 && t <= 12) ? t - 8 : 0);
            cv = t <= 1;  // CONSTANT / VERBATIM
            bs_act = L.bs;
        }
        for (int o = 32; o > 0; o >>= 1) {
            ord = max(ord, (uint32_t)__shfl_xor((int)ord, o));
            bs_act = max(bs_act, (uint32_t)__shfl_xor((int)bs_act, o));
        }
        const bool mix = __builtin_amdgcn_ballot_w64(cv) != 0;
        const uint32_t mb = mix ? (ord <= 8 ? 8u + MIX_BIT : 32u + MIX_BIT)
                                : (ord <= 4 ? 4u : (ord <= 8 ? 8u : (ord <= 12 ? 12u : (ord <= 16 ? 16u : 32u))));
        if constexpr (FIRST) {
            if (lane == 0) {
                a.group_mb[g0 / (uint32_t)F] = mb;
                if (a.bucket_used) atomicOr(a.bucket_used, bucket_bit(mb & ~MIX_BIT, (mb & MIX_BIT) != 0));
            }
        }
        if (!rest && mb != (uint32_t)MB + (MIX ? MIX_BIT : 0u)) continue;  // another launch decodes this wave's frames
        run_subframe<KIND, MB, LAY, false, MIX, WBR>(L, rd, fc, a.out, nch, c, c1m, bs_act, a.dummy, a.wb_bytes);

        // ---- frame end and record -----------------------------------------------------
        uint32_t endbits = (rd.pos() + 7) & ~7u;  // alignToByte (:546)
        // the subframe's error: a read error first, else a value out of range (zflac reads
        // all residuals before it predicts)
        int lerr = L.err ? L.err : (L.dom ? (int)E_OUT_OF_DOMAIN : 0);
        if (s.frame_ok && !lerr && c == nch - 1 && endbits + 16 > L.end) lerr = E_END_OF_STREAM;  // CRC-16 (:548)
        int ferr = 0;  // first error in channel order
        uint32_t dcr = 0;
        for (int cc = nch - 1; cc >= 0; cc--) {
            const int e = __shfl(lerr, cc * F + j);
            if (e) ferr = e;
            dcr |= (uint32_t)__shfl((int)L.dcr, cc * F + j);
        }
        if (LAY == LAY_STEREO && !ferr && dcr) ferr = E_OUT_OF_DOMAIN;  // decorrelation, after the CRC (:553)
        const uint32_t last_end = (uint32_t)__shfl((int)endbits, (nch - 1) * F + j);
        if (fvalid && c == 0) {
            a.c_err[f] = ferr;
            a.c_info[f] = s.hdr_info;
            a.c_rate[f] = s.rate;
            a.c_end[f] = (s.pos & ~(uint64_t)15) + last_end / 8 + 2;
        }
    }
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) of one kernel, once per device: the
// attribute belongs to the kernel's instance on the current device, so a process that
// decodes on several devices sets it on each (`done`: one bit per device already set).
__host__ inline hipError_t set_lds_limit(std::atomic<uint64_t>& done, const void* fn, size_t bytes) {
    int dev = 0;
    if (const hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_acq_rel);
    return e;
}

template <int KIND>
hipError_t launch_walk_kind(const DecodeArgs& a, uint32_t max_frames, hipStream_t st) {
    static std::atomic<uint64_t> lds_set{0};
    if (const hipError_t e = set_lds_limit(lds_set, reinterpret_cast<const void*>(&k_walk<KIND>), WALK_LDS_BYTES);
        e != hipSuccess)
        return e;
    uint32_t waves = (max_frames + 63) / 64;
    uint32_t blocks = (waves + WALK_THREADS / 64 - 1) / (WALK_THREADS / 64);
    if (blocks > 8192) blocks = 8192;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL((k_walk<KIND>), dim3(blocks), dim3(WALK_THREADS), WALK_LDS_BYTES, st, a);
    return hipGetLastError();
}

template <int KIND, int LAY>
__host__ __forceinline__ dim3 decode_grid(const DecodeArgs& a, uint32_t max_frames) {
    const uint32_t F = 64 / (uint32_t)a.nch;
    uint32_t waves = (max_frames + F - 1) / F;
    uint32_t blocks = (waves + DEC_WAVES - 1) / DEC_WAVES;
    if (blocks > 8192) blocks = 8192;
    if (blocks == 0) blocks = 1;
    return dim3(blocks);
}

// Does bucket (mb, mix) get a launch of its own? Always for order 8 (it classifies every
// frame group), else when the host predicts it (DecodeArgs::full_mask; 0 = every bucket).
__host__ __forceinline__ bool bucket_launched(const DecodeArgs& a, uint32_t mb, bool mix) {
    return a.full_mask == 0 || (a.full_mask & bucket_bit(mb, mix)) || (mb == 8 && !mix);
}

// Pure (predicted-only) bucket kernels. Bucket 8 first: it records every frame group's
// bucket in a.group_mb for the others. The MIX kernels (launch_decode_mix) live in their own
// translation unit (decode_k*_*_mix.hip), so this code object holds only the pure kernels.
// A bucket the host does not predict costs no launch: its groups (if any) are decoded by
// the `rest` launch (launch_decode_mix with rest_only), which the host issues only after a
// run that needed it (each empty launch costs ~5 us of a ~0.55 ms step, and far more with
// several runs in flight, where it waits for LDS to dispatch).
// The staged write-back of a launch: through the buffer resource when the host offers one
// (DecodeArgs::wb_bytes != 0) and the kernel stages its PCM, else through the pointer.
template <int KIND, int LAY>
__host__ __forceinline__ bool wb_rsrc(const DecodeArgs& a) {
    return staged<KIND, LAY>() && a.wb_bytes != 0;
}

// One bucket kernel, either write-back form. Dynamic LDS above 64 KiB (four waves' rings and
// stages; the 32-bit-container units' larger rings) must be allowed per kernel.
template <int KIND, int LAY, int MB, bool MIX, bool WBR>
__host__ hipError_t launch_bucket_wb(const DecodeArgs& a, dim3 g, hipStream_t st) {
    if constexpr (DEC_LDS_BYTES > 64 * 1024) {
        static std::atomic<uint64_t> lds_set{0};
        if (const hipError_t e = set_lds_limit(lds_set, reinterpret_cast<const void*>(&k_decode<KIND, LAY, MB, MIX, WBR>),
                                               DEC_LDS_BYTES);
            e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL((k_decode<KIND, LAY, MB, MIX, WBR>), g, dim3(DEC_THREADS), DEC_LDS_BYTES, st, a);
    return hipSuccess;
}
template <int KIND, int LAY, int MB, bool MIX>
__host__ hipError_t launch_bucket(const DecodeArgs& a, dim3 g, hipStream_t st) {
    if constexpr (staged<KIND, LAY>()) {
        if (wb_rsrc<KIND, LAY>(a)) return launch_bucket_wb<KIND, LAY, MB, MIX, true>(a, g, st);
    }
    return launch_bucket_wb<KIND, LAY, MB, MIX, false>(a, g, st);
}

template <int KIND, int LAY>
hipError_t launch_decode_layout(const DecodeArgs& a, uint32_t max_frames, hipStream_t st) {
    if (a.rest_only) return hipSuccess;
    const dim3 g = decode_grid<KIND, LAY>(a, max_frames);
    hipError_t e = launch_bucket<KIND, LAY, 8, false>(a, g, st);
    if (e == hipSuccess && bucket_launched(a, 4, false)) e = launch_bucket<KIND, LAY, 4, false>(a, g, st);
    if (e == hipSuccess && bucket_launched(a, 12, false)) e = launch_bucket<KIND, LAY, 12, false>(a, g, st);
    if (e == hipSuccess && bucket_launched(a, 16, false)) e = launch_bucket<KIND, LAY, 16, false>(a, g, st);
    if (e == hipSuccess && bucket_launched(a, 32, false)) e = launch_bucket<KIND, LAY, 32, false>(a, g, st);
    return e != hipSuccess ? e : hipGetLastError();
}

// Waves with CONSTANT / VERBATIM lanes (bucket 8 or 32 + MIX_BIT), after the pure kernels.
// With rest_only: just the `rest` launch of the most general kernel (order 32, constant /
// verbatim lanes) on a small grid, for the groups of buckets without a launch of their own.
template <int KIND, int LAY>
hipError_t launch_decode_mix(const DecodeArgs& a, uint32_t max_frames, hipStream_t st) {
    const dim3 g = decode_grid<KIND, LAY>(a, max_frames);
    if (a.rest_only) {
        DecodeArgs r = a;
        r.rest = 1;
        const dim3 gr(g.x < SPARSE_DECODE_BLOCKS ? g.x : SPARSE_DECODE_BLOCKS);
        const hipError_t e = launch_bucket<KIND, LAY, 32, true>(r, gr, st);
        return e != hipSuccess ? e : hipGetLastError();
    }
    hipError_t e = hipSuccess;
    if (bucket_launched(a, 8, true)) e = launch_bucket<KIND, LAY, 8, true>(a, g, st);
    if (e == hipSuccess && bucket_launched(a, 32, true)) e = launch_bucket<KIND, LAY, 32, true>(a, g, st);
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace zflac
