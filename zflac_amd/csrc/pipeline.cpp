// pipeline.cpp -- the device pipeline of a batch: upload, class layout and buffers, the
// kernel argument builders, the launches of a run (submit_batch), its results
// (finish_batch) and batch creation.
//
// Reference: Senryoku/zflac src/zflac.zig (decode :217-310, decode_frames :312-602).
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <thread>
#include <unordered_map>

#include "batch.h"
#include "launch.h"

namespace zflac {
namespace {

// One per device: the windows' events are recorded on the streams of that device's batches.
Uploader& uploader(int device) {
    static std::mutex mu;
    static std::unordered_map<int, Uploader*> per_device;  // never destroyed: outlives every batch
    std::lock_guard<std::mutex> lock(mu);
    Uploader*& u = per_device[device];
    if (!u) u = new Uploader();
    return *u;
}

// bytes [a, b) of the layout into dst
void fill_window(uint8_t* dst, uint64_t a, uint64_t b, const std::vector<uint64_t>& in_off,
                 const std::vector<const uint8_t*>& srcs, const std::vector<uint64_t>& lens) {
    size_t m = std::upper_bound(in_off.begin(), in_off.end(), a) - in_off.begin();
    m = m ? m - 1 : 0;
    uint64_t p = a;
    for (; p < b && m < in_off.size(); m++) {
        const uint64_t s0 = in_off[m], s1 = in_off[m] + lens[m];
        if (s1 <= p) continue;
        if (s0 >= b) break;
        if (s0 > p) {
            std::memset(dst + (p - a), 0, s0 - p);
            p = s0;
        }
        const uint64_t e = std::min(s1, b);
        std::memcpy(dst + (p - a), srcs[m] + (p - s0), e - p);
        p = e;
    }
    if (p < b) std::memset(dst + (p - a), 0, b - p);
}

void upload_streams(int device, uint8_t* dev, uint64_t total, const std::vector<uint64_t>& in_off,
                    const std::vector<const uint8_t*>& srcs, const std::vector<uint64_t>& lens, hipStream_t st) {
    Uploader& U = uploader(device);
    std::lock_guard<std::mutex> lock(U.mu);
    for (int k = 0; k < 2; k++) {
        if (!U.pin[k]) ck(hipHostMalloc(reinterpret_cast<void**>(&U.pin[k]), Uploader::WIN, hipHostMallocDefault));
        if (!U.done[k]) ck(hipEventCreate(&U.done[k]));
    }
    int k = 0;
    for (uint64_t a = 0; a < total; a += Uploader::WIN, k ^= 1) {
        const uint64_t b = std::min(a + Uploader::WIN, total);
        if (U.used[k]) ck(hipEventSynchronize(U.done[k]));  // the DMA of this window's last use
        const uint64_t n = b - a;
        const int nt = n >= (8ull << 20) ? 4 : 1;
        std::vector<std::thread> ts;
        for (int t = 1; t < nt; t++)
            ts.emplace_back(fill_window, U.pin[k] + n * t / nt, a + n * t / nt, a + n * (t + 1) / nt,
                            std::cref(in_off), std::cref(srcs), std::cref(lens));
        fill_window(U.pin[k], a, a + n / nt, in_off, srcs, lens);
        for (auto& t : ts) t.join();
        ck(hipMemcpyAsync(dev + a, U.pin[k], n, hipMemcpyHostToDevice, st));
        ck(hipEventRecord(U.done[k], st));
        U.used[k] = true;
    }
    ck(hipStreamSynchronize(st));
}

// The k_decode buckets (history size MB, MIX for constant / verbatim subframes) that get a
// launch of their own: predicted from the first subframe of each member's first frame, whose
// type byte follows the frame header (src/zflac.zig:426-429). k_decode classifies every frame
// group itself (the order-8 launch); groups of a bucket without a launch are decoded by the
// `rest` launch (enqueue_rest), after which the bucket is added to the mask (finish_batch).
uint32_t plan_buckets(const zflac_batch* b, const Class& C, const zflac_stream* src) {
    uint32_t mask = bucket_bit(8, false);
    for (uint32_t i : C.members) {
        const StreamState& s = b->streams[i];
        const uint64_t p = s.frames_begin + s.first.hdr_len;
        if (s.first.crc_eof || p >= s.len) continue;
        const uint32_t t = (src[i].data[p] >> 1) & 63;
        const uint32_t ord = t >= 32 ? t - 31 : (t >= 8 && t <= 12 ? t - 8 : 0);
        if (t <= 1) mask |= bucket_bit(8, true) | bucket_bit(32, true);  // the wave's order is unknown
        else mask |= bucket_bit(ord <= 4 ? 4 : ord <= 8 ? 8 : ord <= 12 ? 12 : ord <= 16 ? 16 : 32, false);
    }
    return mask;
}

// Output room for a stream whose STREAMINFO total is 0 (unknown): zflac then reads frames until
// fewer than 4 bytes are left (src/zflac.zig:343-350) and grows its buffer as it goes. Once per
// batch (here, at creation) a k_scan over the class gives every stream's frame-sync candidates
// and the sample units their headers claim; the chain zflac walks is made of candidates, so
// their units bound its output. That is the stream's reservation, and the parallel pass then
// certifies its chain to the end of the stream (k_verify). A stream whose candidates claim more
// than UNKNOWN_MAX_PER_BYTE output elements per input byte (a flood of false syncs) gets no
// reservation and goes to the sequential planner. (Silence as constant subframes, the most
// compressible content, is ~800 elements per byte at 4,096-sample blocks.)
constexpr uint64_t UNKNOWN_MAX_PER_BYTE = 4096;

void prescan_unknown_totals(zflac_batch* b, Class& C, std::vector<uint64_t>& units, std::vector<uint64_t>& cands) {
    hipStream_t st = b->stream;
    ck(launch_scan(scan_args(C), st));
    std::vector<uint32_t> cnt(C.chunks.size());
    std::vector<unsigned long long> u(C.chunks.size());
    if (!C.chunks.empty()) {
        ck(hipMemcpyAsync(cnt.data(), C.chunk_cnt.p, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        ck(hipMemcpyAsync(u.data(), C.chunk_units.p, u.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
    ck(hipStreamSynchronize(st));
    units.assign(C.members.size(), 0);
    cands.assign(C.members.size(), 0);
    for (size_t k = 0; k < C.chunks.size(); k++) {
        units[C.chunks[k].stream] += u[k];
        cands[C.chunks[k].stream] += cnt[k];
    }
}

void plan_front(zflac_batch* b, Class& C);  // below

void alloc_class(zflac_batch* b, Class& C, const zflac_stream* src) {
    C.full_mask = plan_buckets(b, C, src);
    const int esz = esz_of_kind(C.kind);
    // input layout: each stream 16-byte aligned
    std::vector<uint64_t> in_off(C.members.size());
    uint64_t off = 0;
    for (size_t m = 0; m < C.members.size(); m++) {
        in_off[m] = off;
        off += (b->streams[C.members[m]].len + 15) & ~(uint64_t)15;
    }
    C.in_bytes = off;
    C.in.alloc(off + INPUT_PAD);
    uint64_t est_frames = 0, grid_frames = 0;
    C.desc.resize(C.members.size());
    C.chunks.clear();
    C.any_unknown = false;
    for (size_t m = 0; m < C.members.size(); m++) {
        StreamState& s = b->streams[C.members[m]];
        s.slot = (uint32_t)m;
        StreamDesc& D = C.desc[m];
        std::memset(&D, 0, sizeof(D));
        D.in_begin = in_off[m] + s.frames_begin;
        D.in_end = in_off[m] + s.len;
        D.valid_total = s.si.total > 0;
        D.total = D.valid_total ? s.si.total * (uint64_t)s.nch : 0;
        D.out_cap = D.total;  // (total unknown: from the pre-scan below)
        if (!D.valid_total) C.any_unknown = true;
        D.rate_hz = s.first.rate;
        D.si_rate = s.si.sample_rate;
        D.byte1 = (uint8_t)s.first.byte1;
        D.nch = (uint8_t)s.nch;
        D.dcode = (uint8_t)s.first.dcode;
        D.si_bps = (uint8_t)s.si.bps;
        D.justify = (b->flags & FLAG_NO_JUSTIFY) ? 0 : justify_of(s.si.bps);
        D.first_chunk = (uint32_t)C.chunks.size();
        const uint64_t abase0 = D.in_begin & ~(uint64_t)15;
        for (uint64_t a = abase0; a < D.in_end; a += CHUNK_BYTES) {
            ChunkDesc ch;
            ch.begin = std::max(a, D.in_begin);
            ch.end = std::min(a + CHUNK_BYTES, D.in_end);
            ch.stream = (uint32_t)m;
            ch.pad_ = 0;
            C.chunks.push_back(ch);
        }
        D.end_chunk = (uint32_t)C.chunks.size();
        const uint64_t minb = std::max<uint64_t>(16, s.si.min_block ? s.si.min_block : 16);
        // (at most one candidate per two bytes: a huge STREAMINFO total cannot inflate it)
        const uint64_t est = std::min<uint64_t>(s.si.total ? s.si.total / minb : s.len / 16, s.len / 2) + 2;
        if (D.valid_total) est_frames += est;  // (total unknown: the pre-scan's candidate count)
        // fixed blocking with a known total: zflac reads exactly ceil(total / block) frames (:341)
        const bool fixed = s.si.min_block == s.si.max_block && s.si.min_block >= 16;
        if (D.valid_total) grid_frames += fixed ? (s.si.total + s.si.min_block - 1) / s.si.min_block : est;
    }
    std::vector<const uint8_t*> srcs(C.members.size());
    std::vector<uint64_t> lens(C.members.size());
    for (size_t m = 0; m < C.members.size(); m++) {
        srcs[m] = src[C.members[m]].data;
        lens[m] = b->streams[C.members[m]].len;
    }
    upload_streams(b->device, C.in.p, C.in.n, in_off, srcs, lens, b->stream);  // inputs resident in HBM
    C.d_desc.alloc(C.desc.size());
    const size_t nc = std::max<size_t>(C.chunks.size(), 1);
    C.d_chunks.alloc(nc);
    if (!C.chunks.empty())
        ck(hipMemcpy(C.d_chunks.p, C.chunks.data(), C.chunks.size() * sizeof(ChunkDesc), hipMemcpyHostToDevice));
    C.chunk_cnt.alloc(nc);
    C.chunk_units.alloc(nc);
    C.chunk_slots.alloc(nc * CHUNK_CAP);
    C.chunk_slot_units.alloc(nc * CHUNK_CAP);
    C.chunk_off.alloc(nc + 1);
    C.chunk_uoff.alloc(nc + 1);
    C.misc.alloc(4 + C.members.size());
    // (misc[3], k_hop's hop_failed mark, is compared with the run's epoch and zeroed by no hop run)
    ck(hipMemset(C.misc.p, 0, (4 + C.members.size()) * sizeof(uint32_t)));
    C.status = C.misc.p + 4;
    C.dummy.alloc(DUMMY_BYTES + PROBE_BYTES);
    if (C.any_unknown) {  // reservations of the streams without a STREAMINFO total
        ck(hipMemcpy(C.d_desc.p, C.desc.data(), C.desc.size() * sizeof(StreamDesc), hipMemcpyHostToDevice));
        std::vector<uint64_t> units, cands;
        prescan_unknown_totals(b, C, units, cands);
        for (size_t m = 0; m < C.members.size(); m++) {
            StreamDesc& D = C.desc[m];
            if (D.valid_total) continue;
            const uint64_t avail = D.in_end - D.in_begin;
            D.out_cap = units[m] <= UNKNOWN_MAX_PER_BYTE * avail + (1u << 20) ? units[m] : 0;
            est_frames += cands[m] + 2;
            grid_frames += cands[m] + 2;
        }
    }
    // output layout: each stream's region starts on a 32-byte boundary, whatever the length of
    // the streams before it: the packed 16-byte stores of the fast path need 16-byte aligned
    // frames, and zflac's backing is 32-byte aligned (:331)
    const uint64_t align_elems = 32 / (uint64_t)esz;
    auto layout = [&]() {
        uint64_t o = 0;
        for (StreamDesc& D : C.desc) {
            o = (o + align_elems - 1) & ~(align_elems - 1);
            D.out_base = o;
            o += D.out_cap;
        }
        return o;
    };
    uint64_t out = layout();
    if (C.any_unknown) {
        // The reservations of unknown totals come from candidate headers, which planted false
        // syncs can inflate: together with the rest of the class they get at most half of the
        // device's free memory (the largest dropped first, to the planner), and none at all if
        // the allocation still fails.
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        while (out * esz > free_b / 2) {
            StreamDesc* big = nullptr;
            for (StreamDesc& D : C.desc)
                if (!D.valid_total && D.out_cap && (!big || D.out_cap > big->out_cap)) big = &D;
            if (!big) break;
            big->out_cap = 0;
            out = layout();
        }
    }
    try {
        C.out.alloc(out * esz + 32);
    } catch (const DeviceError&) {
        bool dropped = false;
        for (StreamDesc& D : C.desc)
            if (!D.valid_total && D.out_cap) {
                D.out_cap = 0;
                dropped = true;
            }
        if (!dropped) throw;
        (void)hipGetLastError();  // (the failed hipMalloc's error must not surface at a later check)
        out = layout();
        C.out.alloc(out * esz + 32);
    }
    C.out_elems = out;
    ck(hipMemcpy(C.d_desc.p, C.desc.data(), C.desc.size() * sizeof(StreamDesc), hipMemcpyHostToDevice));
    const size_t units_at = (4 + C.members.size() + 1) & ~(size_t)1;  // (u32 index, 8-byte aligned)
    const size_t pin_words = units_at + (C.any_unknown ? 2 * C.members.size() : 0);
    ck(hipHostMalloc(reinterpret_cast<void**>(&C.pin.p), pin_words * sizeof(uint32_t), hipHostMallocDefault));
    std::memset(C.pin.p, 0, pin_words * sizeof(uint32_t));
    C.h_misc = C.pin.p;
    C.h_status = C.pin.p + 4;
    if (C.any_unknown) {
        C.units.alloc(C.members.size());
        C.h_units = reinterpret_cast<uint64_t*>(C.pin.p + units_at);
    }
    C.cap = (uint32_t)std::min<uint64_t>(est_frames + C.chunks.size() * 2 + 1024, 0x7FFFFFFFull);
    C.est_frames = est_frames;
    C.grid_frames = (uint32_t)std::min<uint64_t>(grid_frames + grid_frames / 64 + 64, C.cap);
    plan_front(b, C);
}

// ZFLAC_FRONT=scan|hop|auto for batches created without ZFLAC_FLAG_FRONT_*; ZFLAC_HOP_MAX_FRAMES /
// ZFLAC_HOP_MIN_STREAMS replace the compiled limits (the sweeps they were measured with, tests).
FrontMode front_mode(int flags) {
    const int f = flags & (ZFLAC_FLAG_FRONT_SCAN | ZFLAC_FLAG_FRONT_HOP);
    if (f == ZFLAC_FLAG_FRONT_SCAN) return FRONT_FORCE_SCAN;
    if (f == ZFLAC_FLAG_FRONT_HOP) return FRONT_FORCE_HOP;
    if (f) return FRONT_AUTO;
    const char* e = std::getenv("ZFLAC_FRONT");
    return !e ? FRONT_AUTO : (e[0] == 's' ? FRONT_FORCE_SCAN : (e[0] == 'h' ? FRONT_FORCE_HOP : FRONT_AUTO));
}

void plan_front(zflac_batch* b, Class& C) {
    HopLimits lim;
    if (const char* e = std::getenv("ZFLAC_HOP_MAX_FRAMES")) lim.max_frames = (uint32_t)std::strtoul(e, nullptr, 10);
    if (const char* e = std::getenv("ZFLAC_HOP_MIN_STREAMS")) lim.min_streams = (uint32_t)std::strtoul(e, nullptr, 10);
    std::vector<const StreamPlan*> plans(C.members.size());
    for (size_t m = 0; m < C.members.size(); m++) plans[m] = &b->streams[C.members[m]];
    C.hop.resize(C.members.size());
    uint64_t total = 0;
    C.front = plan_hop(plans.data(), plans.size(), front_mode(b->flags), lim, C.hop.data(), &total);
    if (C.front == FRONT_HOP && total > C.cap) C.front = FRONT_SCAN;  // (cap >= the exact count: never)
    if (C.front != FRONT_HOP) {
        C.hop.clear();
        return;
    }
    C.hop_frames = (uint32_t)total;
    C.d_hop.alloc(C.hop.size());
    ck(hipMemcpy(C.d_hop.p, C.hop.data(), C.hop.size() * sizeof(HopDesc), hipMemcpyHostToDevice));
}

void alloc_candidates(Class& C) {
    C.c_pos.alloc(C.cap);
    C.c_out.alloc(C.cap);
    C.c_end.alloc(C.cap);
    C.c_stream.alloc(C.cap);
    C.c_info.alloc(C.cap);
    C.c_rate.alloc(C.cap);
    C.c_err.alloc(C.cap);
    C.sub.alloc((size_t)C.cap * MAX_CH);
    C.group_mb.alloc((size_t)C.cap / 4 + 2);  // one per k_decode frame group (>= 8 frames each)
}

}  // namespace

// The kernel arguments of a class's run, one builder per struct: a call site sets only what
// differs for its launch.
ScanArgs scan_args(Class& C) {
    ScanArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in = C.in.p;
    a.streams = C.d_desc.p;
    a.chunks = C.d_chunks.p;
    a.n_chunks = (uint32_t)C.chunks.size();
    a.chunk_cnt = C.chunk_cnt.p;
    a.chunk_units = C.chunk_units.p;
    a.chunk_slots = C.chunk_slots.p;
    a.chunk_slot_units = C.chunk_slot_units.p;
    a.status = C.status;
    a.n_status = (uint32_t)C.members.size();
    a.misc = C.misc.p;
    return a;
}

CompactArgs compact_args(Class& C) {
    CompactArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in = C.in.p;
    a.streams = C.d_desc.p;
    a.chunks = C.d_chunks.p;
    a.n_chunks = (uint32_t)C.chunks.size();
    a.chunk_cnt = C.chunk_cnt.p;
    a.chunk_slots = C.chunk_slots.p;
    a.chunk_slot_units = C.chunk_slot_units.p;
    a.chunk_off = C.chunk_off.p;
    a.chunk_uoff = C.chunk_uoff.p;
    a.cap = C.cap;
    a.c_pos = C.c_pos.p;
    a.c_stream = C.c_stream.p;
    a.c_out = C.c_out.p;
    a.overflow = C.misc.p + 1;
    return a;
}

HopArgs hop_args(Class& C) {
    HopArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in = C.in.p;
    a.streams = C.d_desc.p;
    a.hop = C.d_hop.p;
    a.n_streams = (uint32_t)C.members.size();
    a.total_frames = C.hop_frames;
    a.cap = C.cap;
    if (++C.hop_epoch == 0) C.hop_epoch = 1;
    a.epoch = C.hop_epoch;
    a.c_pos = C.c_pos.p;
    a.c_stream = C.c_stream.p;
    a.c_out = C.c_out.p;
    a.chunk_off = C.chunk_off.p;
    a.status = C.status;
    a.misc = C.misc.p;
    return a;
}

static VerifyArgs verify_args(Class& C) {
    VerifyArgs a;
    std::memset(&a, 0, sizeof(a));
    a.streams = C.d_desc.p;
    a.n_streams = (uint32_t)C.members.size();
    a.chunk_off = C.chunk_off.p;
    a.c_pos = C.c_pos.p;
    a.c_stream = C.c_stream.p;
    a.c_out = C.c_out.p;
    a.n_frames = C.misc.p;
    a.cap = C.cap;
    a.c_end = C.c_end.p;
    a.c_err = C.c_err.p;
    a.c_info = C.c_info.p;
    a.c_rate = C.c_rate.p;
    a.status = C.status;
    a.units = C.any_unknown ? C.units.p : nullptr;
    return a;
}

// (every candidate of the class's last run; C.crc_bad holds C.cap verdicts)
static Crc16Args crc16_args(Class& C) {
    Crc16Args a;
    std::memset(&a, 0, sizeof(a));
    a.in = C.in.p;
    a.in_size = C.in.n;
    a.pos = C.c_pos.p;
    a.end = C.c_end.p;
    a.err = C.c_err.p;
    a.streams = C.d_desc.p;
    a.c_stream = C.c_stream.p;
    a.c_out = C.c_out.p;
    a.n_frames = C.misc.p;
    a.cap = C.cap;
    a.bad = C.crc_bad.p;
    return a;
}

DecodeArgs decode_args(Class& C) {
    DecodeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in = C.in.p;
    a.in_size = C.in.n;
    a.out = C.out.p;
    a.streams = C.d_desc.p;
    a.c_pos = C.c_pos.p;
    a.c_stream = C.c_stream.p;
    a.c_out = C.c_out.p;
    a.n_frames = C.misc.p;
    a.cap = C.cap;
    a.c_end = C.c_end.p;
    a.c_err = C.c_err.p;
    a.c_info = C.c_info.p;
    a.c_rate = C.c_rate.p;
    a.nch = C.nch;
    a.write = 1;
    a.dummy = C.dummy.p;
    a.sub_start = C.sub.p;
    a.group_mb = C.group_mb.p;
    // the staged write-back's form, per launch: the buffer resource wherever it can cover the
    // class's whole output (ZFLAC_STAGE_WB=ptr keeps the pointer form: tests, timing experiments)
    const char* e = std::getenv("ZFLAC_STAGE_WB");
    const bool wb_ptr = e && e[0] == 'p';
    a.wb_bytes = !wb_ptr && C.out.n <= WB_RSRC_MAX && (reinterpret_cast<uintptr_t>(C.out.p) & 15) == 0
                     ? (uint32_t)C.out.n
                     : 0u;
    return a;
}

// Which subframe-start walk a launch over `frames` frames of `nch` channels uses: k_walk
// (lane per frame: 64 serial chains per wave, nch - 1 subframes each) needs tens of thousands
// of subframe walks to fill the chip; k_walk_wave (wave per frame, wave-wide bit scan of each
// Rice partition) fills it with a few thousand, at several times the instructions per code.
// So the wave walk below WAVE_WALK_MAX_FRAMES subframe walks, the lane walk above, for every
// channel count (a 32,768-frame 6-channel stream: lane walk).
// ZFLAC_WALK=lane / wave forces one (timing experiments).
static bool use_wave_walk(uint64_t frames, int nch, int flags) {
    static const int forced = [] {
        const char* e = std::getenv("ZFLAC_WALK");
        return !e ? 0 : (e[0] == 'w' ? 1 : (e[0] == 'l' ? 2 : 0));
    }();
    if (flags & ZFLAC_FLAG_WALK_WAVE) return true;
    if (flags & ZFLAC_FLAG_WALK_LANE) return false;
    if (forced) return forced == 1;
    return frames * (uint64_t)(nch - 1) < WAVE_WALK_MAX_FRAMES;
}

// [container kind][layout: 0 = 3..8 channels, 1 = mono, 2 = stereo]
static constexpr DecodeLaunch* launch_decode_fn[3][3] = {
    {launch_decode_k0_multi, launch_decode_k0_mono, launch_decode_k0_stereo},
    {launch_decode_k1_multi, launch_decode_k1_mono, launch_decode_k1_stereo},
    {launch_decode_k2_multi, launch_decode_k2_mono, launch_decode_k2_stereo},
};
static constexpr DecodeLaunch* launch_walk_fn[3] = {launch_walk_k0, launch_walk_k1, launch_walk_k2};

// (documented in batch.h)
hipError_t launch_decode(int kind, const DecodeArgs& a, uint32_t max_frames, hipStream_t st, hipEvent_t mid,
                         hipStream_t front, hipEvent_t join, uint64_t est_frames, int flags) {
    const int lay = a.nch == 2 ? 2 : (a.nch == 1 ? 1 : 0);
    hipStream_t ws = front ? front : st;
    if (a.nch > 1 && !a.rest_only) {
        const hipError_t e = use_wave_walk(est_frames ? est_frames : max_frames, a.nch, flags)
                                 ? launch_walk_wave(kind, a, max_frames, ws)
                                 : launch_walk_fn[kind](a, max_frames, ws);
        if (e != hipSuccess) return e;
    }
    if (mid) {
        const hipError_t e = hipEventRecord(mid, ws);
        if (e != hipSuccess) return e;
    }
    if (front) {
        hipError_t e = hipEventRecord(join, front);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, join, 0);
        if (e != hipSuccess) return e;
    }
    return launch_decode_fn[kind][lay](a, max_frames, st);
}

// Launch the whole parallel pipeline of one class on the batch stream.
void enqueue_class(zflac_batch* b, Class& C, bool timing_first, bool timing_last) {
    hipStream_t st = b->front ? b->front : b->rs;  // scan, compact (and the walk) there
    const uint32_t nch = (uint32_t)C.chunks.size();
    if (nch == 0)  // (k_scan zeroes them otherwise)
        ck(hipMemsetAsync(C.misc.p, 0, (4 + C.members.size()) * sizeof(uint32_t), st));
    if (timing_first) ck(hipEventRecord(b->ev[0], st));
    C.front_run = C.front;
    if (C.front == FRONT_HOP) {  // the frame table by hopping from header to header: one launch
        ck(launch_hop(hop_args(C), st));
    } else {
        ck(launch_scan(scan_args(C), st));
        if (nch) ck(launch_scan_chunks(C.chunk_cnt.p, C.chunk_units.p, nch, C.chunk_off.p, C.chunk_uoff.p, C.misc.p, st));
        ck(launch_compact(compact_args(C), st));
    }
    if (timing_last) ck(hipEventRecord(b->ev[1], st));
    DecodeArgs da = decode_args(C);
    da.bucket_used = C.misc.p + 2;
    da.full_mask = C.full_mask;
    ck(launch_decode(C.kind, da, std::min(C.grid_frames, C.cap), b->rs, timing_last ? b->ev[4] : nullptr,
                     b->front, b->front_join, C.est_frames, b->flags));
    st = b->rs;  // decode, verify and the read-backs
    if (timing_last) ck(hipEventRecord(b->ev[2], st));
    ck(launch_verify(verify_args(C), C.cap, st));
    if (timing_last) ck(hipEventRecord(b->ev[3], st));
    // the counters and the status words in one read-back (contiguous on both sides)
    ck(hipMemcpyAsync(C.h_misc, C.misc.p, (4 + C.members.size()) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (C.any_unknown)
        ck(hipMemcpyAsync(C.h_units, C.units.p, C.members.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
}

// After a run whose order-8 launch found frame groups of a bucket the host did not
// predict (bucket_used outside full_mask): the rest launch decodes them, then the chain
// check and the read-backs run again (synchronous; a correct prediction never gets here).
static void enqueue_rest(zflac_batch* b, Class& C) {
    hipStream_t st = b->stream;
    DecodeArgs da = decode_args(C);
    da.full_mask = C.full_mask;
    da.rest_only = 1;
    ck(launch_decode(C.kind, da, std::min(C.grid_frames, C.cap), st));
    ck(hipMemsetAsync(C.status, 0, C.members.size() * sizeof(uint32_t), st));
    ck(launch_verify(verify_args(C), C.cap, st));
    ck(hipMemcpyAsync(C.h_status, C.status, C.members.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (C.any_unknown)
        ck(hipMemcpyAsync(C.h_units, C.units.p, C.members.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    ck(hipStreamSynchronize(st));
}

// Phase 1 of a run: every class's parallel pipeline on the next of the device's run streams,
// no host wait. Batches submitted back to back overlap on the device (each has its own
// buffers, consecutive runs different streams): the scan and walk of one run beside the
// decode of the other.
void submit_batch(zflac_batch* b) {
    ck(hipSetDevice(b->device));
    const bool timing = (b->flags & ZFLAC_FLAG_TIMING) != 0;
    // (no wait on the batch's own stream: everything create and finish enqueue there is
    // synchronized before they return. A marker recorded there would sit in a hardware queue
    // it may share with a run or md5 hub stream, behind a hash of several milliseconds.)
    b->rs = next_run_stream(b->device);
    if (b->exp_pending) {  // an export on a caller's stream still reads the samples this run overwrites
        ck(hipStreamWaitEvent(b->rs, b->ev_exp, 0));
        if (b->front) ck(hipStreamWaitEvent(b->front, b->ev_exp, 0));
        b->exp_pending = false;  // from here on the run's own events cover it
    }
    for (size_t ci = 0; ci < b->classes.size(); ci++) {
        Class& C = *b->classes[ci];
        C.redone = false;
        alloc_candidates(C);
        enqueue_class(b, C, timing && ci == 0, timing && ci + 1 == b->classes.size());
    }
    b->md5_hub = !b->pipe_who.empty() && !std::getenv("ZFLAC_MD5_NOHUB");
    if (!b->pipe_who.empty() && !b->md5_hub) {  // STREAMINFO MD5 of the streams this run certifies
        const uint32_t n = (uint32_t)b->pipe_who.size();
        if (timing) ck(hipEventRecord(b->ev[8], b->rs));
        ck(launch_md5(b->pipe_jobs.p, n, b->pipe_dig.p, b->rs, b->pipe_coop, &b->md5_pipe_kernel));
        if (timing) ck(hipEventRecord(b->ev[9], b->rs));
        ck(hipMemcpyAsync(b->pipe_pin, b->pipe_dig.p, (size_t)n * 16, hipMemcpyDeviceToHost, b->rs));
    }
    ck(hipEventRecord(b->ev_done, b->rs));  // zflac_hip_batch_ready
    if (b->md5_hub) {  // the hash of the streams this run certifies, in the device's md5 hub
        Md5Hub& h = md5_hub(b->device);
        std::lock_guard<std::mutex> lock(h.mu);
        b->md5_failed = false;  // (a failure of an earlier run of this batch is that run's)
        b->md5_pending = true;
        h.pend.push_back(b);
        if (h.pend.size() >= std::min<uint32_t>(h.runs, MD5_MAX_SEGS)) hub_flush(h);
    }
}

// Phase 2: wait for the pipeline, redo a class whose candidate table overflowed (grown,
// synchronously; not part of the recorded kernel timings), then the per-stream results,
// the sequential planner for streams the chain check did not certify, CRC-16 and MD5.
void finish_batch(zflac_batch* b) {
    ck(hipSetDevice(b->device));
    const bool timing = (b->flags & ZFLAC_FLAG_TIMING) != 0;
    ck(hipEventSynchronize(b->ev_done));  // the run, on its run stream
    b->rs = b->stream;  // from here on (regrowth, rest launch, planner): the batch's own stream
    if (b->md5_hub) {  // the run's hash (and its digests' read-back) in the md5 hub
        hub_release(b);
        if (b->md5_failed) {
            b->md5_failed = false;
            throw DeviceError{};  // the md5 hub launch holding this run failed
        }
        ck(hipEventSynchronize(b->ev_md5));
    }
    uint32_t rest_launches = 0, sequential = 0, used = 0, planned = 0;
    b->front_planned = b->front_used = 0;
    for (size_t ci = 0; ci < b->classes.size(); ci++) {
        Class& C = *b->classes[ci];
        planned |= C.full_mask;  // (only this function changes it, below)
        b->front_planned |= C.front_run;
        C.front_used = C.front_run;
        if (C.front_run == FRONT_HOP && C.h_misc[3] == C.hop_epoch) {
            // the hop lost a stream (numbers out of sequence, a size jump beyond its probes):
            // the class once more with the scan front, synchronously, and from now on
            C.front = C.front_used = FRONT_SCAN;
            C.redone = true;
            enqueue_class(b, C, false, false);
            ck(hipStreamSynchronize(b->stream));
        }
        b->front_used |= C.front_used;
        for (int attempt = 0; attempt < 3; attempt++) {
            if (!C.h_misc[1] && C.h_misc[0] <= C.cap) break;
            C.cap = std::max<uint32_t>(C.h_misc[0] + 1024, C.cap * 2);  // candidate table overflow: grow, redo
            C.grid_frames = std::max(C.grid_frames, C.h_misc[0]);
            alloc_candidates(C);
            C.redone = true;
            enqueue_class(b, C, false, false);
            ck(hipStreamSynchronize(b->stream));
        }
        // more candidates than the grids were sized for (false syncs): correct (the kernels
        // stride over them), but slower; size the next run's grids for them
        if (C.h_misc[0] > C.grid_frames) C.grid_frames = std::min(C.cap, C.h_misc[0] + C.h_misc[0] / 64 + 64);
        used |= C.h_misc[2] & BUCKET_MASK_ALL;
        if (C.full_mask && (C.h_misc[2] & ~C.full_mask)) {  // a bucket without a launch was used
            enqueue_rest(b, C);
            C.redone = true;
            rest_launches++;
            // from now on that bucket gets a launch of its own: later runs keep the pipelined
            // MD5 and skip the synchronous rest launch (launches are only ever added)
            C.full_mask |= C.h_misc[2] & BUCKET_MASK_ALL;
        }
    }
    const bool crc = (b->flags & ZFLAC_FLAG_CHECK_CRC16) != 0;
    b->timings.crc16_ms = 0;
    if (crc && !b->classes.empty()) {  // every candidate's trailer, after the chain checks
        if (timing) ck(hipEventRecord(b->ev[5], b->stream));
        for (auto& cp : b->classes) {
            Class& C = *cp;
            C.crc_bad.alloc(C.cap);
            ck(launch_crc16(crc16_args(C), std::min(C.h_misc[0], C.cap), b->stream));
        }
        if (timing) ck(hipEventRecord(b->ev[6], b->stream));
        ck(hipStreamSynchronize(b->stream));
        if (timing) {
            float tc = 0;
            ck(hipEventElapsedTime(&tc, b->ev[5], b->ev[6]));
            b->timings.crc16_ms = tc;
        }
    }
    if (timing && !b->classes.empty()) {
        float t01 = 0, t14 = 0, t42 = 0, t23 = 0, t03 = 0;
        ck(hipEventElapsedTime(&t01, b->ev[0], b->ev[1]));
        ck(hipEventElapsedTime(&t14, b->ev[1], b->ev[4]));
        ck(hipEventElapsedTime(&t42, b->ev[4], b->ev[2]));
        ck(hipEventElapsedTime(&t23, b->ev[2], b->ev[3]));
        ck(hipEventElapsedTime(&t03, b->ev[0], b->ev[3]));
        b->timings.scan_ms = t01;
        b->timings.walk_ms = t14;
        b->timings.decode_ms = t42;
        b->timings.verify_ms = t23;
        b->timings.total_ms = t03;
        b->have_timing = true;
    }
    // results
    uint64_t frames = 0, in_bytes = 0, out_bytes = 0, samples = 0;
    for (auto& cp : b->classes) {
        Class& C = *cp;
        const int esz = esz_of_kind(C.kind);
        std::vector<uint32_t> h_off, h_crc;
        const uint32_t nfr = std::min(C.h_misc[0], C.cap);
        if (crc && nfr) {
            h_crc.resize(nfr);
            ck(hipMemcpy(h_crc.data(), C.crc_bad.p, nfr * 4, hipMemcpyDeviceToHost));
        }
        for (size_t m = 0; m < C.members.size(); m++) {
            StreamState& s = b->streams[C.members[m]];
            s.override_out.reset();
            s.info = zflac_info{};
            s.info.sample_kind = (uint8_t)C.kind;
            if (C.h_status[m] == 0 && !(b->flags & ZFLAC_FLAG_FORCE_SLOW)) {
                const StreamDesc& D = C.desc[m];
                s.err = 0;
                s.dev_samples = C.out.p + D.out_base * esz;
                s.info.n_samples = D.valid_total ? D.total : C.h_units[m];
                s.info.channels = (uint8_t)s.nch;
                s.info.sample_rate = s.first.rate;
                s.info.bits_per_sample = (uint8_t)depth_bits(s.first.dcode, (int)s.si.bps);
                if (crc) {  // a certified stream's candidates up to its total are exactly its frames
                            // (k_crc16 passes the ones past the total: zflac never reads them)
                    if (h_off.empty()) {
                        h_off.resize(C.chunks.size() + 1);
                        ck(hipMemcpy(h_off.data(), C.chunk_off.p, h_off.size() * 4, hipMemcpyDeviceToHost));
                    }
                    const uint32_t f0 = std::min(h_off[D.first_chunk], nfr), f1 = std::min(h_off[D.end_chunk], nfr);
                    for (uint32_t f = f0; f < f1; f++)
                        if (h_crc[f]) {
                            s.err = E_FRAME_CRC;
                            s.info = zflac_info{};
                            s.info.sample_kind = (uint8_t)C.kind;
                            break;
                        }
                }
            } else {
                if (h_off.empty()) {
                    h_off.resize(C.chunks.size() + 1);
                    ck(hipMemcpy(h_off.data(), C.chunk_off.p, h_off.size() * 4, hipMemcpyDeviceToHost));
                }
                finish_stream_sequential(b, C, (uint32_t)m, h_off, std::min(C.h_misc[0], C.cap));
                sequential++;
            }
            s.info.samples_bytes = s.info.n_samples * esz;
            if (!s.err) {
                in_bytes += s.len - s.frames_begin;
                out_bytes += s.info.samples_bytes;
                samples += s.info.n_samples;
            }
        }
        frames += std::min(C.h_misc[0], C.cap);
    }
    b->timings.md5_ms = 0;
    if (b->flags & ZFLAC_FLAG_DEVICE_MD5) finish_md5(b, timing && !b->classes.empty());
    else
        for (auto& s : b->streams) s.md5_dev = 0, s.md5_src = ZFLAC_MD5_SRC_NONE;
    b->timings.frames = frames;
    b->timings.input_bytes = in_bytes;
    b->timings.output_bytes = out_bytes;
    b->timings.samples = samples;
    b->timings.rest_launches = rest_launches;
    b->timings.sequential_streams = sequential;
    b->buckets_used = used;
    b->buckets_planned = planned;
}

int create_batch(const zflac_stream* streams, size_t n, int device, int flags, zflac_batch** out) {
    if (!out || (n && !streams)) return E_INVALID_ARGUMENT;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return E_DEVICE;
    std::unique_ptr<zflac_batch> b(new (std::nothrow) zflac_batch());
    if (!b) return E_OUT_OF_MEMORY;
    b->device = device;
    b->flags = flags;
    const int rc = guarded([&]() -> int {
        ck(hipSetDevice(device));
        (void)device_streams(device);  // the run and md5 hub streams first (their own hardware queues)
        ck(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        b->rs = b->stream;
        if (const char* fp = std::getenv("ZFLAC_FRONT_PRIORITY"); fp && fp[0] == '1') {
            int least = 0, greatest = 0;
            ck(hipDeviceGetStreamPriorityRange(&least, &greatest));
            ck(hipStreamCreateWithPriority(&b->front, hipStreamNonBlocking, greatest));
            ck(hipEventCreateWithFlags(&b->front_join, hipEventDisableTiming));
        }
        // timing-only events: no system-scope fence (cache writeback + invalidate) at each
        // record, which would otherwise slow the kernel after it
        for (auto& e : b->ev) ck(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
        ck(hipEventCreateWithFlags(&b->ev_done, hipEventDisableTiming));
        ck(hipEventCreateWithFlags(&b->ev_md5, hipEventDisableTiming));
        const double t0 = now_ms();
        b->streams.resize(n);
        for (size_t i = 0; i < n; i++) {
            if (!streams[i].data && streams[i].len) return E_INVALID_ARGUMENT;
            plan_stream(b->streams[i], streams[i].data, streams[i].len);
        }
        const double t1 = now_ms();
        b->timings.plan_ms = t1 - t0;
        for (size_t i = 0; i < n; i++) {
            StreamState& s = b->streams[i];
            if (s.host_err || s.no_frames) continue;
            int ci = -1;
            for (size_t k = 0; k < b->classes.size(); k++)
                if (b->classes[k]->kind == s.kind && b->classes[k]->nch == s.nch) ci = (int)k;
            if (ci < 0) {
                b->classes.emplace_back(new Class());
                b->classes.back()->kind = s.kind;
                b->classes.back()->nch = s.nch;
                ci = (int)b->classes.size() - 1;
            }
            s.cls = ci;
            b->classes[ci]->members.push_back((uint32_t)i);
        }
        for (auto& C : b->classes) alloc_class(b.get(), *C, streams);
        if (flags & ZFLAC_FLAG_DEVICE_MD5) plan_md5_pipeline(b.get());
        b->timings.upload_ms = now_ms() - t1;
        // streams resolved on the host
        for (auto& s : b->streams) {
            if (s.host_err) s.err = s.host_err;
            if (s.no_frames) {
                s.err = 0;
                s.info = zflac_info{};
                s.info.sample_kind = (uint8_t)s.kind;
            }
        }
        return E_OK;
    });
    if (rc) return rc;
    *out = b.release();
    return E_OK;
}

}  // namespace zflac
