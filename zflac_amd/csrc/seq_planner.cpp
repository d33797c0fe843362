// seq_planner.cpp -- sequential chain planner (src/zflac.zig:340-581 state machine) for
// streams the fast path could not certify. Frame records come from the fast pass when the
// chain position is a sync candidate, otherwise from a one-frame device probe.
#include <cstring>
#include <unordered_map>

#include "batch.h"
#include "launch.h"

namespace zflac {
namespace {

struct FrameRec {
    uint64_t end;
    int32_t err;
    uint32_t info;
    uint32_t rate;
};

struct SeqRunner {
    zflac_batch* b;
    Class& C;
    uint32_t slot;
    DevBuf<uint64_t> p_pos, p_out, p_end;
    DevBuf<uint32_t> p_stream, p_info, p_rate;
    DevBuf<int32_t> p_err;
    DevBuf<uint32_t> p_sub, p_mb, p_crc, p_cnt;
    DevBuf<uint64_t> p_sync;
    DevBuf<StreamDesc> p_desc;

    SeqRunner(zflac_batch* b_, Class& C_, uint32_t slot_) : b(b_), C(C_), slot(slot_) {}

    // decode the explicit frame list `pos` (absolute input offsets) with output offsets
    // `outoff` relative to `desc.out_base`; returns records
    void run_list(const std::vector<uint64_t>& pos, const std::vector<uint64_t>& outoff, const StreamDesc& desc,
                  void* out, int write, std::vector<FrameRec>& recs) {
        const size_t n = pos.size();
        p_pos.alloc(n);
        p_out.alloc(n);
        p_end.alloc(n);
        p_stream.alloc(n);
        p_info.alloc(n);
        p_rate.alloc(n);
        p_err.alloc(n);
        p_desc.alloc(1);
        std::vector<uint32_t> zeros(n, 0);
        hipStream_t st = b->stream;
        ck(hipMemcpyAsync(p_pos.p, pos.data(), n * 8, hipMemcpyHostToDevice, st));
        ck(hipMemcpyAsync(p_out.p, outoff.data(), n * 8, hipMemcpyHostToDevice, st));
        ck(hipMemcpyAsync(p_stream.p, zeros.data(), n * 4, hipMemcpyHostToDevice, st));
        ck(hipMemcpyAsync(p_desc.p, &desc, sizeof(desc), hipMemcpyHostToDevice, st));
        DecodeArgs a;
        std::memset(&a, 0, sizeof(a));
        a.in = C.in.p;
        a.in_size = C.in.n;
        a.out = out;
        a.streams = p_desc.p;
        a.c_pos = p_pos.p;
        a.c_stream = p_stream.p;
        a.c_out = p_out.p;
        a.n_frames = nullptr;
        a.n_frames_host = (uint32_t)n;
        a.cap = (uint32_t)n;
        a.c_end = p_end.p;
        a.c_err = p_err.p;
        a.c_info = p_info.p;
        a.c_rate = p_rate.p;
        a.nch = C.nch;
        a.write = write;
        a.dummy = C.dummy.p;
        p_sub.alloc(n * MAX_CH);
        a.sub_start = p_sub.p;
        p_mb.alloc(n / 4 + 2);
        a.group_mb = p_mb.p;
        ck(launch_decode(C.kind, a, (uint32_t)n, st, nullptr, nullptr, nullptr, 0, b->flags));
        std::vector<uint64_t> e(n);
        std::vector<int32_t> er(n);
        std::vector<uint32_t> in(n), ra(n);
        ck(hipMemcpyAsync(e.data(), p_end.p, n * 8, hipMemcpyDeviceToHost, st));
        ck(hipMemcpyAsync(er.data(), p_err.p, n * 4, hipMemcpyDeviceToHost, st));
        ck(hipMemcpyAsync(in.data(), p_info.p, n * 4, hipMemcpyDeviceToHost, st));
        ck(hipMemcpyAsync(ra.data(), p_rate.p, n * 4, hipMemcpyDeviceToHost, st));
        ck(hipStreamSynchronize(st));
        recs.resize(n);
        for (size_t i = 0; i < n; i++) recs[i] = FrameRec{e[i], er[i], in[i], ra[i]};
    }

    // Sync codes in [lo, hi) whose header matches the stream (k_sync_list), sorted.
    std::vector<uint64_t> sync_list(uint64_t lo, uint64_t hi, const StreamDesc& D) {
        hipStream_t st = b->stream;
        uint32_t cap = 4096, n = 0;
        for (int attempt = 0; attempt < 2; attempt++) {
            p_sync.alloc(cap);
            p_cnt.alloc(1);
            ck(hipMemsetAsync(p_cnt.p, 0, 4, st));
            SyncListArgs a;
            a.in = C.in.p;
            a.lo = lo;
            a.hi = hi;
            a.in_end = D.in_end;
            a.si_rate = D.si_rate;
            a.rate_hz = D.rate_hz;
            a.nch = D.nch;
            a.dcode = D.dcode;
            a.pos = p_sync.p;
            a.count = p_cnt.p;
            a.cap = cap;
            ck(launch_sync_list(a, st));
            ck(hipMemcpyAsync(&n, p_cnt.p, 4, hipMemcpyDeviceToHost, st));
            ck(hipStreamSynchronize(st));
            if (n <= cap) break;
            cap = n;  // more than fit: once more with room for all
        }
        std::vector<uint64_t> out(std::min(n, cap));
        if (!out.empty()) {
            ck(hipMemcpyAsync(out.data(), p_sync.p, out.size() * 8, hipMemcpyDeviceToHost, st));
            ck(hipStreamSynchronize(st));
        }
        std::sort(out.begin(), out.end());
        return out;
    }

    // k_crc16 over the frames [pos[i], end[i]); true when every trailer matches
    bool crc16_ok(const std::vector<uint64_t>& pos, const std::vector<uint64_t>& end) {
        const size_t n = pos.size();
        if (!n) return true;
        hipStream_t st = b->stream;
        p_pos.alloc(n);
        p_end.alloc(n);
        p_crc.alloc(n);
        ck(hipMemcpyAsync(p_pos.p, pos.data(), n * 8, hipMemcpyHostToDevice, st));
        ck(hipMemcpyAsync(p_end.p, end.data(), n * 8, hipMemcpyHostToDevice, st));
        Crc16Args a;
        std::memset(&a, 0, sizeof(a));
        a.in = C.in.p;
        a.in_size = C.in.n;
        a.pos = p_pos.p;
        a.end = p_end.p;
        a.n_frames_host = (uint32_t)n;
        a.cap = (uint32_t)n;
        a.bad = p_crc.p;
        ck(launch_crc16(a, (uint32_t)n, st));
        std::vector<uint32_t> bad(n);
        ck(hipMemcpyAsync(bad.data(), p_crc.p, n * 4, hipMemcpyDeviceToHost, st));
        ck(hipStreamSynchronize(st));
        return std::none_of(bad.begin(), bad.end(), [](uint32_t x) { return x != 0; });
    }
};

}  // namespace

void finish_stream_sequential(zflac_batch* b, Class& C, uint32_t slot, const std::vector<uint32_t>& h_chunk_off,
                              uint32_t nframes) {
    StreamState& s = b->streams[C.members[slot]];
    const StreamDesc D = C.desc[slot];
    hipStream_t st = b->stream;
    // fast-pass records of this stream's candidates
    std::unordered_map<uint64_t, FrameRec> recs;
    const uint32_t f0 = std::min(h_chunk_off[D.first_chunk], nframes);
    const uint32_t f1 = std::min(h_chunk_off[D.end_chunk], nframes);
    if (f1 > f0 && !(b->flags & ZFLAC_FLAG_FORCE_SLOW)) {
        const size_t n = f1 - f0;
        std::vector<uint64_t> pos(n), end(n);
        std::vector<int32_t> err(n);
        std::vector<uint32_t> info(n), rate(n);
        ck(hipMemcpyAsync(pos.data(), C.c_pos.p + f0, n * 8, hipMemcpyDeviceToHost, st));
        ck(hipMemcpyAsync(end.data(), C.c_end.p + f0, n * 8, hipMemcpyDeviceToHost, st));
        ck(hipMemcpyAsync(err.data(), C.c_err.p + f0, n * 4, hipMemcpyDeviceToHost, st));
        ck(hipMemcpyAsync(info.data(), C.c_info.p + f0, n * 4, hipMemcpyDeviceToHost, st));
        ck(hipMemcpyAsync(rate.data(), C.c_rate.p + f0, n * 4, hipMemcpyDeviceToHost, st));
        ck(hipStreamSynchronize(st));
        for (size_t i = 0; i < n; i++) recs[pos[i]] = FrameRec{end[i], err[i], info[i], rate[i]};
    }
    SeqRunner R(b, C, slot);
    StreamDesc probe_desc = D;
    probe_desc.out_base = 0;
    probe_desc.out_cap = 0;
    probe_desc.valid_total = 0;
    probe_desc.total = 0;

    // state machine of decode_frames (src/zflac.zig:321-581)
    bool valid_total = s.si.total > 0;
    const uint64_t expC = s.si.channels;
    const uint64_t total = expC * (valid_total ? s.si.total : 4096);
    uint64_t buf_len = total;
    uint64_t offset = 0;
    uint64_t p = D.in_begin;
    bool first = true;
    uint32_t rate0 = 0, count0 = 0, dcode0 = 0;
    int bps0 = 0;
    std::vector<uint64_t> list_pos, list_out, list_end;
    int err = 0;
    // batched probes: a chain position without a record asks for every matching sync code
    // in a window ahead of it (doubling, 1 .. 64 MiB) and decodes them in one launch
    uint64_t probe_win = 1ull << 20;
    for (;;) {
        if (valid_total && offset >= total) break;  // :341
        if (D.in_end - p < 4) {                     // :343-350
            if (valid_total) err = E_END_OF_STREAM;
            break;
        }
        FrameRec rec;
        auto it = recs.find(p);
        if (it != recs.end()) {
            rec = it->second;
        } else {
            const uint64_t hi = std::min<uint64_t>(D.in_end, p + probe_win);
            probe_win = std::min<uint64_t>(probe_win * 2, 64ull << 20);
            std::vector<uint64_t> pos = R.sync_list(p, hi, D);
            if (pos.empty() || pos[0] != p) pos.insert(pos.begin(), p);  // zflac reads p whatever it holds
            std::vector<FrameRec> got;
            R.run_list(pos, std::vector<uint64_t>(pos.size(), 0), probe_desc, C.out.p, 0, got);
            for (size_t i = 0; i < pos.size(); i++) recs[pos[i]] = got[i];
            rec = recs[p];
        }
        if (rec.info & INFO_PRE_ERR) { err = rec.err; break; }
        const uint32_t bs = (rec.info & 0xFFFF) + 1, code = (rec.info >> 16) & 15, dcode = (rec.info >> 20) & 7;
        if (first) {  // :376-388
            rate0 = rec.rate;
            count0 = (uint32_t)channels_count(code);
            dcode0 = dcode;
            bps0 = depth_bits(dcode, (int)s.si.bps);
            if (bps0 < 0) { err = E_OUT_OF_DOMAIN; break; }
            if (count0 != expC) { err = E_INCONSISTENT_PARAMETERS; break; }
            first = false;
        } else if (rate0 != rec.rate || count0 != (uint32_t)channels_count(code) || dcode0 != dcode) {
            err = E_INCONSISTENT_PARAMETERS;  // :391
            break;
        }
        const uint64_t expected = offset + (uint64_t)bs * count0;  // :394-402
        if (buf_len < expected) {
            buf_len = std::max(2 * buf_len, expected);
            valid_total = false;
        }
        if (bs == 1 && valid_total && offset + count0 < total) { err = E_INVALID_FRAME_HEADER; break; }  // :405
        if (rec.info & INFO_CRC_EOF) { err = E_END_OF_STREAM; break; }
        if (rec.err) { err = rec.err; break; }
        list_pos.push_back(p);
        list_out.push_back(offset);
        list_end.push_back(rec.end);
        offset += (uint64_t)bs * count0;
        p = rec.end;
    }
    // optional CRC-16 of the frames read before the loop stopped: zflac would read each
    // trailer before the next frame, so a mismatch there comes before `err`
    if ((b->flags & ZFLAC_FLAG_CHECK_CRC16) && !R.crc16_ok(list_pos, list_end)) err = E_FRAME_CRC;
    s.err = err;
    if (err) return;
    // final decode of the certified chain into this stream's region (or an override)
    const int esz = esz_of_kind(C.kind);
    StreamDesc wd = D;
    wd.out_base = 0;
    wd.out_cap = offset;
    wd.valid_total = 0;
    wd.total = 0;
    uint8_t* dst;
    if (offset <= D.out_cap) {
        dst = C.out.p + D.out_base * esz;
    } else {
        s.override_out.reset(new DevBuf<uint8_t>());
        s.override_out->alloc(offset * esz + 16);
        dst = s.override_out->p;
    }
    if (!list_pos.empty()) {
        std::vector<FrameRec> out_recs;
        R.run_list(list_pos, list_out, wd, dst, 1, out_recs);
        for (auto& r : out_recs)
            if (r.err) { s.err = r.err; return; }
    }
    s.dev_samples = dst;
    s.info.n_samples = offset;
    s.info.channels = (uint8_t)count0;
    s.info.sample_rate = rate0;
    s.info.bits_per_sample = (uint8_t)bps0;
}

}  // namespace zflac
