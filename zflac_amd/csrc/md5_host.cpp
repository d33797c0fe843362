// md5_host.cpp -- the host side of MD5 verification and of the per-device streams: the run
// streams and the md5 hub (declared in batch.h), the host hash of a sample read-back, and
// the device hash of a run (pipelined through the hub, or synchronous for the rest).
#include <cstdlib>
#include <cstring>
#include <thread>
#include <unordered_map>

#include "batch.h"
#include "launch.h"
#include "md5.hpp"

namespace zflac {

// ZFLAC_HUB_CUS=N (N > 0): the md5 hub's streams on N CUs of their own and the run streams on
// the others (hipExtStreamCreateWithCUMask; the lowest N bits of the device's CU mask). The
// hash is one serial chain per stream, compute-only: on CUs it shares with the decode, its
// waves slow the decode waves there, and a decode launch ends with its slowest wave.
static uint32_t hub_cus() {
    const char* e = std::getenv("ZFLAC_HUB_CUS");
    return e ? (uint32_t)std::max(0, atoi(e)) : 0u;
}

DeviceStreams::DeviceStreams() {
    if (const char* e = std::getenv("ZFLAC_RUN_STREAMS")) n_run = (uint32_t)std::max(1, std::min(atoi(e), MAX_RUN_STREAMS));
    if (const char* e = std::getenv("ZFLAC_HUB_STREAMS")) hub.n_st = (uint32_t)std::max(1, std::min(atoi(e), MAX_HUB_STREAMS));
    const uint32_t nh = hub_cus();
    int dev = 0, ncu = 0;
    ck(hipGetDevice(&dev));
    ck(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    if (nh > 0 && nh < (uint32_t)ncu) {
        const uint32_t words = ((uint32_t)ncu + 31) / 32;
        std::vector<uint32_t> hm(words, 0u), rm(words, 0u);
        for (uint32_t c = 0; c < (uint32_t)ncu; c++) (c < nh ? hm : rm)[c / 32] |= 1u << (c % 32);
        for (uint32_t i = 0; i < n_run; i++) ck(hipExtStreamCreateWithCUMask(&run[i], words, rm.data()));
        for (uint32_t i = 0; i < hub.n_st; i++) ck(hipExtStreamCreateWithCUMask(&hub.st[i], words, hm.data()));
    } else {
        for (uint32_t i = 0; i < n_run; i++) ck(hipStreamCreateWithFlags(&run[i], hipStreamNonBlocking));
        for (uint32_t i = 0; i < hub.n_st; i++) ck(hipStreamCreateWithFlags(&hub.st[i], hipStreamNonBlocking));
    }
    ck(hipEventCreateWithFlags(&hub.last, hipEventDisableTiming));
    if (const char* e = std::getenv("ZFLAC_MD5_RUNS")) hub.runs = (uint32_t)std::max(1, std::min(atoi(e), MD5_MAX_SEGS));
}

// (call with the device current)
DeviceStreams& device_streams(int device) {
    static std::mutex mu;
    static std::unordered_map<int, DeviceStreams*> per_device;  // never destroyed: outlives every batch
    std::lock_guard<std::mutex> lock(mu);
    DeviceStreams*& d = per_device[device];
    if (!d) {
        d = new DeviceStreams();
        d->hub.device = device;
    }
    return *d;
}

Md5Hub& md5_hub(int device) { return device_streams(device).hub; }

hipStream_t next_run_stream(int device) {
    DeviceStreams& d = device_streams(device);
    std::lock_guard<std::mutex> lock(d.mu);
    return d.run[d.next++ % d.n_run];
}

// The launch of hub_flush: every pending run in one k_md5 launch on the next hub stream.
static void hub_flush_runs(Md5Hub& h) {
    // fault injection for the tests only (tests/test_gpu.py: a failed hub launch must not
    // poison the batch's next run): ZFLAC_FAULT_HUB_FLUSH=1 makes this flush throw
    if (const char* f = std::getenv("ZFLAC_FAULT_HUB_FLUSH"); f && f[0] == '1') throw DeviceError{};
    hipStream_t hs = h.st[h.next++ % h.n_st];
    Md5Segs sg;
    std::memset(&sg, 0, sizeof(sg));
    uint32_t n = 0;
    int coop = h.pend[0]->pipe_coop;  // the cooperative kernel only when every run's jobs allow it
    for (zflac_batch* b : h.pend) {
        if (b->pipe_coop != coop) coop = -1;
        ck(hipStreamWaitEvent(hs, b->ev_done, 0));
        sg.jobs[sg.nseg] = b->pipe_jobs.p;
        sg.dig[sg.nseg] = b->pipe_dig.p;
        sg.start[sg.nseg] = n;
        n += (uint32_t)b->pipe_who.size();
        sg.nseg++;
    }
    sg.start[sg.nseg] = n;
    for (zflac_batch* b : h.pend)  // every run gets the shared launch's time (md5_ms)
        if (b->flags & ZFLAC_FLAG_TIMING) ck(hipEventRecord(b->ev[8], hs));
    uint32_t kernel = 0;
    ck(launch_md5_multi(sg, hs, coop, &kernel));
    for (zflac_batch* b : h.pend) {
        b->md5_pipe_kernel = kernel;  // every run of the flush: one launch hashes them all
        if (b->flags & ZFLAC_FLAG_TIMING) ck(hipEventRecord(b->ev[9], hs));
        ck(hipMemcpyAsync(b->pipe_pin, b->pipe_dig.p, b->pipe_who.size() * 16, hipMemcpyDeviceToHost, hs));
        ck(hipEventRecord(b->ev_md5, hs));
        b->md5_pending = false;
    }
    ck(hipEventRecord(h.last, hs));
    h.any = true;
    h.pend.clear();
}

// One launch over every pending run (caller holds hub.mu). Any exit, a throwing HIP call
// included, leaves the hub empty: the runs of a launch that failed part way are marked
// md5_failed (their wait reports DeviceError) instead of staying queued, so no later flush
// can touch a batch destroyed in between.
void hub_flush(Md5Hub& h) {
    if (h.pend.empty()) return;
    try {
        DeviceScope dev(h.device);
        hub_flush_runs(h);
    } catch (...) {
        for (zflac_batch* b : h.pend) {
            if (b->md5_pending) b->md5_failed = true;
            b->md5_pending = false;
        }
        h.pend.clear();
        throw;
    }
}

// The run's hash launched (flushing the hub if it is still pending).
void hub_release(zflac_batch* b) {
    if (!b->md5_pending) return;
    Md5Hub& h = md5_hub(b->device);
    std::lock_guard<std::mutex> lock(h.mu);
    if (b->md5_pending) hub_flush(h);
}

// Drop the run from the hub without hashing it (a failed submit or wait, a destroyed batch).
void hub_forget(zflac_batch* b) {
    Md5Hub& h = md5_hub(b->device);
    std::lock_guard<std::mutex> lock(h.mu);
    h.pend.erase(std::remove(h.pend.begin(), h.pend.end(), b), h.pend.end());
    b->md5_pending = false;
    b->md5_failed = false;  // a forgotten run has no hash to fail; never leak into the next run
}

// MD5 of the decoded stream exactly as zflac hashes it: before left-justify, 24-bit
// containers hash 3 bytes per sample (src/zflac.zig:267-280). Fed in element-aligned
// pieces, so the read can hash chunks as they land.
namespace {
class SampleHasher {
public:
    // `justified`: the samples carry the left-justify shift (false: decoded without it)
    explicit SampleHasher(const StreamState& s, bool justified = true)
        : kind_(s.kind), js_(justified ? justify_of(s.si.bps) : 0), w24_((s.si.bps + 7) / 8 * 8 == 24) {}
    void update(const void* samples, uint64_t n) {  // n elements of the stream's container
        if (kind_ == 0 || (kind_ == 1 && !js_) || (kind_ == 2 && !js_ && !w24_)) {
            md_.update(samples, n * (kind_ == 0 ? 1 : kind_ == 1 ? 2 : 4));
            return;
        }
        uint8_t tmp[4096 * 4];
        for (uint64_t i = 0; i < n; i += 4096) {
            const uint64_t m = std::min<uint64_t>(4096, n - i);
            if (kind_ == 1) {
                const int16_t* v = static_cast<const int16_t*>(samples) + i;
                int16_t* t = reinterpret_cast<int16_t*>(tmp);
                for (uint64_t k = 0; k < m; k++) t[k] = (int16_t)(v[k] >> js_);
                md_.update(tmp, m * 2);
            } else {
                const int32_t* v = static_cast<const int32_t*>(samples) + i;
                const int w = w24_ ? 3 : 4;
                for (uint64_t k = 0; k < m; k++) {
                    const uint32_t x = (uint32_t)(v[k] >> js_);
                    for (int bb = 0; bb < w; bb++) tmp[k * w + bb] = (uint8_t)(x >> (8 * bb));
                }
                md_.update(tmp, m * w);
            }
        }
    }
    bool matches(const uint8_t* expected) {
        uint8_t dig[16];
        md_.finish(dig);
        return std::memcmp(dig, expected, 16) == 0;
    }

private:
    Md5 md_;
    int kind_;
    uint32_t js_;
    bool w24_;
};
}  // namespace

static bool md5_matches(const StreamState& s, const void* host_samples) {
    SampleHasher h(s);
    h.update(host_samples, s.info.n_samples);
    return h.matches(s.si.md5);
}

// zflac hashes before it left-justifies, and keeps a predicted sample that leaves the stream's
// depth as long as it fits the SampleType. The shift then pushes bits out that the hash reads
// (a 12-bit stream's sample of 32767), and the digest of the justified samples, shifted back,
// is not zflac's. So a mismatch of a justified stream is checked once more: the stream alone,
// decoded again without the shift (FLAG_NO_JUSTIFY), hashed on the host. Streams inside their
// depth never come here with a good digest; a stream that really fails its checksum pays one
// more decode.
bool md5_before_justify(zflac_batch* b, StreamState& s) {
    if (!justify_of(s.si.bps) || s.cls < 0 || (b->flags & FLAG_NO_JUSTIFY)) return false;
    b->md5_rechecks++;  // (zflac_hip_batch_md5_stats: from here on the stream is decoded again)
    const Class& C = *b->classes[s.cls];
    const StreamDesc& D = C.desc[s.slot];
    std::vector<uint8_t> bytes(s.len);
    ck(hipMemcpy(bytes.data(), C.in.p + (D.in_begin - s.frames_begin), s.len, hipMemcpyDeviceToHost));
    const zflac_stream in{bytes.data(), bytes.size()};
    zflac_batch* raw = nullptr;
    if (create_batch(&in, 1, b->device, FLAG_NO_JUSTIFY, &raw) != E_OK) return false;
    std::unique_ptr<zflac_batch> hold(raw);
    try {
        submit_batch(raw);
        finish_batch(raw);
    } catch (...) {  // nothing of it may still run when the batch is freed
        (void)hipStreamSynchronize(raw->stream);
        if (raw->rs) (void)hipStreamSynchronize(raw->rs);
        throw;
    }
    const StreamState& t = raw->streams[0];
    if (t.err || !t.dev_samples || t.info.n_samples != s.info.n_samples) return false;
    std::vector<uint8_t> samples(t.info.samples_bytes);
    if (!samples.empty()) ck(hipMemcpy(samples.data(), t.dev_samples, samples.size(), hipMemcpyDeviceToHost));
    SampleHasher h(s, /*justified=*/false);
    h.update(samples.data(), t.info.n_samples);
    return h.matches(s.si.md5);
}

// D2H of one stream's samples into caller memory, with the STREAMINFO MD5 when `hash`.
// Long streams: the calling thread copies chunk after chunk while a helper thread hashes
// every chunk already landed, so the call costs about max(D2H, MD5) instead of their sum.
int read_samples(zflac_batch* b, StreamState& s, void* out, bool hash) {
    const uint64_t bytes = s.info.samples_bytes;
    const uint64_t esz = (uint64_t)esz_of_kind(s.kind);
    constexpr uint64_t CHUNK = 32ull << 20;  // a multiple of every element size
    const double t0 = now_ms();
    double t_md5 = 0;
    bool ok = true;
    if (!hash || bytes <= 2 * CHUNK) {
        if (bytes) ck(hipMemcpy(out, s.dev_samples, bytes, hipMemcpyDeviceToHost));
        if (hash) {
            const double t1 = now_ms();
            ok = md5_matches(s, out);
            t_md5 = now_ms() - t1;
        }
    } else {
        std::atomic<uint64_t> landed{0};
        std::thread hasher([&] {
            const double h0 = now_ms();
            SampleHasher h(s);
            uint64_t done = 0;
            while (done < bytes) {
                const uint64_t l = landed.load(std::memory_order_acquire);
                if (l == done) {
                    std::this_thread::yield();
                    continue;
                }
                h.update(static_cast<const uint8_t*>(out) + done, (l - done) / esz);
                done = l;
            }
            ok = h.matches(s.si.md5);
            t_md5 = now_ms() - h0;
        });
        hipError_t e = hipSuccess;
        for (uint64_t off = 0; off < bytes; off += CHUNK) {
            const uint64_t len = std::min(CHUNK, bytes - off);
            if (e == hipSuccess)
                e = hipMemcpy(static_cast<uint8_t*>(out) + off, static_cast<const uint8_t*>(s.dev_samples) + off, len,
                              hipMemcpyDeviceToHost);
            landed.store(off + len, std::memory_order_release);  // on failure: drain the hasher
        }
        hasher.join();
        ck(e);
    }
    b->timings.read_ms = now_ms() - t0;
    b->timings.host_md5_ms = t_md5;
    return ok ? E_OK : E_INVALID_CHECKSUM;
}

// k_md5 job of stream s over `n` samples at `data` (device), as zflac hashes them.
static Md5Job md5_job(const StreamState& s, const void* data, uint64_t n, const uint32_t* status) {
    Md5Job j{};
    j.data = static_cast<const uint8_t*>(data);
    j.n = n;
    j.status = status;
    const uint32_t js = justify_of(s.si.bps);
    j.js = js;
    if (s.kind == 0) {
        j.mode = MD5_RAW, j.width = 1;
    } else if (s.kind == 1) {
        j.mode = js ? MD5_S16_SHIFT : MD5_RAW, j.width = 2;
    } else if ((s.si.bps + 7) / 8 * 8 == 24) {
        j.mode = MD5_S24, j.width = 3;
    } else {
        j.mode = js ? MD5_S32_SHIFT : MD5_RAW, j.width = 4;
    }
    return j;
}

// The Md5Mode all `jobs` share when every one's samples are 16-byte aligned: k_md5_coop
// (cooperative loads) can hash them; else -1 (k_md5, each lane its own loads).
static int coop_mode_of(const std::vector<Md5Job>& jobs) {
    if (jobs.empty() || std::getenv("ZFLAC_MD5_LANE_LOADS")) return -1;
    for (const Md5Job& j : jobs)
        if (j.mode != jobs[0].mode || (reinterpret_cast<uintptr_t>(j.data) & 15) != 0) return -1;
    return (int)jobs[0].mode;
}

// Order of `jobs` longest message first: the lanes of a wave then run chains of similar length.
static std::vector<uint32_t> longest_first(const std::vector<Md5Job>& jobs) {
    std::vector<uint32_t> ord(jobs.size());
    for (uint32_t k = 0; k < ord.size(); k++) ord[k] = k;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) {
        return jobs[x].n * jobs[x].width > jobs[y].n * jobs[y].width;
    });
    return ord;
}

// Digest words (k_md5 layout) -> the stream's verdict; a mismatch becomes its error, as
// decode() returns InvalidChecksum (src/zflac.zig:279-280).
static void take_digest(StreamState& s, const uint32_t* d, int src) {
    s.md5_src = src;
    for (int w = 0; w < 4; w++)
        for (int q = 0; q < 4; q++) s.md5_dig[4 * w + q] = (uint8_t)(d[w] >> (8 * q));
    s.md5_dev = std::memcmp(s.md5_dig, s.si.md5, 16) == 0 ? 1 : 2;
    if (s.md5_dev == 2) s.err = E_INVALID_CHECKSUM;
}

// ZFLAC_FLAG_DEVICE_MD5 at batch creation: one k_md5 job per stream the parallel pass can
// certify (STREAMINFO total known), over its region of the class output, gated on the run's
// k_verify status; submit enqueues them behind the run (pipelined: the hash of one batch runs
// beside the decode of the others in flight).
void plan_md5_pipeline(zflac_batch* b) {
    std::vector<Md5Job> jobs;
    std::vector<uint32_t> who;
    for (auto& cp : b->classes) {
        Class& C = *cp;
        const int esz = esz_of_kind(C.kind);
        for (size_t m = 0; m < C.members.size(); m++) {
            const StreamDesc& D = C.desc[m];
            if (!D.valid_total) continue;
            jobs.push_back(md5_job(b->streams[C.members[m]], C.out.p + D.out_base * esz, D.total, C.status + m));
            who.push_back(C.members[m]);
        }
    }
    if (jobs.empty()) return;
    const std::vector<uint32_t> ord = longest_first(jobs);
    std::vector<Md5Job> sorted(jobs.size());
    b->pipe_who.resize(jobs.size());
    for (size_t k = 0; k < ord.size(); k++) {
        sorted[k] = jobs[ord[k]];
        b->pipe_who[k] = who[ord[k]];
    }
    b->pipe_coop = coop_mode_of(sorted);
    b->pipe_jobs.alloc(sorted.size());
    b->pipe_dig.alloc(sorted.size() * 4);
    ck(hipMemcpy(b->pipe_jobs.p, sorted.data(), sorted.size() * sizeof(Md5Job), hipMemcpyHostToDevice));
    ck(hipHostMalloc(reinterpret_cast<void**>(&b->pipe_pin), sorted.size() * 16, hipHostMallocDefault));
}

// STREAMINFO MD5 of the streams `which` on the device (k_md5, one lane per stream),
// synchronously: the streams the pipelined hash could not cover (decoded by the sequential
// planner, or re-run after a candidate-table regrowth).
static void run_md5_device(zflac_batch* b, const std::vector<uint32_t>& which, bool timing) {
    std::vector<Md5Job> jobs;
    for (uint32_t i : which) {
        const StreamState& s = b->streams[i];
        jobs.push_back(md5_job(s, s.dev_samples, s.info.n_samples, nullptr));
    }
    if (jobs.empty()) return;
    const std::vector<uint32_t> ord = longest_first(jobs);
    std::vector<Md5Job> sorted(jobs.size());
    for (size_t k = 0; k < ord.size(); k++) sorted[k] = jobs[ord[k]];
    b->md5_jobs.alloc(sorted.size());
    b->md5_dig.alloc(sorted.size() * 4);
    ck(hipMemcpyAsync(b->md5_jobs.p, sorted.data(), sorted.size() * sizeof(Md5Job), hipMemcpyHostToDevice,
                      b->stream));
    if (timing) ck(hipEventRecord(b->ev[5], b->stream));
    uint32_t kernel = 0;
    ck(launch_md5(b->md5_jobs.p, (uint32_t)sorted.size(), b->md5_dig.p, b->stream, coop_mode_of(sorted), &kernel));
    b->md5_kernels |= kernel;
    if (timing) ck(hipEventRecord(b->ev[6], b->stream));
    std::vector<uint32_t> dig(sorted.size() * 4);
    ck(hipMemcpyAsync(dig.data(), b->md5_dig.p, dig.size() * 4, hipMemcpyDeviceToHost, b->stream));
    ck(hipStreamSynchronize(b->stream));
    if (timing) {
        float t = 0;
        ck(hipEventElapsedTime(&t, b->ev[5], b->ev[6]));
        b->timings.md5_ms += t;
    }
    for (size_t k = 0; k < ord.size(); k++) take_digest(b->streams[which[ord[k]]], &dig[k * 4], ZFLAC_MD5_SRC_SYNC);
}

// After a run: the pipelined digests of the streams the run certified, then a synchronous
// k_md5 for every other decoded stream.
void finish_md5(zflac_batch* b, bool timing) {
    std::vector<char> done(b->streams.size(), 0);
    for (auto& s : b->streams) s.md5_dev = 0, s.md5_src = ZFLAC_MD5_SRC_NONE;
    b->md5_kernels = 0;
    if (!b->pipe_who.empty()) {
        if (timing) {
            float t = 0;
            ck(hipEventElapsedTime(&t, b->ev[8], b->ev[9]));
            b->timings.md5_ms = t;
        }
        for (size_t k = 0; k < b->pipe_who.size(); k++) {
            const uint32_t i = b->pipe_who[k];
            StreamState& s = b->streams[i];
            const Class& C = *b->classes[s.cls];
            if (s.err || !s.dev_samples || C.redone || C.h_status[s.slot] != 0 || (b->flags & ZFLAC_FLAG_FORCE_SLOW))
                continue;
            take_digest(s, b->pipe_pin + k * 4, ZFLAC_MD5_SRC_PIPELINED);
            b->md5_kernels |= b->md5_pipe_kernel;
            done[i] = 1;
        }
    }
    std::vector<uint32_t> rest;
    for (uint32_t i = 0; i < b->streams.size(); i++)
        if (!done[i] && !b->streams[i].err && b->streams[i].dev_samples) rest.push_back(i);
    run_md5_device(b, rest, timing);
    for (auto& s : b->streams) {  // a mismatch of a justified stream: once more, before the shift
        if (s.md5_dev == 2 && md5_before_justify(b, s)) {
            s.err = E_OK;
            s.md5_dev = 1;
            s.md5_src = ZFLAC_MD5_SRC_HOST_RECHECK;
            std::memcpy(s.md5_dig, s.si.md5, 16);  // the digest as zflac takes it
        }
    }
}

}  // namespace zflac
