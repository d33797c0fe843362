// batch.h -- the types the host units share (pipeline.cpp, seq_planner.cpp, md5_host.cpp,
// export_host.cpp, abi.cpp): device buffers, a stream's and a class's state, the per-device run streams and
// md5 hub, the batch itself, and the prototypes of the functions one unit calls in another.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/zflac_hip.h"
#include "common.h"
#include "export_plan.h"
#include "resample_plan.h"
#include "stream_plan.h"

namespace zflac {

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct DeviceError {};
inline void ck(hipError_t e) {
    if (e != hipSuccess) throw DeviceError{};
}

// The C boundary: the code `f` returns, or the one that stands for what it threw. Nothing leaves.
template <typename F>
int guarded(F&& f) noexcept {
    try {
        return f();
    } catch (const DeviceError&) {
        return E_DEVICE;
    } catch (const std::bad_alloc&) {
        return E_OUT_OF_MEMORY;
    } catch (...) {  // e.g. std::system_error: a helper thread could not start
        return E_DEVICE;
    }
}

// ---------------------------------------------------------------------------------
// Device memory helpers
// ---------------------------------------------------------------------------------
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void alloc(size_t count) {
        if (count <= n && p) return;
        release();
        ck(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T)));
        n = count;
    }
};

// One polyphase tap table of a batch (zflac_hip_batch_export_resampled), kept in device memory
// under the parameters it was built from.
struct ResampleTable {
    uint32_t fin = 0, fout = 0, zeros = 0;
    double rolloff = 0, beta = 0;
    ResampleRatio ratio;
    DevBuf<float> taps;  // h[L][K]
};

struct StreamState : StreamPlan {  // the host parse (stream_plan.h), then:
    int cls = -1;
    uint32_t slot = 0;  // index inside its class
    // result
    int err = 0;
    zflac_info info = {};
    const void* dev_samples = nullptr;  // device pointer of the decoded samples
    int md5_dev = 0;                    // 0 not hashed on the device, 1 match, 2 mismatch
    uint8_t md5_dig[16] = {};           // device digest (md5_dev != 0)
    int md5_src = 0;                    // ZFLAC_MD5_SRC_* of md5_dig (zflac_hip_batch_md5_source)
    std::unique_ptr<DevBuf<uint8_t>> override_out;
};

struct Class {
    int kind = 1;
    int nch = 2;
    std::vector<uint32_t> members;  // stream indices
    std::vector<StreamDesc> desc;
    std::vector<ChunkDesc> chunks;
    uint64_t in_bytes = 0, out_elems = 0;
    uint32_t cap = 0;
    uint64_t est_frames = 0;  // frames expected from the STREAMINFO totals (walk choice)
    // frames the walk / decode grids are sized for (their loops stride over any excess): the
    // exact frame count of fixed-blocking streams with a STREAMINFO total, plus slack; raised
    // when a run finds more candidates (false syncs) than that
    uint32_t grid_frames = 0;
    // decode launches given a full grid (DecodeArgs::full_mask): the buckets predicted from
    // the first subframe of each member's first frame, at batch creation (plan_buckets)
    uint32_t full_mask = 0;
    bool redone = false;  // the last run re-ran the class (candidate table regrown)
    // The front that builds the frame table: k_scan + k_scan_chunks + k_compact, or k_hop
    // (plan_hop, stream_plan.h). A run whose hop lost a stream (h_misc[3] == hop_epoch) is redone
    // with the scan front by finish_batch, and the class keeps the scan front from then on.
    Front front = FRONT_SCAN;     // of the next run
    Front front_run = FRONT_SCAN, front_used = FRONT_SCAN;  // of the last run: enqueued with / results from
    std::vector<HopDesc> hop;
    DevBuf<HopDesc> d_hop;
    uint32_t hop_frames = 0;  // sum of the streams' frame counts
    uint32_t hop_epoch = 0;   // HopArgs::epoch of the last hop run
    DevBuf<uint8_t> in;
    DevBuf<uint8_t> out;
    DevBuf<StreamDesc> d_desc;
    DevBuf<ChunkDesc> d_chunks;
    DevBuf<uint32_t> chunk_cnt, chunk_off, chunk_slot_units, misc;  // misc: 4 counters, then `status`
    uint32_t* status = nullptr;  // per-member status words, misc.p + 4 (one read-back for both)
    DevBuf<unsigned long long> chunk_units, chunk_uoff;
    DevBuf<uint64_t> chunk_slots;
    DevBuf<uint64_t> c_pos, c_out, c_end;
    DevBuf<uint32_t> c_stream, c_info, c_rate, sub, group_mb;
    DevBuf<int32_t> c_err;
    DevBuf<uint32_t> crc_bad;  // k_crc16 verdict per candidate (ZFLAC_FLAG_CHECK_CRC16)
    DevBuf<uint8_t> dummy;  // sink of masked-off packed stores (64 lanes x 32 B)
    // pinned host mirror, so the per-run read-backs are plain DMA on the batch stream:
    // [0] n_frames, [1] overflow, [2] decode buckets used, [3] unused, then one status word per member
    struct Pinned {
        uint32_t* p = nullptr;
        ~Pinned() {
            if (p) (void)hipHostFree(p);
        }
    } pin;
    uint32_t* h_misc = nullptr;
    uint32_t* h_status = nullptr;
    // members whose STREAMINFO total is unknown but whose output is reserved (unknown_total_cap):
    // k_verify certifies their chain to the end of the stream and writes its length here
    bool any_unknown = false;
    DevBuf<uint64_t> units;
    uint64_t* h_units = nullptr;  // pinned mirror, after the status words
};

// Makes `dev` the calling thread's current device for a scope and restores the previous
// one: hub flushes can be triggered from any batch's call (ready / wait / destroy), on a
// thread whose current device is another one.
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ck(hipSetDevice(dev));
    }
    ~DeviceScope() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// Copy streams into their HBM layout (stream m at in_off[m], zeros elsewhere, `total`
// bytes) through two pinned 32 MiB windows: host threads fill one window while the DMA
// engine drains the other. The windows are a lazily created per-process context, shared
// by all batches under a lock.
struct Uploader {
    static constexpr uint64_t WIN = 32ull << 20;
    std::mutex mu;
    uint8_t* pin[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
};

// ---------------------------------------------------------------------------------
// md5 hub: one per device. MD5 is one serial chain per stream (~8 ms for a C5 stream of
// 32 frames), so a run's hash lasts as long as its longest chain whatever its lane count.
// Hashing each run on its own batch stream made the decode+MD5 throughput the number of
// batches in flight over (decode + hash latency), and each batch held a hardware queue for
// its whole hash. The hub collects the DEVICE_MD5 runs whose decode has been enqueued and
// hashes up to MD5_MAX_SEGS of them in ONE k_md5_coop launch on its own stream (waiting
// on each run's decode event), so few launches and few hardware queues carry every chain.
// A run is flushed into a launch once `runs` are pending, when its batch is waited on, or
// when its batch polls _ready with its decode done and no hub launch in flight.
// ---------------------------------------------------------------------------------
constexpr int MAX_HUB_STREAMS = 4;
struct Md5Hub {
    std::mutex mu;
    hipStream_t st[MAX_HUB_STREAMS] = {};  // launches alternate between the first n_st
    uint32_t n_st = 1, next = 0;
    hipEvent_t last = nullptr;  // behind the newest hub launch
    bool any = false;
    std::vector<zflac_batch*> pend;
    uint32_t runs = 8;
    int device = 0;  // the hub's launches and copies run with this device current
};

// The device's run streams: every batch run (zflac_hip_batch_submit) goes to the next one
// in turn, so any number of batches in flight use n_run (3 by default) hardware queues (runs
// on one stream execute in submit order). bench.py keeps four runs in flight and sets
// ZFLAC_RUN_STREAMS from its --inflight (four: 1-3 % faster than three since round 4).
// Created before any batch's own stream, so that with enough hardware queues
// (GPU_MAX_HW_QUEUES) the run streams and the md5 hub stream each hold one of their own.
// ZFLAC_RUN_STREAMS / ZFLAC_HUB_STREAMS override the counts (at most 8 / 4).
constexpr int MAX_RUN_STREAMS = 8;
struct DeviceStreams {
    std::mutex mu;
    hipStream_t run[MAX_RUN_STREAMS] = {};
    uint32_t n_run = 3, next = 0;
    Md5Hub hub;
    DeviceStreams();
};

// md5_host.cpp
DeviceStreams& device_streams(int device);  // (call with the device current)
Md5Hub& md5_hub(int device);
hipStream_t next_run_stream(int device);
void hub_flush(Md5Hub& h);           // one launch over every pending run (caller holds h.mu)
void hub_release(zflac_batch* b);    // flush a run still pending in its device's md5 hub
void hub_forget(zflac_batch* b);     // drop a run from its device's md5 hub without hashing it
int read_samples(zflac_batch* b, StreamState& s, void* out, bool hash);
// Internal batch flag (never set by a caller of the ABI): the kernels store the samples without
// the left-justify shift. Only md5_before_justify creates such a batch.
constexpr int FLAG_NO_JUSTIFY = 1 << 30;
// After a digest mismatch of a left-justified stream: is the digest of its samples before the
// shift STREAMINFO's, as zflac hashes them (src/zflac.zig:267-306)?
bool md5_before_justify(zflac_batch* b, StreamState& s);
void plan_md5_pipeline(zflac_batch* b);
void finish_md5(zflac_batch* b, bool timing);

// pipeline.cpp
DecodeArgs decode_args(Class& C);
ScanArgs scan_args(Class& C);
CompactArgs compact_args(Class& C);
HopArgs hop_args(Class& C);  // (a new epoch each call)
// k_walk or k_walk_wave (subframe start offsets, 2+ channels) then k_decode; `mid`
// (optional) is recorded between the two launches. With a `front` stream the walk runs
// there and k_decode waits for it on `st` through the event `join`. `est_frames`: the
// frame count the walk choice is made for (the launch grid is sized for `max_frames`).
hipError_t launch_decode(int kind, const DecodeArgs& a, uint32_t max_frames, hipStream_t st,
                         hipEvent_t mid = nullptr, hipStream_t front = nullptr, hipEvent_t join = nullptr,
                         uint64_t est_frames = 0, int flags = 0);
void enqueue_class(zflac_batch* b, Class& C, bool timing_first, bool timing_last);
void submit_batch(zflac_batch* b);
void finish_batch(zflac_batch* b);
int create_batch(const zflac_stream* streams, size_t n, int device, int flags, zflac_batch** out);

// seq_planner.cpp
void finish_stream_sequential(zflac_batch* b, Class& C, uint32_t slot, const std::vector<uint32_t>& h_chunk_off,
                              uint32_t nframes);

// export_host.cpp
// The four dense exports: plan (export_plan.h), write the row records, stage the tables, launch,
// and finish as the caller's stream asks.
int export_dense(zflac_batch* b, const ExportCall& call, const zflac_mix_desc* mix, void* dst, size_t dst_bytes,
                 uint64_t* valid_frames, void* stream);

// mel_host.cpp
// The feature plan (zflac_mel: the device tables and the plan's own stream) and its runs; the
// argument checks, the tables and the grid rule are mel_plan.h's.
int mel_create(const zflac_mel_desc* d, uint32_t math, int device, zflac_mel** out);
// f != NULL: zflac_hip_mel_create_framed
int mel_create_framed(const zflac_mel_desc* d, const zflac_mel_frame_desc* f, uint32_t math, int device, zflac_mel** out);
uint64_t mel_plan_frames_of(const zflac_mel* m, uint64_t n_samples);
int mel_cmvn(zflac_mel* m, const zflac_mel_cmvn_desc* c, void* stream);
int mel_math(const zflac_mel* m);
int mel_run(zflac_mel* m, const float* wave, uint64_t rows, uint64_t wave_frames, uint64_t row_stride,
            uint64_t first_frame, uint64_t frames, void* dst, size_t dst_bytes, void* stream);
int mel_run_ex(zflac_mel* m, const zflac_mel_run_desc* r, void* stream);
void mel_destroy(zflac_mel* m);

// cepstra_host.cpp
// The cepstra plan (zflac_cepstra: the matrix and the delta scales on the device, the plan's own
// stream) and its runs; the argument checks, the scales and the grids are cepstra_plan.h's.
int cepstra_create(const zflac_cepstra_desc* d, int device, zflac_cepstra** out);
uint32_t cepstra_features(const zflac_cepstra* c);
int cepstra_delta_scales_of(const zflac_cepstra* c, uint32_t order, float* out, uint32_t cap);
int cepstra_project(zflac_cepstra* c, const zflac_cepstra_project_desc* r, void* stream);
int cepstra_cmvn(zflac_cepstra* c, const zflac_mel_cmvn_desc* d, void* stream);
int cepstra_deltas(zflac_cepstra* c, const zflac_cepstra_delta_desc* r, void* stream);
void cepstra_destroy(zflac_cepstra* c);

}  // namespace zflac

// ---------------------------------------------------------------------------------
// Batch
// ---------------------------------------------------------------------------------
struct zflac_batch {
    int device = 0;
    int flags = 0;
    hipStream_t stream = nullptr;
    // ZFLAC_FRONT_PRIORITY=1: a second, highest-priority stream for the scan / compact / walk
    // of each run, so that with several runs in flight their workgroups are dispatched ahead
    // of another run's decode workgroups (an experiment knob; nullptr = one stream)
    hipStream_t front = nullptr;
    hipEvent_t front_join = nullptr;
    std::vector<zflac::StreamState> streams;
    std::vector<std::unique_ptr<zflac::Class>> classes;
    hipEvent_t ev[10] = {};
    hipEvent_t ev_done = nullptr;  // recorded behind the last work _submit enqueued (_ready)
    // the HIP stream of the run in flight: one of the device's run streams (DeviceStreams),
    // so that many batches in flight share a few hardware queues; `stream` (the batch's own)
    // carries the synchronous work (upload, regrowth, the sequential planner, read-backs)
    hipStream_t rs = nullptr;
    // ZFLAC_FLAG_DEVICE_MD5 runs hash in the device's md5 hub (one k_md5_coop launch over
    // the runs of several batches, on the hub's stream): ev_done then marks the decode only,
    // ev_md5 the hash and its digest read-back; md5_pending until the hub launched it
    hipEvent_t ev_md5 = nullptr;
    // written under the hub's lock, read without it by _ready / hub_release (other threads
    // flush the hub from their own batches' submit / wait / ready)
    std::atomic<bool> md5_pending{false};
    bool md5_failed = false;  // the hub launch that held this run threw: its digests are void
    bool md5_hub = false;  // this run's hash goes through the hub
    bool have_timing = false;
    bool ran = false;        // results exist only after a completed batch_run / batch_wait
    bool submitted = false;  // batch_submit enqueued a run that batch_wait has not finished
    double submit_t0 = 0;    // host clock at submit (run_wall_ms)
    zflac::DevBuf<zflac::Md5Job> md5_jobs;
    zflac::DevBuf<uint32_t> md5_dig;
    // ZFLAC_FLAG_DEVICE_MD5: k_md5 over every certifiable stream, enqueued by submit behind
    // the run's k_verify (pipe_who[k] = stream of job k, longest first); its digests land in
    // pinned memory with the run's other read-backs
    zflac::DevBuf<zflac::Md5Job> pipe_jobs;
    int pipe_coop = -1;  // coop_mode_of(the pipe jobs)
    zflac::DevBuf<uint32_t> pipe_dig;
    std::vector<uint32_t> pipe_who;
    uint32_t* pipe_pin = nullptr;
    zflac_timings timings = {};
    // zflac_hip_batch_export / _export_resampled: the per-row table (ExportRow or ResampleRow
    // records, room for the larger) goes through exp_pin (pinned) into exp_rows with an async copy
    // on the export's stream. ev_exp_copy marks that copy (the next export
    // waits for it on the host before it refills exp_pin), ev_exp the kernel (the next export's
    // stream waits for it before it overwrites exp_rows; while exp_pending, so do the next
    // run's streams before they overwrite the samples, and the destructor on the host).
    uint8_t* exp_pin = nullptr;
    zflac::DevBuf<uint8_t> exp_rows;
    // the streams as the export planner sees them: scratch of one call (refilled by each, nothing
    // carried between calls), kept here only so that a call allocates nothing
    std::vector<zflac::ExportStream> exp_views;
    hipEvent_t ev_exp_copy = nullptr, ev_exp = nullptr;
    hipEvent_t ev_exp_t[2] = {};  // ZFLAC_FLAG_TIMING: around a synchronous export
    bool exp_any = false;      // ev_exp_copy / ev_exp have been recorded
    bool exp_pending = false;  // an export on a caller's stream may still read the samples
    double export_ms = -1;
    // the resampled export's tap tables, one per distinct (source rate, target rate, zeros,
    // rolloff, beta) met so far; a later export with the same parameters builds nothing
    std::vector<std::unique_ptr<zflac::ResampleTable>> rs_tables;
    uint64_t rs_built = 0;  // tables built over the batch's lifetime
    // zflac_hip_batch_decode_buckets: over the classes, the buckets the last completed run's
    // classification found (h_misc[2]) and the launch plan (full_mask) that run was enqueued with
    uint32_t buckets_used = 0, buckets_planned = 0;
    // zflac_hip_batch_front: over the classes, the fronts the last completed run was enqueued
    // with and the ones its frame tables came from (ZFLAC_FRONT_*)
    int front_planned = 0, front_used = 0;
    // zflac_hip_batch_md5_stats: the Md5Kernel of the pipelined launch that holds the run in flight
    // (set by submit on the run stream, or by the hub's flush under the hub's lock, before
    // md5_pending falls), the kernels the last completed run's digests came from, and the stream
    // decodes of md5_before_justify over the batch's lifetime
    uint32_t md5_pipe_kernel = 0, md5_kernels = 0;
    uint64_t md5_rechecks = 0;
    ~zflac_batch();  // abi.cpp
};
