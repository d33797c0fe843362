// abi.cpp -- the extern "C" ABI of include/zflac_hip.h over the host units (batch.h), the
// batch's destructor, the build id, and the entry points of the diagnostic builds.
#include <cstring>

#include "batch.h"
#include "launch.h"
#include "mel_plan.h"

using namespace zflac;

zflac_batch::~zflac_batch() {
    if (exp_pending) (void)hipEventSynchronize(ev_exp);  // a caller's stream may still read the samples
    if (stream) (void)hipStreamSynchronize(stream);  // a submitted run may still use the buffers
    if (ev_done) (void)hipEventSynchronize(ev_done);  // ... on its run stream
    if (md5_pending) {  // still in the md5 hub: flush it, then let the hash finish
        try {
            hub_release(this);
        } catch (...) {
        }
        try {
            hub_forget(this);  // never leave a pointer to this batch in the hub
        } catch (...) {
        }
    }
    if (md5_hub && ev_md5) (void)hipEventSynchronize(ev_md5);
    if (front) (void)hipStreamSynchronize(front);
    classes.clear();
    for (auto& s : streams) s.override_out.reset();
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
    if (ev_done) (void)hipEventDestroy(ev_done);
    if (ev_md5) (void)hipEventDestroy(ev_md5);
    if (pipe_pin) (void)hipHostFree(pipe_pin);
    if (exp_pin) (void)hipHostFree(exp_pin);
    if (ev_exp_copy) (void)hipEventDestroy(ev_exp_copy);
    if (ev_exp) (void)hipEventDestroy(ev_exp);
    for (auto& e : ev_exp_t)
        if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (front) (void)hipStreamDestroy(front);
    if (front_join) (void)hipEventDestroy(front_join);
}

extern "C" {

const char* zflac_hip_error_name(int code) {
    switch (code) {
        case 0: return "OK";
        case 1: return "InvalidSignature";
        case 2: return "InvalidMetadataHeader";
        case 3: return "MissingStreaminfo";
        case 4: return "Unimplemented";
        case 5: return "InvalidChecksum";
        case 6: return "InvalidFrameHeader";
        case 7: return "InconsistentParameters";
        case 8: return "InvalidCodedNumber";
        case 9: return "InvalidSubframeHeader";
        case 10: return "InvalidResidualCodingMethod";
        case 11: return "EndOfStream";
        case 12: return "OutOfMemory";
        case 13: return "DeviceError";
        case 14: return "InvalidArgument";
        case 15: return "OutOfDomain";
        case 16: return "FrameCrcMismatch";
        default: return "Unknown";
    }
}

int zflac_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* zflac_hip_version(void) { return "zflac_hip gfx950 r4"; }

#ifndef ZFLAC_BUILD_ID
#define ZFLAC_BUILD_ID "unknown"
#endif
const char* zflac_hip_build_id(void) { return ZFLAC_BUILD_ID; }

int zflac_hip_batch_create(const zflac_stream* streams, size_t n, int device, int flags, zflac_batch** out) {
    return create_batch(streams, n, device, flags, out);
}

// After a failed submit: the work already enqueued (on the batch stream and, with
// ZFLAC_FRONT_PRIORITY, the front stream) may still use the candidate buffers a retry
// reallocates.
static void drain_failed_submit(zflac_batch* b) {
    try {
        hub_forget(b);
    } catch (...) {
    }
    (void)hipStreamSynchronize(b->stream);
    if (b->rs) (void)hipStreamSynchronize(b->rs);
    if (b->front) (void)hipStreamSynchronize(b->front);
    b->rs = b->stream;
    b->submitted = false;
}

int zflac_hip_batch_submit(zflac_batch* b) {
    if (!b || b->submitted) return E_INVALID_ARGUMENT;
    b->ran = false;
    const int rc = guarded([&]() -> int {
        b->submit_t0 = now_ms();
        b->submitted = true;
        submit_batch(b);
        return E_OK;
    });
    if (rc) drain_failed_submit(b);
    return rc;
}

int zflac_hip_batch_wait(zflac_batch* b) {
    if (!b || !b->submitted) return E_INVALID_ARGUMENT;
    b->submitted = false;
    const int rc = guarded([&]() -> int {
        finish_batch(b);
        b->timings.run_wall_ms = now_ms() - b->submit_t0;
        b->ran = true;
        return E_OK;
    });
    if (rc != E_OK && b->md5_pending) {  // failed before the hub released this run
        try {
            hub_forget(b);
        } catch (...) {
        }
    }
    return rc;
}

int zflac_hip_batch_ready(zflac_batch* b) {
    if (!b || !b->submitted) return -E_INVALID_ARGUMENT;
    hipError_t e = hipEventQuery(b->ev_done);
    if (e == hipSuccess && b->md5_hub) {
        try {
            Md5Hub& h = md5_hub(b->device);
            std::lock_guard<std::mutex> lock(h.mu);
            if (b->md5_pending) {  // decoded, hash not launched: launch it if the hub is idle
                if (!h.any || hipEventQuery(h.last) == hipSuccess) hub_flush(h);
                return 0;
            }
            // the hub launch holding this run failed (possibly another thread's flush): ev_md5
            // was never recorded for this run, so it must not be queried
            if (b->md5_failed) return -E_DEVICE;
        } catch (const DeviceError&) {
            return -E_DEVICE;
        }
        e = hipEventQuery(b->ev_md5);
    }
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) return 0;
    return -E_DEVICE;
}

int zflac_hip_batch_run(zflac_batch* b) {
    const int rc = zflac_hip_batch_submit(b);
    return rc ? rc : zflac_hip_batch_wait(b);
}

size_t zflac_hip_batch_size(zflac_batch* b) { return b ? b->streams.size() : 0; }

int zflac_hip_batch_info(zflac_batch* b, size_t i, zflac_info* info) {
    if (!b || !b->ran || i >= b->streams.size()) return E_INVALID_ARGUMENT;
    const StreamState& s = b->streams[i];
    if (info) *info = s.info;
    return s.err;
}

const void* zflac_hip_batch_device_samples(zflac_batch* b, size_t i) {
    if (!b || !b->ran || i >= b->streams.size() || b->streams[i].err) return nullptr;
    return b->streams[i].dev_samples;
}

int zflac_hip_batch_read(zflac_batch* b, size_t i, void* out, size_t out_bytes, int verify_md5) {
    if (!b || !b->ran || i >= b->streams.size()) return E_INVALID_ARGUMENT;
    StreamState& s = b->streams[i];
    if (s.err) return s.err;
    if (out_bytes < s.info.samples_bytes || (!out && s.info.samples_bytes)) return E_INVALID_ARGUMENT;
    return guarded([&]() -> int {
        ck(hipSetDevice(b->device));
        // a device verdict stands in for the host hash (a mismatch is already s.err)
        int rc = read_samples(b, s, out, verify_md5 && !s.md5_dev);  // InvalidChecksum at :279-280
        // (a left-justified stream: the verdict belongs to the samples before the shift)
        if (rc == E_INVALID_CHECKSUM && md5_before_justify(b, s)) rc = E_OK;
        return rc;
    });
}

int zflac_hip_batch_md5(zflac_batch* b, size_t i, uint8_t* digest) {
    if (!b || !b->ran || i >= b->streams.size() || !digest) return E_INVALID_ARGUMENT;
    const StreamState& s = b->streams[i];
    if (!s.md5_dev) return E_INVALID_ARGUMENT;
    std::memcpy(digest, s.md5_dig, 16);
    return E_OK;
}

int zflac_hip_batch_timings(zflac_batch* b, zflac_timings* t) {
    return zflac_hip_batch_timings_ex(b, t, ZFLAC_TIMINGS_V1_SIZE);
}

int zflac_hip_batch_timings_ex(zflac_batch* b, zflac_timings* t, size_t size) {
    if (!b || !t || size == 0) return E_INVALID_ARGUMENT;
    // the caller's struct may be older (shorter) or newer (longer) than this library's
    std::memcpy(t, &b->timings, std::min(size, sizeof(zflac_timings)));
    if (size > sizeof(zflac_timings)) std::memset(reinterpret_cast<uint8_t*>(t) + sizeof(zflac_timings), 0,
                                                  size - sizeof(zflac_timings));
    return b->have_timing ? E_OK : E_INVALID_ARGUMENT;  // the host wall-clock fields are always filled
}

int zflac_hip_abi_version(void) { return ZFLAC_HIP_ABI_VERSION; }

int zflac_hip_batch_export(zflac_batch* b, const zflac_export_desc* d, void* dst_device, size_t dst_bytes,
                           uint64_t* valid_frames, void* stream) {
    return export_dense(b, export_call(d), nullptr, dst_device, dst_bytes, valid_frames, stream);
}

int zflac_hip_batch_export_mixed(zflac_batch* b, const zflac_export_desc* d, const zflac_mix_desc* mix,
                                 void* dst_device, size_t dst_bytes, uint64_t* valid_frames, void* stream) {
    return export_dense(b, export_call(d), mix, dst_device, dst_bytes, valid_frames, stream);
}

uint64_t zflac_hip_resampled_frames(uint64_t n_frames, uint32_t rate_in, uint32_t rate_out) {
    return resampled_frames(n_frames, rate_in, rate_out);
}

int zflac_hip_batch_export_resampled(zflac_batch* b, const zflac_resample_desc* d, void* dst_device, size_t dst_bytes,
                                     uint64_t* valid_frames, void* stream) {
    return export_dense(b, export_call(d), nullptr, dst_device, dst_bytes, valid_frames, stream);
}

int zflac_hip_batch_export_resampled_mixed(zflac_batch* b, const zflac_resample_desc* d, const zflac_mix_desc* mix,
                                           void* dst_device, size_t dst_bytes, uint64_t* valid_frames, void* stream) {
    return export_dense(b, export_call(d), mix, dst_device, dst_bytes, valid_frames, stream);
}

int zflac_hip_mel_create(const zflac_mel_desc* d, int device, zflac_mel** out) {
    return mel_create(d, ZFLAC_MEL_MATH_F32, device, out);
}

int zflac_hip_mel_create_ex(const zflac_mel_desc* d, uint32_t math, int device, zflac_mel** out) {
    return mel_create(d, math, device, out);
}

int zflac_hip_mel_math(const zflac_mel* m) { return mel_math(m); }

int zflac_hip_mel_create_framed(const zflac_mel_desc* d, const zflac_mel_frame_desc* f, uint32_t math, int device,
                                zflac_mel** out) {
    return mel_create_framed(d, f, math, device, out);
}

uint64_t zflac_hip_mel_plan_frames(const zflac_mel* m, uint64_t n_samples) { return mel_plan_frames_of(m, n_samples); }

int zflac_hip_mel_cmvn(zflac_mel* m, const zflac_mel_cmvn_desc* c, void* stream) { return mel_cmvn(m, c, stream); }

int zflac_hip_mel_run(zflac_mel* m, const float* wave_device, uint64_t rows, uint64_t wave_frames, uint64_t row_stride,
                      uint64_t first_frame, uint64_t frames, void* dst_device, size_t dst_bytes, void* stream) {
    return mel_run(m, wave_device, rows, wave_frames, row_stride, first_frame, frames, dst_device, dst_bytes, stream);
}

int zflac_hip_mel_run_ex(zflac_mel* m, const zflac_mel_run_desc* r, void* stream) { return mel_run_ex(m, r, stream); }

uint64_t zflac_hip_mel_frames(uint64_t n_samples, uint32_t n_fft, uint32_t hop, int center) {
    return mel_frames(n_samples, n_fft, hop, center);
}

void zflac_hip_mel_destroy(zflac_mel* m) { mel_destroy(m); }

int zflac_hip_cepstra_create(const zflac_cepstra_desc* d, int device, zflac_cepstra** out) {
    return cepstra_create(d, device, out);
}

void zflac_hip_cepstra_destroy(zflac_cepstra* p) { cepstra_destroy(p); }

uint32_t zflac_hip_cepstra_features(const zflac_cepstra* p) { return cepstra_features(p); }

int zflac_hip_cepstra_delta_scales(const zflac_cepstra* p, uint32_t order, float* out, uint32_t cap) {
    return cepstra_delta_scales_of(p, order, out, cap);
}

int zflac_hip_cepstra_project(zflac_cepstra* p, const zflac_cepstra_project_desc* r, void* stream) {
    return cepstra_project(p, r, stream);
}

int zflac_hip_cepstra_cmvn(zflac_cepstra* p, const zflac_mel_cmvn_desc* c, void* stream) { return cepstra_cmvn(p, c, stream); }

int zflac_hip_cepstra_deltas(zflac_cepstra* p, const zflac_cepstra_delta_desc* r, void* stream) {
    return cepstra_deltas(p, r, stream);
}

int zflac_hip_batch_resample_tables(zflac_batch* b, uint64_t* built, uint64_t* held_floats) {
    if (!b) return E_INVALID_ARGUMENT;
    if (built) *built = b->rs_built;
    if (held_floats) {
        *held_floats = 0;
        for (auto& t : b->rs_tables) *held_floats += t->ratio.table_floats();
    }
    return E_OK;
}

static_assert(ZFLAC_BUCKET_8 == bucket_bit(8, false) && ZFLAC_BUCKET_4 == bucket_bit(4, false) &&
                  ZFLAC_BUCKET_16 == bucket_bit(16, false) && ZFLAC_BUCKET_32 == bucket_bit(32, false) &&
                  ZFLAC_BUCKET_MIX_8 == bucket_bit(8, true) && ZFLAC_BUCKET_MIX_32 == bucket_bit(32, true) &&
                  ZFLAC_BUCKET_12 == bucket_bit(12, false) && ZFLAC_BUCKET_ALL == BUCKET_MASK_ALL,
              "ZFLAC_BUCKET_* (zflac_hip.h) and bucket_bit() (common.h) disagree");

int zflac_hip_batch_decode_buckets(zflac_batch* b, uint32_t* used, uint32_t* planned) {
    if (!b || !used || !planned || !b->ran || b->submitted) return E_INVALID_ARGUMENT;
    *used = b->buckets_used;
    *planned = b->buckets_planned;
    return E_OK;
}

static_assert(ZFLAC_FRONT_SCAN == FRONT_SCAN && ZFLAC_FRONT_HOP == FRONT_HOP,
              "ZFLAC_FRONT_* (zflac_hip.h) and Front (stream_plan.h) disagree");

int zflac_hip_batch_front(zflac_batch* b, int* planned, int* used) {
    if (!b || !planned || !used || !b->ran || b->submitted) return E_INVALID_ARGUMENT;
    *planned = b->front_planned;
    *used = b->front_used;
    return E_OK;
}

static_assert(ZFLAC_MD5_K_COOP == MD5_K_COOP && ZFLAC_MD5_K_MULTI == MD5_K_MULTI && ZFLAC_MD5_K_LANE == MD5_K_LANE,
              "ZFLAC_MD5_K_* (zflac_hip.h) and Md5Kernel (common.h) disagree");

int zflac_hip_batch_md5_source(zflac_batch* b, size_t i, int* source) {
    if (!b || !b->ran || i >= b->streams.size() || !source) return E_INVALID_ARGUMENT;
    const StreamState& s = b->streams[i];
    *source = (s.err || !s.md5_dev) ? ZFLAC_MD5_SRC_NONE : s.md5_src;
    return E_OK;
}

int zflac_hip_batch_md5_stats(zflac_batch* b, uint32_t* kernels, uint64_t* rechecks) {
    if (!b || !kernels || !rechecks || !b->ran || b->submitted) return E_INVALID_ARGUMENT;
    *kernels = b->md5_kernels;
    *rechecks = b->md5_rechecks;
    return E_OK;
}

int zflac_hip_batch_export_ms(zflac_batch* b, double* ms) {
    if (!b || !ms || b->export_ms < 0) return E_INVALID_ARGUMENT;
    *ms = b->export_ms;
    return E_OK;
}

#ifdef ZFLAC_PROBE
// Timing-probe build only (tools/probe.py, run through tools/gpu.sh probe): cycle counters the
// decode kernels accumulate behind the dummy store region of the first class; zeroed after reading.
extern "C" int zflac_hip_probe(zflac_batch* b, unsigned long long* out, int n) {
    if (!b || b->classes.empty() || n > (int)(PROBE_BYTES / 8)) return E_INVALID_ARGUMENT;
    auto& C = *b->classes[0];
    uint8_t* p = reinterpret_cast<uint8_t*>(C.dummy.p) + DUMMY_BYTES;
    if (hipMemcpy(out, p, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return E_DEVICE;
    if (hipMemset(p, 0, PROBE_BYTES) != hipSuccess) return E_DEVICE;
    return E_OK;
}
#endif

#ifdef ZFLAC_REPLAY
// Diagnostic build only (tools/replay.py): re-enqueue parts of each batch's last run `reps`
// times, batch i on its own run stream, with no host work in between, and return the wall
// time: what = 1 walk, 2 decode, 3 walk + decode, 4 the whole run (enqueue_class: fills, scan,
// compact, walk, decode, verify, read-backs). Separates the device's throughput for each part
// from the host side of submit / wait. Outputs are rewritten with the same values.
extern "C" int zflac_hip_replay(zflac_batch** bs, int nb, int reps, int what, double* ms) {
    try {
        if (nb <= 0 || !bs || !ms) return E_INVALID_ARGUMENT;
        ck(hipSetDevice(bs[0]->device));
        for (int i = 0; i < nb; i++) {  // one run stream (hardware queue) per batch, as submit
            ck(hipStreamSynchronize(bs[i]->rs));
            bs[i]->rs = next_run_stream(bs[i]->device);
        }
        const double t0 = now_ms();
        for (int r = 0; r < reps; r++) {
            for (int i = 0; i < nb; i++) {
                zflac_batch* b = bs[i];
                Class& C = *b->classes[0];
                if (what == 4) {
                    enqueue_class(b, C, false, false);
                    continue;
                }
                if (what >= 8 && C.front == FRONT_HOP) {  // the front alone: k_hop
                    ck(launch_hop(hop_args(C), b->rs));
                    continue;
                }
                if (what >= 8) {  // the front alone: 8 k_scan, 16 k_scan + k_scan_chunks + k_compact
                    const ScanArgs sa = scan_args(C);
                    ck(launch_scan(sa, b->rs));
                    if (what == 16) {
                        ck(launch_scan_chunks(C.chunk_cnt.p, C.chunk_units.p, sa.n_chunks, C.chunk_off.p,
                                              C.chunk_uoff.p, C.misc.p, b->rs));
                        ck(launch_compact(compact_args(C), b->rs));
                    }
                    continue;
                }
                DecodeArgs da = decode_args(C);
                da.full_mask = C.full_mask;
                const uint32_t mf = std::min(C.grid_frames, C.cap);
                if (what & 1) ck(launch_walk_k1(da, mf, b->rs));
                if (what & 2) ck(launch_decode_k1_stereo(da, mf, b->rs));
            }
        }
        for (int i = 0; i < nb; i++) ck(hipStreamSynchronize(bs[i]->rs));
        *ms = now_ms() - t0;
        for (int i = 0; i < nb; i++) bs[i]->rs = bs[i]->stream;
        return E_OK;
    } catch (const DeviceError&) {
        return E_DEVICE;
    }
}
#endif

void zflac_hip_batch_destroy(zflac_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    delete b;
}

int zflac_hip_open(const uint8_t* buf, size_t len, int device, zflac_batch** out_batch, zflac_info* info) {
    return zflac_hip_open_ex(buf, len, device, 0, out_batch, info);
}

int zflac_hip_open_ex(const uint8_t* buf, size_t len, int device, int flags, zflac_batch** out_batch,
                      zflac_info* info) {
    if (!out_batch) return E_INVALID_ARGUMENT;
    zflac_stream s{buf, len};
    int rc = create_batch(&s, 1, device, flags, out_batch);
    if (rc) return rc;
    rc = zflac_hip_batch_run(*out_batch);
    if (rc) return rc;
    return zflac_hip_batch_info(*out_batch, 0, info);
}

int zflac_hip_read(zflac_batch* b, void* out_samples, size_t out_bytes) {
    return zflac_hip_batch_read(b, 0, out_samples, out_bytes, 1);
}

void zflac_hip_close(zflac_batch* b) { zflac_hip_batch_destroy(b); }

}  // extern "C"
