// abi.cpp -- the extern "C" ABI of include/zflac_hip.h over the host units (batch.h), the
// batch's destructor, the build id, and the entry points of the diagnostic builds.
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "batch.h"
#include "launch.h"

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

// ---- dense export: what zflac_hip_batch_export and zflac_hip_batch_export_resampled share ----
namespace {

struct ExportShape {
    size_t n;
    uint64_t T, C, esz, tiles;
    uint32_t vec;
};

// the checks both exports make, in the plain export's order (max_dtype: the last dtype the call takes)
bool export_shape(zflac_batch* b, uint32_t size, uint32_t want_size, int dtype, int max_dtype, int layout,
                  uint64_t channels, uint64_t frames, const void* dst, size_t dst_bytes, ExportShape& s) {
    if (!b || !dst || size != want_size) return false;
    if (dtype > max_dtype || layout > ZFLAC_LAYOUT_INTERLEAVED || !channels || !frames) return false;
    if (!b->ran || b->submitted) return false;
    s.n = b->streams.size();
    s.T = frames;
    s.C = channels;
    s.esz = (dtype == ZFLAC_EXPORT_F16 || dtype == ZFLAC_EXPORT_BF16) ? 2 : 4;
    const unsigned __int128 need = (unsigned __int128)s.n * s.C * s.T * s.esz;  // < 2^64 * 2^16 * 2^64 * 4
    if (need > (unsigned __int128)dst_bytes) return false;
    s.tiles = (s.T + EXPORT_TILE - 1) / EXPORT_TILE;
    if ((unsigned __int128)s.n * s.tiles > 0x7FFFFFFFull) return false;  // gridDim.x
    const uint64_t row_bytes = (layout == ZFLAC_LAYOUT_PLANAR ? s.T : s.T * s.C) * s.esz;
    s.vec = (reinterpret_cast<uintptr_t>(dst) % 16 == 0 && row_bytes % 16 == 0) ? 1u : 0u;
    return true;
}

// stream i as k_export's row record; r.src stays null unless the stream has frames from `start` on
ExportRow export_row(const StreamState& s, uint64_t start) {
    ExportRow r;
    std::memset(&r, 0, sizeof(r));
    r.start = start;
    r.kind = s.info.sample_kind;
    if (!s.err && s.info.channels && s.dev_samples) {
        r.nch = s.info.channels;
        r.n_frames = s.info.n_samples / s.info.channels;
        if (r.start < r.n_frames) r.src = s.dev_samples;
    }
    return r;
}

// The matrices of a mixed export, checked and laid out as the kernels read them: at[n] is where
// the C x n matrix of the n-channel streams starts in `table` (0: none, the fit rule), table[0] is
// unused. any: the call has a matrix and launches the mixed kernel.
struct MixPlan {
    bool any = false;
    uint16_t at[MIX_MAX_CH + 1] = {};
    std::vector<float> table;
};

// zflac_mix_desc's rules (mix may be NULL). Every non-NULL matrix is read here, so the caller may
// free it when the call returns.
bool mix_plan(const zflac_mix_desc* mix, int dtype, uint64_t channels, MixPlan& p) {
    if (!mix) return true;
    if (mix->size != sizeof(zflac_mix_desc) || mix->reserved) return false;
    static_assert(ZFLAC_MIX_MAX_CHANNELS == MIX_MAX_CH, "zflac_hip.h and common.h disagree");
    for (uint32_t n = 1; n <= MIX_MAX_CH; n++) {
        const float* m = mix->matrix[n - 1];
        if (!m) continue;
        if (dtype == ZFLAC_EXPORT_I32 || channels > MIX_MAX_CH) return false;
        if (!p.any) p.table.assign(1, 0.0f);
        p.any = true;
        p.at[n] = (uint16_t)p.table.size();
        for (uint64_t i = 0; i < channels * n; i++) {
            const float a = std::fabs(m[i]);  // (NaN fails the range test)
            if (a != 0.0f && !(a >= 0x1p-64f && a <= 0x1p64f)) return false;
            p.table.push_back(a == 0.0f ? 0.0f : m[i]);
        }
    }
    return true;
}

// ExportRow::mix of a stream of nch channels
uint16_t mix_at(const MixPlan& p, uint32_t nch) { return nch <= MIX_MAX_CH ? p.at[nch] : 0; }

// bytes of n row records with the coefficient table behind them (16-byte aligned)
size_t mix_table_offset(size_t row_bytes) { return (row_bytes + 15) & ~(size_t)15; }

// Before the row records are written: the buffers exist and the last export has let go of them.
// Returns whether this export is timed.
bool export_begin(zflac_batch* b, size_t n, void* stream, hipStream_t st) {
    if (!b->exp_pin) {
        // room for the larger record and for a mixed export's coefficient table behind the records
        const size_t bytes = mix_table_offset(n * sizeof(ResampleRow)) + MIX_TABLE_FLOATS * sizeof(float);
        ck(hipHostMalloc(reinterpret_cast<void**>(&b->exp_pin), bytes, hipHostMallocDefault));
        b->exp_rows.alloc(bytes);
        ck(hipEventCreateWithFlags(&b->ev_exp_copy, hipEventDisableTiming));
        ck(hipEventCreateWithFlags(&b->ev_exp, hipEventDisableTiming));
    }
    if (b->exp_any) {
        ck(hipEventSynchronize(b->ev_exp_copy));     // the last export's copy has read exp_pin
        ck(hipStreamWaitEvent(st, b->ev_exp, 0));    // and its kernel exp_rows, before this copy lands
    }
    const bool timed = !stream && (b->flags & ZFLAC_FLAG_TIMING);
    if (timed)
        for (auto& e : b->ev_exp_t)
            if (!e) ck(hipEventCreate(&e));
    return timed;
}

// After the row records (row_bytes of them) are in exp_pin: the coefficient table goes behind
// them, so that one copy takes both. Returns the table's device address (null without a matrix)
// and grows `bytes`, what export_run copies.
const float* mix_stage(zflac_batch* b, const MixPlan& p, size_t row_bytes, size_t& bytes) {
    bytes = row_bytes;
    if (!p.any) return nullptr;
    const size_t at = mix_table_offset(row_bytes);
    std::memset(b->exp_pin + row_bytes, 0, at - row_bytes);
    std::memcpy(b->exp_pin + at, p.table.data(), p.table.size() * sizeof(float));
    bytes = at + p.table.size() * sizeof(float);
    return reinterpret_cast<const float*>(b->exp_rows.p + at);
}

// The records are in exp_pin: copy them, launch, and finish as the caller's stream asks.
template <typename Launch>
void export_run(zflac_batch* b, size_t bytes, bool timed, void* stream, hipStream_t st, Launch launch) {
    if (timed) ck(hipEventRecord(b->ev_exp_t[0], st));
    ck(hipMemcpyAsync(b->exp_rows.p, b->exp_pin, bytes, hipMemcpyHostToDevice, st));
    ck(hipEventRecord(b->ev_exp_copy, st));
    const hipError_t le = launch();
    ck(hipEventRecord(b->ev_exp, st));  // (also after a failed launch: the copy above is enqueued)
    b->exp_any = true;
    ck(le);
    if (timed) ck(hipEventRecord(b->ev_exp_t[1], st));
    if (stream) {
        b->exp_pending = true;
    } else {
        ck(hipStreamSynchronize(st));
        if (timed) {
            float ms = 0;
            ck(hipEventElapsedTime(&ms, b->ev_exp_t[0], b->ev_exp_t[1]));
            b->export_ms = ms;
        }
    }
}

// The batch's table for these parameters: the one it holds, or a new one (built on the host,
// uploaded before this returns).
ResampleTable* resample_table(zflac_batch* b, uint32_t fin, const zflac_resample_desc* d, const ResampleRatio& ratio) {
    for (auto& t : b->rs_tables)
        if (t->fin == fin && t->fout == d->sample_rate && t->zeros == d->zeros && t->rolloff == d->rolloff &&
            t->beta == d->beta)
            return t.get();
    auto t = std::make_unique<ResampleTable>();
    t->fin = fin;
    t->fout = d->sample_rate;
    t->zeros = d->zeros;
    t->rolloff = d->rolloff;
    t->beta = d->beta;
    t->ratio = ratio;
    std::vector<float> h;
    resample_taps(ratio, d->zeros, d->beta, h);
    t->taps.alloc(h.size());
    ck(hipMemcpy(t->taps.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    b->rs_built++;
    b->rs_tables.push_back(std::move(t));
    return b->rs_tables.back().get();
}

}  // namespace

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
    try {
        b->submit_t0 = now_ms();
        b->submitted = true;
        submit_batch(b);
    } catch (const DeviceError&) {
        drain_failed_submit(b);
        return E_DEVICE;
    } catch (const std::bad_alloc&) {
        drain_failed_submit(b);
        return E_OUT_OF_MEMORY;
    } catch (const std::exception&) {
        drain_failed_submit(b);
        return E_DEVICE;
    }
    return E_OK;
}

int zflac_hip_batch_wait(zflac_batch* b) {
    if (!b || !b->submitted) return E_INVALID_ARGUMENT;
    b->submitted = false;
    int rc = E_OK;
    try {
        finish_batch(b);
        b->timings.run_wall_ms = now_ms() - b->submit_t0;
        b->ran = true;
    } catch (const DeviceError&) {
        rc = E_DEVICE;
    } catch (const std::bad_alloc&) {
        rc = E_OUT_OF_MEMORY;
    } catch (const std::exception&) {
        rc = E_DEVICE;
    }
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
    try {
        ck(hipSetDevice(b->device));
        // a device verdict stands in for the host hash (a mismatch is already s.err)
        return read_samples(b, s, out, verify_md5 && !s.md5_dev);  // InvalidChecksum at :279-280
    } catch (const DeviceError&) {
        return E_DEVICE;
    } catch (const std::exception&) {  // std::system_error: the hashing thread could not start
        return E_DEVICE;
    }
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

// zflac_hip_batch_export (mix == NULL) and zflac_hip_batch_export_mixed
static int export_plain(zflac_batch* b, const zflac_export_desc* d, const zflac_mix_desc* mix, void* dst_device,
                        size_t dst_bytes, uint64_t* valid_frames, void* stream) {
    ExportShape s;
    MixPlan mp;
    if (!d || !export_shape(b, d->size, sizeof(zflac_export_desc), d->dtype, ZFLAC_EXPORT_I32, d->layout, d->channels,
                            d->frames, dst_device, dst_bytes, s))
        return E_INVALID_ARGUMENT;
    try {
        if (!mix_plan(mix, d->dtype, s.C, mp)) return E_INVALID_ARGUMENT;
    } catch (const std::bad_alloc&) {
        return E_OUT_OF_MEMORY;
    }
    const size_t n = s.n;
    for (size_t i = 0; valid_frames && i < n; i++) {
        const StreamState& st = b->streams[i];
        const uint64_t start = d->starts ? d->starts[i] : 0;
        const uint64_t nf = (st.err || !st.info.channels) ? 0 : st.info.n_samples / st.info.channels;
        valid_frames[i] = nf > start ? std::min(nf - start, s.T) : 0;
    }
    if (n == 0) return E_OK;
    try {
        DeviceScope scope(b->device);
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : b->stream;
        const bool timed = export_begin(b, n, stream, st);
        ExportRow* rows = reinterpret_cast<ExportRow*>(b->exp_pin);
        for (size_t i = 0; i < n; i++) {
            rows[i] = export_row(b->streams[i], d->starts ? d->starts[i] : 0);
            rows[i].mix = mix_at(mp, rows[i].nch);
        }
        size_t bytes;
        const float* coef = mix_stage(b, mp, n * sizeof(ExportRow), bytes);
        ExportArgs a;
        std::memset(&a, 0, sizeof(a));
        a.rows = reinterpret_cast<const ExportRow*>(b->exp_rows.p);
        a.dst = dst_device;
        a.frames = s.T;
        a.channels = (uint32_t)s.C;
        a.n_rows = (uint32_t)n;
        a.tiles = (uint32_t)s.tiles;
        a.vec = s.vec;
        export_run(b, bytes, timed, stream, st, [&] {  // without a matrix: k_export, as ever
            return coef ? launch_export_mixed(d->dtype, d->layout, a, coef, st) : launch_export(d->dtype, d->layout, a, st);
        });
    } catch (const DeviceError&) {
        return E_DEVICE;
    } catch (const std::bad_alloc&) {
        return E_OUT_OF_MEMORY;
    }
    return E_OK;
}

int zflac_hip_batch_export(zflac_batch* b, const zflac_export_desc* d, void* dst_device, size_t dst_bytes,
                           uint64_t* valid_frames, void* stream) {
    return export_plain(b, d, nullptr, dst_device, dst_bytes, valid_frames, stream);
}

int zflac_hip_batch_export_mixed(zflac_batch* b, const zflac_export_desc* d, const zflac_mix_desc* mix,
                                 void* dst_device, size_t dst_bytes, uint64_t* valid_frames, void* stream) {
    return export_plain(b, d, mix, dst_device, dst_bytes, valid_frames, stream);
}

uint64_t zflac_hip_resampled_frames(uint64_t n_frames, uint32_t rate_in, uint32_t rate_out) {
    return resampled_frames(n_frames, rate_in, rate_out);
}

// zflac_hip_batch_export_resampled (mix == NULL) and zflac_hip_batch_export_resampled_mixed
static int export_resampled(zflac_batch* b, const zflac_resample_desc* d, const zflac_mix_desc* mix, void* dst_device,
                            size_t dst_bytes, uint64_t* valid_frames, void* stream) {
    ExportShape s;
    MixPlan mp;
    if (!d || !export_shape(b, d->size, sizeof(zflac_resample_desc), d->dtype, ZFLAC_EXPORT_BF16, d->layout,
                            d->channels, d->frames, dst_device, dst_bytes, s))
        return E_INVALID_ARGUMENT;
    if (!d->sample_rate || d->sample_rate > RESAMPLE_MAX_RATE || d->reserved ||
        !resample_params_ok(d->zeros, d->rolloff, d->beta))
        return E_INVALID_ARGUMENT;
    try {
        if (!mix_plan(mix, d->dtype, s.C, mp)) return E_INVALID_ARGUMENT;
    } catch (const std::bad_alloc&) {
        return E_OUT_OF_MEMORY;
    }
    // channels of stream `st` that k_resample stages: min(its own, C), or C when it is mixed first
    auto staged = [&](const StreamState& st) {
        return mix_at(mp, st.info.channels) ? s.C : std::min<uint64_t>(st.info.channels, s.C);
    };
    const size_t n = s.n;
    // What each row takes, before anything is written or enqueued. plan[i] < 0: k_export's
    // paths (same rate, error, rate 0); else the index of the row's ratio in `ratios`.
    struct Need {
        uint32_t fin;
        ResampleRatio ratio;
    };
    std::vector<Need> needs;
    std::vector<int> plan(n, -1);
    std::vector<uint64_t> n_out(n, 0);
    uint64_t floats = 0, tiles = s.tiles;
    try {
        for (size_t i = 0; i < n; i++) {
            const StreamState& st = b->streams[i];
            if (st.err || !st.info.channels || !st.info.sample_rate) continue;
            const uint64_t nf = st.info.n_samples / st.info.channels;
            const uint32_t fin = st.info.sample_rate;
            if (fin == d->sample_rate) {
                n_out[i] = nf;
                continue;
            }
            n_out[i] = resampled_frames(nf, fin, d->sample_rate);
            int k = 0;
            while (k < (int)needs.size() && needs[k].fin != fin) k++;
            if (k == (int)needs.size()) {
                Need nd;
                nd.fin = fin;
                if (!resample_ratio(fin, d->sample_rate, d->zeros, d->rolloff, nd.ratio)) return E_INVALID_ARGUMENT;
                if (nd.ratio.K > RESAMPLE_MAX_TAPS) return E_INVALID_ARGUMENT;
                floats += nd.ratio.table_floats();
                if (floats > RESAMPLE_MAX_TABLE_FLOATS) return E_INVALID_ARGUMENT;
                needs.push_back(nd);
            }
            plan[i] = k;
            const ResampleTile rt = resample_tile(needs[k].ratio, (uint32_t)staged(st));
            tiles = std::max(tiles, (s.T + rt.tile - 1) / rt.tile);
        }
    } catch (const std::bad_alloc&) {
        return E_OUT_OF_MEMORY;
    }
    if ((unsigned __int128)n * tiles > 0x7FFFFFFFull) return E_INVALID_ARGUMENT;  // gridDim.x
    for (size_t i = 0; valid_frames && i < n; i++) {
        const uint64_t start = d->starts ? d->starts[i] : 0;
        valid_frames[i] = n_out[i] > start ? std::min(n_out[i] - start, s.T) : 0;
    }
    if (n == 0) return E_OK;
    try {
        DeviceScope scope(b->device);
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : b->stream;
        // Tables this call needs and the batch does not hold. Were they to take the batch past the
        // limit, the tables this call does not need go first (hipFree waits for the device, so
        // for any earlier export that reads them).
        uint64_t held = 0;
        for (auto& t : b->rs_tables) held += t->ratio.table_floats();
        if (held + floats > RESAMPLE_MAX_TABLE_FLOATS) {
            std::erase_if(b->rs_tables, [&](const std::unique_ptr<ResampleTable>& t) {
                if (t->fout == d->sample_rate && t->zeros == d->zeros && t->rolloff == d->rolloff && t->beta == d->beta)
                    for (const Need& nd : needs)
                        if (nd.fin == t->fin) return false;
                return true;
            });
        }
        std::vector<const ResampleTable*> tabs;
        for (const Need& nd : needs) tabs.push_back(resample_table(b, nd.fin, d, nd.ratio));
        const bool timed = export_begin(b, n, stream, st);
        ResampleRow* rows = reinterpret_cast<ResampleRow*>(b->exp_pin);
        for (size_t i = 0; i < n; i++) {
            const StreamState& ss = b->streams[i];
            ResampleRow r;
            std::memset(&r, 0, sizeof(r));
            const uint64_t start = d->starts ? d->starts[i] : 0;
            if (plan[i] < 0) {
                r.e = export_row(ss, start);
                if (!n_out[i]) r.e.src = nullptr;  // a stream whose rate is 0: a zero row
            } else {
                const ResampleTable* t = tabs[plan[i]];
                const ResampleTile rt = resample_tile(t->ratio, (uint32_t)staged(ss));
                r.e = export_row(ss, 0);  // (src by the source's length ...)
                r.e.start = start;        // ... the window by the resampled stream's)
                r.n_out = n_out[i];
                if (r.e.src && start < r.n_out) {
                    r.taps = t->taps.p;
                    r.L = t->ratio.L;
                    r.M = t->ratio.M;
                    r.W = t->ratio.W;
                    r.K = (uint32_t)t->ratio.K;
                    r.tile = rt.tile;
                    r.cg = rt.cg;
                    r.tab_lds = rt.tab_lds;
                } else {
                    r.e.src = nullptr;  // no frames, or the window is past the end: a zero row
                }
            }
            r.e.mix = mix_at(mp, r.e.nch);
            rows[i] = r;
        }
        size_t bytes;
        const float* coef = mix_stage(b, mp, n * sizeof(ResampleRow), bytes);
        ResampleArgs a;
        std::memset(&a, 0, sizeof(a));
        a.rows = reinterpret_cast<const ResampleRow*>(b->exp_rows.p);
        a.dst = dst_device;
        a.frames = s.T;
        a.channels = (uint32_t)s.C;
        a.n_rows = (uint32_t)n;
        a.tiles = (uint32_t)tiles;
        a.vec = s.vec;
        export_run(b, bytes, timed, stream, st, [&] {  // without a matrix: k_resample, as ever
            return coef ? launch_resample_mixed(d->dtype, d->layout, a, coef, st)
                        : launch_resample(d->dtype, d->layout, a, st);
        });
    } catch (const DeviceError&) {
        return E_DEVICE;
    } catch (const std::bad_alloc&) {
        return E_OUT_OF_MEMORY;
    }
    return E_OK;
}

int zflac_hip_batch_export_resampled(zflac_batch* b, const zflac_resample_desc* d, void* dst_device, size_t dst_bytes,
                                     uint64_t* valid_frames, void* stream) {
    return export_resampled(b, d, nullptr, dst_device, dst_bytes, valid_frames, stream);
}

int zflac_hip_batch_export_resampled_mixed(zflac_batch* b, const zflac_resample_desc* d, const zflac_mix_desc* mix,
                                           void* dst_device, size_t dst_bytes, uint64_t* valid_frames, void* stream) {
    return export_resampled(b, d, mix, dst_device, dst_bytes, valid_frames, stream);
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
