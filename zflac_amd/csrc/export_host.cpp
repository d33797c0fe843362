// export_host.cpp -- the device half of the four dense exports: the stream views export_plan.cpp
// plans from, the pinned record buffer and its events, the batch's tap tables, the launch.
#include <cstring>

#include "batch.h"
#include "launch.h"

namespace zflac {

namespace {

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
const float* mix_stage(zflac_batch* b, const ExportPlan& p, size_t row_bytes, size_t& bytes) {
    bytes = row_bytes;
    if (!p.mixed) return nullptr;
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

bool table_is(const ResampleTable& t, uint32_t fin, const ExportCall& c) {
    return t.fin == fin && t.fout == c.sample_rate && t.zeros == c.zeros && t.rolloff == c.rolloff && t.beta == c.beta;
}

// The batch's table for these parameters: the one it holds, or a new one (built on the host,
// uploaded before this returns).
ResampleTable* resample_table(zflac_batch* b, uint32_t fin, const ExportCall& c, const ResampleRatio& ratio) {
    for (auto& t : b->rs_tables)
        if (table_is(*t, fin, c)) return t.get();
    auto t = std::make_unique<ResampleTable>();
    t->fin = fin;
    t->fout = c.sample_rate;
    t->zeros = c.zeros;
    t->rolloff = c.rolloff;
    t->beta = c.beta;
    t->ratio = ratio;
    std::vector<float> h;
    resample_taps(ratio, c.zeros, c.beta, h);
    t->taps.alloc(h.size());
    ck(hipMemcpy(t->taps.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    b->rs_built++;
    b->rs_tables.push_back(std::move(t));
    return b->rs_tables.back().get();
}

// The device tables of plan.needs, in that order. Were the ones the batch does not hold to take
// it past the limit, the tables this call does not need go first (hipFree waits for the device,
// so for any earlier export that reads them).
std::vector<const float*> resample_tables(zflac_batch* b, const ExportCall& c, const ExportPlan& p) {
    uint64_t held = 0;
    for (auto& t : b->rs_tables) held += t->ratio.table_floats();
    if (held + p.need_floats > RESAMPLE_MAX_TABLE_FLOATS) {
        std::erase_if(b->rs_tables, [&](const std::unique_ptr<ResampleTable>& t) {
            for (const ExportPlan::Need& nd : p.needs)
                if (table_is(*t, nd.fin, c)) return false;
            return true;
        });
    }
    std::vector<const float*> taps;
    for (const ExportPlan::Need& nd : p.needs) taps.push_back(resample_table(b, nd.fin, c, nd.ratio)->taps.p);
    return taps;
}

// What the planner sees of the batch's streams, in b->exp_views (kept: no allocation per call).
// Invariant relied on: a run that leaves a stream with err == 0 and channels != 0 has set its
// dev_samples (finish_batch, finish_stream_sequential), so folding a null dev_samples into "no
// samples" changes no valid length and no ratio the calls used to derive from err and channels alone.
const ExportStream* export_views(zflac_batch* b) {
    b->exp_views.resize(b->streams.size());
    for (size_t i = 0; i < b->streams.size(); i++) {
        const StreamState& s = b->streams[i];
        ExportStream v;
        v.kind = s.info.sample_kind;
        if (!s.err && s.info.channels && s.dev_samples) {
            v.samples = s.dev_samples;
            v.nch = s.info.channels;
            v.n_frames = s.info.n_samples / s.info.channels;
            v.rate = s.info.sample_rate;
        }
        b->exp_views[i] = v;
    }
    return b->exp_views.data();
}

ExportArgs export_args(const zflac_batch* b, const ExportPlan& p, void* dst) {
    ExportArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rows = reinterpret_cast<const ExportRow*>(b->exp_rows.p);
    a.dst = dst;
    a.frames = p.T;
    a.channels = (uint32_t)p.C;
    a.n_rows = (uint32_t)p.n;
    a.tiles = (uint32_t)p.tiles;
    a.vec = p.vec;
    return a;
}

ResampleArgs resample_args(const zflac_batch* b, const ExportPlan& p, void* dst) {
    ResampleArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rows = reinterpret_cast<const ResampleRow*>(b->exp_rows.p);
    a.dst = dst;
    a.frames = p.T;
    a.channels = (uint32_t)p.C;
    a.n_rows = (uint32_t)p.n;
    a.tiles = (uint32_t)p.tiles;
    a.vec = p.vec;
    return a;
}

}  // namespace

int export_dense(zflac_batch* b, const ExportCall& c, const zflac_mix_desc* mix, void* dst, size_t dst_bytes,
                 uint64_t* valid_frames, void* stream) {
    if (!b || !b->ran || b->submitted) return E_INVALID_ARGUMENT;
    return guarded([&]() -> int {
        const ExportStream* views = export_views(b);
        ExportPlan p;
        const int rc = plan_export(views, b->streams.size(), c, mix, reinterpret_cast<uintptr_t>(dst), dst_bytes,
                                   valid_frames, p);
        if (rc || p.n == 0) return rc;
        DeviceScope scope(b->device);
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : b->stream;
        size_t bytes;
        if (c.resampled) {
            const std::vector<const float*> taps = resample_tables(b, c, p);
            const bool timed = export_begin(b, p.n, stream, st);
            write_resample_rows(p, views, taps.data(), reinterpret_cast<ResampleRow*>(b->exp_pin));
            const float* coef = mix_stage(b, p, p.n * sizeof(ResampleRow), bytes);
            const ResampleArgs a = resample_args(b, p, dst);
            export_run(b, bytes, timed, stream, st, [&] {  // without a matrix: k_resample, as ever
                return coef ? launch_resample_mixed(c.dtype, c.layout, a, coef, st)
                            : launch_resample(c.dtype, c.layout, a, st);
            });
        } else {
            const bool timed = export_begin(b, p.n, stream, st);
            write_export_rows(p, views, reinterpret_cast<ExportRow*>(b->exp_pin));
            const float* coef = mix_stage(b, p, p.n * sizeof(ExportRow), bytes);
            const ExportArgs a = export_args(b, p, dst);
            export_run(b, bytes, timed, stream, st, [&] {  // without a matrix: k_export, as ever
                return coef ? launch_export_mixed(c.dtype, c.layout, a, coef, st) : launch_export(c.dtype, c.layout, a, st);
            });
        }
        return E_OK;
    });
}

}  // namespace zflac
