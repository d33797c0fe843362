// export_plan.cpp -- the dense exports' host planning (export_plan.h). Plain C++, no HIP.
#include "export_plan.h"

#include <cmath>
#include <cstring>
#include <new>

namespace zflac {

static_assert(ZFLAC_MIX_MAX_CHANNELS == MIX_MAX_CH, "zflac_hip.h and common.h disagree");

namespace {

ExportCall call_of(uint32_t size, uint32_t want_size, int dtype, int max_dtype, int layout, uint64_t channels,
                   uint64_t frames, const uint64_t* starts) {
    ExportCall c;
    c.size = size;
    c.want_size = want_size;
    c.dtype = dtype;
    c.max_dtype = max_dtype;
    c.layout = layout;
    c.channels = channels;
    c.frames = frames;
    c.starts = starts;
    return c;
}

// zflac_mix_desc's rules (mix may be NULL)
bool plan_mix(const zflac_mix_desc* mix, int dtype, ExportPlan& p) {
    if (!mix) return true;
    if (mix->size != sizeof(zflac_mix_desc) || mix->reserved) return false;
    for (uint32_t n = 1; n <= MIX_MAX_CH; n++) {
        const float* m = mix->matrix[n - 1];
        if (!m) continue;
        if (dtype == ZFLAC_EXPORT_I32 || p.C > MIX_MAX_CH) return false;
        if (!p.mixed) p.table.assign(1, 0.0f);
        p.mixed = true;
        p.at[n] = (uint16_t)p.table.size();
        for (uint64_t i = 0; i < p.C * n; i++) {
            const float a = std::fabs(m[i]);  // (NaN fails the range test)
            if (a != 0.0f && !(a >= 0x1p-64f && a <= 0x1p64f)) return false;
            p.table.push_back(a == 0.0f ? 0.0f : m[i]);
        }
    }
    return true;
}

// What each row of the resampled call takes: its length, its ratio, and the grid its tile asks for.
bool plan_ratios(const ExportStream* streams, const ExportCall& c, ExportPlan& p) {
    p.ratio_of.assign(p.n, -1);
    p.n_out.assign(p.n, 0);
    for (size_t i = 0; i < p.n; i++) {
        const ExportStream& s = streams[i];
        if (!s.samples || !s.rate) continue;
        if (s.rate == c.sample_rate) {
            p.n_out[i] = s.n_frames;
            continue;
        }
        p.n_out[i] = resampled_frames(s.n_frames, s.rate, c.sample_rate);
        int k = 0;
        while (k < (int)p.needs.size() && p.needs[k].fin != s.rate) k++;
        if (k == (int)p.needs.size()) {
            ExportPlan::Need nd;
            nd.fin = s.rate;
            if (!resample_ratio(s.rate, c.sample_rate, c.zeros, c.rolloff, nd.ratio)) return false;
            if (nd.ratio.K > RESAMPLE_MAX_TAPS) return false;
            p.need_floats += nd.ratio.table_floats();
            if (p.need_floats > RESAMPLE_MAX_TABLE_FLOATS) return false;
            p.needs.push_back(nd);
        }
        p.ratio_of[i] = k;
        const ResampleTile rt = resample_tile(p.needs[k].ratio, p.staged(s));
        p.tiles = std::max(p.tiles, (p.T + rt.tile - 1) / rt.tile);
    }
    return (unsigned __int128)p.n * p.tiles <= 0x7FFFFFFFull;  // gridDim.x
}

// stream s as k_export's row record; r.src stays null unless the stream has frames from `start` on
ExportRow export_row(const ExportPlan& p, const ExportStream& s, uint64_t start) {
    ExportRow r;
    std::memset(&r, 0, sizeof(r));
    r.start = start;
    r.kind = s.kind;
    if (s.samples) {
        r.nch = s.nch;
        r.n_frames = s.n_frames;
        if (r.start < r.n_frames) r.src = s.samples;
    }
    r.mix = p.mix_at(r.nch);
    return r;
}

}  // namespace

ExportCall export_call(const zflac_export_desc* d) {
    if (!d) return ExportCall{};
    return call_of(d->size, sizeof(zflac_export_desc), d->dtype, ZFLAC_EXPORT_I32, d->layout, d->channels, d->frames,
                   d->starts);
}

ExportCall export_call(const zflac_resample_desc* d) {
    if (!d) return ExportCall{};
    ExportCall c = call_of(d->size, sizeof(zflac_resample_desc), d->dtype, ZFLAC_EXPORT_BF16, d->layout, d->channels,
                           d->frames, d->starts);
    c.resampled = true;
    c.sample_rate = d->sample_rate;
    c.zeros = d->zeros;
    c.reserved = d->reserved;
    c.rolloff = d->rolloff;
    c.beta = d->beta;
    return c;
}

int plan_export(const ExportStream* streams, size_t n, const ExportCall& c, const zflac_mix_desc* mix, uintptr_t dst,
                size_t dst_bytes, uint64_t* valid_frames, ExportPlan& p) {
    if (!dst || c.size != c.want_size) return E_INVALID_ARGUMENT;
    if (c.dtype > c.max_dtype || c.layout > ZFLAC_LAYOUT_INTERLEAVED || !c.channels || !c.frames)
        return E_INVALID_ARGUMENT;
    p.n = n;
    p.T = c.frames;
    p.C = c.channels;
    p.starts = c.starts;
    const uint64_t esz = (c.dtype == ZFLAC_EXPORT_F16 || c.dtype == ZFLAC_EXPORT_BF16) ? 2 : 4;
    const unsigned __int128 need = (unsigned __int128)n * p.C * p.T * esz;  // < 2^64 * 2^16 * 2^64 * 4
    if (need > (unsigned __int128)dst_bytes) return E_INVALID_ARGUMENT;
    p.tiles = (p.T + EXPORT_TILE - 1) / EXPORT_TILE;
    if ((unsigned __int128)n * p.tiles > 0x7FFFFFFFull) return E_INVALID_ARGUMENT;  // gridDim.x
    const uint64_t row_bytes = (c.layout == ZFLAC_LAYOUT_PLANAR ? p.T : p.T * p.C) * esz;
    p.vec = (dst % 16 == 0 && row_bytes % 16 == 0) ? 1u : 0u;
    if (c.resampled && (!c.sample_rate || c.sample_rate > RESAMPLE_MAX_RATE || c.reserved ||
                        !resample_params_ok(c.zeros, c.rolloff, c.beta)))
        return E_INVALID_ARGUMENT;
    try {
        if (!plan_mix(mix, c.dtype, p)) return E_INVALID_ARGUMENT;
        if (c.resampled && !plan_ratios(streams, c, p)) return E_INVALID_ARGUMENT;
    } catch (const std::bad_alloc&) {
        return E_OUT_OF_MEMORY;
    }
    for (size_t i = 0; valid_frames && i < n; i++) {
        const uint64_t start = p.starts ? p.starts[i] : 0;
        const uint64_t len = c.resampled ? p.n_out[i] : streams[i].n_frames;
        valid_frames[i] = len > start ? std::min(len - start, p.T) : 0;
    }
    return E_OK;
}

void write_export_rows(const ExportPlan& p, const ExportStream* streams, ExportRow* rows) {
    for (size_t i = 0; i < p.n; i++) rows[i] = export_row(p, streams[i], p.starts ? p.starts[i] : 0);
}

void write_resample_rows(const ExportPlan& p, const ExportStream* streams, const float* const* taps,
                         ResampleRow* rows) {
    for (size_t i = 0; i < p.n; i++) {
        const ExportStream& s = streams[i];
        ResampleRow r;
        std::memset(&r, 0, sizeof(r));
        const uint64_t start = p.starts ? p.starts[i] : 0;
        if (p.ratio_of[i] < 0) {
            r.e = export_row(p, s, start);
            if (!p.n_out[i]) r.e.src = nullptr;  // a stream whose rate is 0: a zero row
        } else {
            const ResampleRatio& ratio = p.needs[p.ratio_of[i]].ratio;
            const ResampleTile rt = resample_tile(ratio, p.staged(s));
            r.e = export_row(p, s, 0);  // (src by the source's length ...)
            r.e.start = start;          // ... the window by the resampled stream's)
            r.n_out = p.n_out[i];
            if (r.e.src && start < r.n_out) {
                r.taps = taps[p.ratio_of[i]];
                r.L = ratio.L;
                r.M = ratio.M;
                r.W = ratio.W;
                r.K = (uint32_t)ratio.K;
                r.tile = rt.tile;
                r.cg = rt.cg;
                r.tab_lds = rt.tab_lds;
            } else {
                r.e.src = nullptr;  // no frames, or the window is past the end: a zero row
            }
        }
        rows[i] = r;
    }
}

}  // namespace zflac
