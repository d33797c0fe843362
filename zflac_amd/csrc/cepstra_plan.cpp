// cepstra_plan.cpp -- see cepstra_plan.h
#include "cepstra_plan.h"

#include <cmath>

#include "mel_plan.h"

namespace zflac {

static bool float_dtype(uint8_t dt) { return dt == ZFLAC_EXPORT_F32 || dt == ZFLAC_EXPORT_F16 || dt == ZFLAC_EXPORT_BF16; }

int cepstra_plan_create(const zflac_cepstra_desc* d, const void* out_ptr, CepstraPlan& p) {
    if (!d || !out_ptr) return E_INVALID_ARGUMENT;
    if (d->size != sizeof(zflac_cepstra_desc)) return E_INVALID_ARGUMENT;
    if (!float_dtype(d->in_dtype) || !float_dtype(d->out_dtype)) return E_INVALID_ARGUMENT;
    if (d->layout != ZFLAC_MEL_BINS_FIRST && d->layout != ZFLAC_MEL_FRAMES_FIRST) return E_INVALID_ARGUMENT;
    if (d->delta_order > CEPS_MAX_ORDER) return E_INVALID_ARGUMENT;
    if (d->n_in < 1 || d->n_in > CEPS_MAX_DIM) return E_INVALID_ARGUMENT;
    if (d->n_out < 1 || d->n_out > CEPS_MAX_DIM) return E_INVALID_ARGUMENT;
    if (d->delta_order ? d->delta_window < 1 || d->delta_window > CEPS_MAX_WINDOW : d->delta_window != 0)
        return E_INVALID_ARGUMENT;
    if (d->reserved[0] || d->reserved[1] || d->reserved[2]) return E_INVALID_ARGUMENT;
    if (!d->matrix) {
        if (d->n_out != d->n_in) return E_INVALID_ARGUMENT;
        if (d->in_dtype != d->out_dtype) return E_INVALID_ARGUMENT;
        if (d->delta_order == 0) return E_INVALID_ARGUMENT;
    } else {
        const size_t n = (size_t)d->n_out * d->n_in;
        for (size_t i = 0; i < n; i++)
            if (!std::isfinite(d->matrix[i])) return E_INVALID_ARGUMENT;
    }
    p.in_dtype = d->in_dtype;
    p.out_dtype = d->out_dtype;
    p.layout = d->layout;
    p.has_matrix = d->matrix != nullptr;
    p.n_in = d->n_in;
    p.n_out = d->n_out;
    p.delta_order = d->delta_order;
    p.delta_window = d->delta_window;
    return E_OK;
}

std::vector<double> cepstra_delta_scales(uint32_t order, uint32_t window) {
    std::vector<double> s{1.0};
    if (order > CEPS_MAX_ORDER || window < 1 || window > CEPS_MAX_WINDOW) return order ? std::vector<double>{} : s;
    const int W = (int)window;
    double norm = 0.0;
    for (int j = -W; j <= W; j++) norm += (double)(j * j);
    for (uint32_t o = 1; o <= order; o++) {  // s_o[i + j] += s_{o-1}[i] * j / norm
        std::vector<double> next(s.size() + 2 * window, 0.0);
        for (size_t i = 0; i < s.size(); i++)
            for (int j = -W; j <= W; j++) next[i + (size_t)(j + W)] += s[i] * ((double)j / norm);
        s.swap(next);
    }
    return s;
}

uint32_t cepstra_scale_offset(uint32_t order, uint32_t window) {
    uint32_t off = 0;
    for (uint32_t o = 1; o < order; o++) off += 2 * o * window + 1;
    return off;
}

std::vector<float> cepstra_scale_table(uint32_t max_order, uint32_t window) {
    std::vector<float> t;
    for (uint32_t o = 1; o <= max_order; o++)
        for (double v : cepstra_delta_scales(o, window)) t.push_back((float)v);
    return t;
}

uint32_t cepstra_grid_blocks(uint64_t passes) { return passes < CEPS_MAX_GRID ? (uint32_t)passes : (uint32_t)CEPS_MAX_GRID; }

// rows * per_frame * frames * size in 63 bits
static bool fits63(uint64_t rows, uint64_t per_frame, uint64_t frames, uint64_t size) {
    unsigned __int128 b = (unsigned __int128)rows * per_frame;
    if (b >> 63) return false;
    b *= frames;
    if (b >> 63) return false;
    b *= size;
    return !(b >> 63);
}

int cepstra_plan_project(const CepstraPlan* p, const zflac_cepstra_project_desc* r, CepstraGrid& g) {
    g = CepstraGrid{};
    if (!p || !r) return E_INVALID_ARGUMENT;
    if (r->size != sizeof(zflac_cepstra_project_desc)) return E_INVALID_ARGUMENT;
    if (r->reserved != 0) return E_INVALID_ARGUMENT;
    if (!p->has_matrix) return E_INVALID_ARGUMENT;
    if (!r->src_device) return E_INVALID_ARGUMENT;
    if (!r->dst_device) return E_INVALID_ARGUMENT;
    if (r->src_device == r->dst_device) return E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(r->src_device) % p->in_size()) return E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(r->dst_device) % p->out_size()) return E_INVALID_ARGUMENT;
    if (r->frames == 0) return E_INVALID_ARGUMENT;
    if (!fits63(r->rows, p->n_in, r->frames, p->in_size())) return E_INVALID_ARGUMENT;
    if (!fits63(r->rows, p->n_out, r->frames, p->out_size())) return E_INVALID_ARGUMENT;
    g.tiles = (r->frames - 1) / CEPS_FRAMES + 1;
    g.passes = r->rows * g.tiles;
    g.blocks = cepstra_grid_blocks(g.passes);
    return E_OK;
}

int cepstra_plan_deltas(const CepstraPlan* p, const zflac_cepstra_delta_desc* r, CepstraGrid& g) {
    g = CepstraGrid{};
    if (!p || !r) return E_INVALID_ARGUMENT;
    if (r->size != sizeof(zflac_cepstra_delta_desc)) return E_INVALID_ARGUMENT;
    if (r->reserved != 0) return E_INVALID_ARGUMENT;
    if (r->reserved2 != 0) return E_INVALID_ARGUMENT;
    if (p->delta_order == 0) return E_INVALID_ARGUMENT;
    if (!r->src_device) return E_INVALID_ARGUMENT;
    if (!r->dst_device) return E_INVALID_ARGUMENT;
    if (r->src_device == r->dst_device) return E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(r->src_device) % p->out_size()) return E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(r->dst_device) % p->out_size()) return E_INVALID_ARGUMENT;
    if (r->frames == 0) return E_INVALID_ARGUMENT;
    if (!fits63(r->rows, (uint64_t)p->features(), r->frames, p->out_size())) return E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(r->valid_device) % sizeof(uint64_t)) return E_INVALID_ARGUMENT;
    if (!std::isfinite(r->pad_value)) return E_INVALID_ARGUMENT;
    if (p->layout == ZFLAC_MEL_BINS_FIRST) {
        g.tiles = (r->frames - 1) / CEPS_THREADS + 1;
        g.passes = r->rows * p->n_out * g.tiles;
    } else {
        g.tiles = (r->frames - 1) / (CEPS_THREADS / p->n_out) + 1;
        g.passes = r->rows * g.tiles;
    }
    g.blocks = cepstra_grid_blocks(g.passes);
    return E_OK;
}

int cepstra_plan_cmvn(const CepstraPlan* p, const zflac_mel_cmvn_desc* c, uint64_t& passes) {
    MelPlan carrier;  // what mel_plan_cmvn reads of a plan: the bin count, the dtype, the layout
    if (p) {
        carrier.n_bins = p->n_out;
        carrier.dtype = p->out_dtype;
        carrier.layout = p->layout;
    }
    return mel_plan_cmvn(p ? &carrier : nullptr, c, passes);
}

}  // namespace zflac
