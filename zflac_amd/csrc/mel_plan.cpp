// mel_plan.cpp -- see mel_plan.h. Plain C++: tests/c/mel_probe.cpp links this unit alone.
#include "mel_plan.h"

#include <cmath>
#include <cstring>

namespace zflac {

int mel_plan_create(const zflac_mel_desc* d, const void* out_ptr, MelPlan& p) {
    if (!d || !out_ptr) return E_INVALID_ARGUMENT;
    if (d->size != sizeof(zflac_mel_desc)) return E_INVALID_ARGUMENT;
    if (d->dtype != ZFLAC_EXPORT_F32 && d->dtype != ZFLAC_EXPORT_F16 && d->dtype != ZFLAC_EXPORT_BF16)
        return E_INVALID_ARGUMENT;
    if (d->layout != ZFLAC_MEL_BINS_FIRST && d->layout != ZFLAC_MEL_FRAMES_FIRST) return E_INVALID_ARGUMENT;
    if (d->scale != ZFLAC_MEL_POWER && d->scale != ZFLAC_MEL_LOG10 && d->scale != ZFLAC_MEL_LN) return E_INVALID_ARGUMENT;
    if (d->center > 1) return E_INVALID_ARGUMENT;
    if (d->n_fft < 2 || d->n_fft > MEL_MAX_FFT || (d->n_fft & 1)) return E_INVALID_ARGUMENT;
    if (d->hop < 1 || d->hop > d->n_fft) return E_INVALID_ARGUMENT;
    if (d->n_bins < 1 || d->n_bins > MEL_MAX_BINS) return E_INVALID_ARGUMENT;
    if (d->reserved != 0) return E_INVALID_ARGUMENT;
    if (d->scale == ZFLAC_MEL_POWER ? d->floor != 0.0f : !(std::isfinite(d->floor) && d->floor > 0.0f))
        return E_INVALID_ARGUMENT;
    if (!d->window || !d->filters) return E_INVALID_ARGUMENT;
    const uint32_t K = d->n_fft / 2u + 1;
    for (uint32_t n = 0; n < d->n_fft; n++)
        if (!std::isfinite(d->window[n])) return E_INVALID_ARGUMENT;
    for (size_t i = 0; i < (size_t)d->n_bins * K; i++)
        if (!std::isfinite(d->filters[i])) return E_INVALID_ARGUMENT;
    p.dtype = d->dtype;
    p.layout = d->layout;
    p.scale = d->scale;
    p.center = d->center;
    p.n_fft = d->n_fft;
    p.hop = d->hop;
    p.n_bins = d->n_bins;
    p.floor = d->floor;
    p.K = K;
    p.bin_tiles = (K + MEL_TILE - 1) / MEL_TILE;
    p.m_tiles = 1;
    while (p.m_tiles * MEL_TILE < p.n_bins) p.m_tiles *= 2;
    return E_OK;
}

int mel_plan_create_ex(const zflac_mel_desc* d, uint32_t math, const void* out_ptr, MelPlan& p) {
    const int rc = mel_plan_create(d, out_ptr, p);
    if (rc) return rc;
    if (math != ZFLAC_MEL_MATH_F32 && math != ZFLAC_MEL_MATH_BF16X6 && math != ZFLAC_MEL_MATH_BF16X3)
        return E_INVALID_ARGUMENT;
    p.math = math;
    if (math != ZFLAC_MEL_MATH_F32) {
        p.k_blocks = (p.n_fft + MEL_BF16_K - 1) / MEL_BF16_K;
        p.n_pieces = math == ZFLAC_MEL_MATH_BF16X6 ? 3 : 2;
    }
    return E_OK;
}

size_t mel_basis_index(const MelPlan& p, uint32_t n, uint32_t k, uint32_t im) {
    const size_t b = k / MEL_TILE, i = k % MEL_TILE, s = n / 2, h = n % 2;
    return (((b * (p.n_fft / 2) + s) * 2 + im) * 2 + h) * MEL_TILE + i;
}

size_t mel_filter_index(const MelPlan& p, uint32_t m, uint32_t k) {
    const size_t b = k / MEL_TILE, row = k % MEL_TILE, q = m / MEL_TILE;
    const size_t h = (row >> 2) & 1;                    // rows 4..7 of every eight sit in lanes 32..63
    const size_t r = (row & 3) + 4 * (row >> 3);        // mel_acc_row(r) + 4 h == row
    return ((b * 16 + r) * p.m_tiles + q) * 64 + 32 * h + m % MEL_TILE;
}

void mel_tables(const MelPlan& p, const float* window, const float* filters, std::vector<float>& basis,
                std::vector<float>& filt) {
    const uint32_t N = p.n_fft, K = p.K;
    basis.assign(p.basis_floats(), 0.0f);
    filt.assign(p.filter_floats(), 0.0f);
    std::vector<double> co(N), si(N);
    const double two_pi = 6.283185307179586476925286766559;
    for (uint32_t j = 0; j < N; j++) {
        co[j] = std::cos(two_pi * (double)j / (double)N);
        si[j] = (2 * j) % N == 0 ? 0.0 : std::sin(two_pi * (double)j / (double)N);  // s[.][0], s[.][N/2]: exactly 0
    }
    for (uint32_t n = 0; n < N; n++) {
        const double w = window[n];
        for (uint32_t k = 0; k < K; k++) {
            const uint32_t j = (uint32_t)(((uint64_t)n * k) % N);
            basis[mel_basis_index(p, n, k, 0)] = (float)(w * co[j]);
            basis[mel_basis_index(p, n, k, 1)] = (float)(-w * si[j]);
        }
    }
    for (uint32_t m = 0; m < p.n_bins; m++)
        for (uint32_t k = 0; k < K; k++) filt[mel_filter_index(p, m, k)] = filters[(size_t)m * K + k];
}

uint16_t mel_bf16_round(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

float mel_bf16_value(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}

void mel_bf16_split(float v, uint16_t h[3]) {
    for (int i = 0; i < 3; i++) {
        h[i] = mel_bf16_round(v);
        v -= mel_bf16_value(h[i]);  // exact: the rest has at most 24 - 8 (i + 1) significant bits
    }
}

size_t mel_bf16_basis_index(const MelPlan& p, uint32_t k, uint32_t n, uint32_t im, uint32_t piece) {
    const size_t b = k / MEL_TILE, i = k % MEL_TILE, kb = n / MEL_BF16_K, h = (n % MEL_BF16_K) / 8, j = n % 8;
    const size_t g = b / MEL_BF16_GROUP, bi = b % MEL_BF16_GROUP;
    const size_t rest = p.bin_tiles - g * MEL_BF16_GROUP, tg = rest < MEL_BF16_GROUP ? rest : MEL_BF16_GROUP;
    const size_t operand = ((g * MEL_BF16_GROUP * p.k_blocks + kb * tg + bi) * 2 + im) * p.n_pieces + piece;
    return (operand * 64 + 32 * h + i) * 8 + j;
}

void mel_bf16_tables(const MelPlan& p, const float* window, const float* filters, std::vector<uint16_t>& pieces,
                     std::vector<float>& filt) {
    std::vector<float> basis;
    mel_tables(p, window, filters, basis, filt);  // c and s as the f32 plan holds them
    pieces.assign(p.piece_elems(), 0);
    for (uint32_t n = 0; n < p.n_fft; n++)
        for (uint32_t k = 0; k < p.K; k++)
            for (uint32_t im = 0; im < 2; im++) {
                uint16_t h[3];
                mel_bf16_split(basis[mel_basis_index(p, n, k, im)], h);
                for (uint32_t i = 0; i < p.n_pieces; i++) pieces[mel_bf16_basis_index(p, k, n, im, i)] = h[i];
            }
}

int mel_plan_run(const MelPlan* p, uintptr_t wave, uint64_t rows, uint64_t wave_frames, uint64_t row_stride,
                 uint64_t first_frame, uint64_t frames, uintptr_t dst, size_t dst_bytes, MelGrid& g) {
    g = MelGrid{};
    if (!p || !wave || !dst) return E_INVALID_ARGUMENT;
    if (wave % sizeof(float)) return E_INVALID_ARGUMENT;
    if (row_stride < wave_frames) return E_INVALID_ARGUMENT;
    if (frames == 0) return E_INVALID_ARGUMENT;
    unsigned __int128 need = (unsigned __int128)rows * p->n_bins;
    need *= frames;
    need *= p->elem_size();
    if (need > (unsigned __int128)dst_bytes) return E_INVALID_ARGUMENT;
    // every sample index the kernel forms, t * hop - off + n with t < first_frame + frames, is a signed 64-bit value
    const unsigned __int128 last = ((unsigned __int128)first_frame + frames) * p->hop;
    if (last >> 63) return E_INVALID_ARGUMENT;
    // the element offsets into the waveform, (rows - 1) * row_stride + wave_frames, stay below 2^63 too
    if (rows && ((unsigned __int128)rows * row_stride) >> 61) return E_INVALID_ARGUMENT;
    const uint64_t tiles = (frames - 1) / MEL_FRAMES + 1;
    if (tiles > MEL_MAX_GRID || (unsigned __int128)rows * tiles > MEL_MAX_GRID) return E_INVALID_ARGUMENT;
    g.tiles = (uint32_t)tiles;
    g.blocks = rows * tiles;
    return E_OK;
}

int mel_plan_run_ex(const MelPlan* p, const zflac_mel_run_desc* r, MelGrid& g) {
    g = MelGrid{};
    if (!p || !r) return E_INVALID_ARGUMENT;
    if (r->size != sizeof(zflac_mel_run_desc)) return E_INVALID_ARGUMENT;
    if (r->pad != ZFLAC_PAD_ZEROS && r->pad != ZFLAC_PAD_REFLECT) return E_INVALID_ARGUMENT;
    if (r->norm != ZFLAC_NORM_NONE && r->norm != ZFLAC_NORM_ROW_MAX) return E_INVALID_ARGUMENT;
    if (r->reserved != 0) return E_INVALID_ARGUMENT;
    if (r->reserved2 != 0) return E_INVALID_ARGUMENT;
    MelGrid shared;
    const int rc = mel_plan_run(p, reinterpret_cast<uintptr_t>(r->wave_device), r->rows, r->wave_frames, r->row_stride,
                                r->first_frame, r->frames, reinterpret_cast<uintptr_t>(r->dst_device), r->dst_bytes, shared);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(r->lengths_device) % sizeof(uint64_t)) return E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(r->row_max_device) % sizeof(float)) return E_INVALID_ARGUMENT;
    if (r->pad == ZFLAC_PAD_REFLECT && !p->center) return E_INVALID_ARGUMENT;
    if (r->norm == ZFLAC_NORM_ROW_MAX) {
        if (!r->row_max_device) return E_INVALID_ARGUMENT;
        if (p->scale == ZFLAC_MEL_POWER) return E_INVALID_ARGUMENT;
        if (!(std::isfinite(r->range) && r->range >= 0.0f)) return E_INVALID_ARGUMENT;
        if (!std::isfinite(r->add)) return E_INVALID_ARGUMENT;
        if (!(std::isfinite(r->mul) && r->mul != 0.0f)) return E_INVALID_ARGUMENT;
    } else if (r->range != 0.0f || r->add != 0.0f || r->mul != 0.0f) {  // (a NaN is not 0)
        return E_INVALID_ARGUMENT;
    }
    g = shared;
    return E_OK;
}

bool mel_run_is_plain(const zflac_mel_run_desc& r) {
    return r.pad == ZFLAC_PAD_ZEROS && r.norm == ZFLAC_NORM_NONE && !r.lengths_device && !r.row_max_device;
}

uint64_t mel_frames(uint64_t n_samples, uint32_t n_fft, uint32_t hop, int center) {
    if (!hop) return 0;
    if (center) return n_samples ? n_samples / hop + 1 : 0;
    return n_samples >= n_fft ? (n_samples - n_fft) / hop + 1 : 0;
}

}  // namespace zflac
