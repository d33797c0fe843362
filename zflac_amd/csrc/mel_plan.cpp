// mel_plan.cpp -- see mel_plan.h. Plain C++: tests/c/mel_probe.cpp links this unit alone.
#include "mel_plan.h"

#include <cmath>
#include <cstring>

namespace zflac {

// mel_plan_create's checks up to and including floor
static int mel_check_scalars(const zflac_mel_desc* d, const void* out_ptr) {
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
    return E_OK;
}

// ... and the arrays: window (nw floats) and filters, NULL, then every value finite
static int mel_check_arrays(const zflac_mel_desc* d, uint32_t nw) {
    if (!d->window || !d->filters) return E_INVALID_ARGUMENT;
    const uint32_t K = d->n_fft / 2u + 1;
    for (uint32_t n = 0; n < nw; n++)
        if (!std::isfinite(d->window[n])) return E_INVALID_ARGUMENT;
    for (size_t i = 0; i < (size_t)d->n_bins * K; i++)
        if (!std::isfinite(d->filters[i])) return E_INVALID_ARGUMENT;
    return E_OK;
}

static void mel_plan_fill(const zflac_mel_desc* d, MelPlan& p) {
    const uint32_t K = d->n_fft / 2u + 1;
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
    p.win_length = p.span = p.n_fft;
    p.off = p.center ? (int32_t)(p.n_fft / 2) : 0;
}

int mel_plan_create(const zflac_mel_desc* d, const void* out_ptr, MelPlan& p) {
    int rc = mel_check_scalars(d, out_ptr);
    if (!rc) rc = mel_check_arrays(d, d->n_fft);
    if (rc) return rc;
    mel_plan_fill(d, p);
    return E_OK;
}

// math, the last check of both extended creates; the split plan's sample blocks follow the frame
static int mel_plan_math(uint32_t math, MelPlan& p) {
    if (math != ZFLAC_MEL_MATH_F32 && math != ZFLAC_MEL_MATH_BF16X6 && math != ZFLAC_MEL_MATH_BF16X3)
        return E_INVALID_ARGUMENT;
    p.math = math;
    if (math != ZFLAC_MEL_MATH_F32) {
        p.k_blocks = (p.win_length + MEL_BF16_K - 1) / MEL_BF16_K;
        p.n_pieces = math == ZFLAC_MEL_MATH_BF16X6 ? 3 : 2;
    }
    return E_OK;
}

int mel_plan_create_ex(const zflac_mel_desc* d, uint32_t math, const void* out_ptr, MelPlan& p) {
    const int rc = mel_plan_create(d, out_ptr, p);
    if (rc) return rc;
    return mel_plan_math(math, p);
}

int mel_plan_create_framed(const zflac_mel_desc* d, const zflac_mel_frame_desc* f, uint32_t math, const void* out_ptr,
                           MelPlan& p) {
    int rc = mel_check_scalars(d, out_ptr);
    if (rc) return rc;
    if (!f) return E_INVALID_ARGUMENT;
    if (f->size != sizeof(zflac_mel_frame_desc)) return E_INVALID_ARGUMENT;
    if (f->win_length < 1 || f->win_length > d->n_fft) return E_INVALID_ARGUMENT;
    if (f->framing != ZFLAC_FRAMING_STFT && f->framing != ZFLAC_FRAMING_SNIP && f->framing != ZFLAC_FRAMING_KALDI_CENTER)
        return E_INVALID_ARGUMENT;
    if (f->remove_dc > 1) return E_INVALID_ARGUMENT;
    if (!(std::isfinite(f->preemphasis) && f->preemphasis >= 0.0f && f->preemphasis <= 1.0f)) return E_INVALID_ARGUMENT;
    const float ag = std::fabs(f->sample_scale);
    if (!(std::isfinite(ag) && ag >= 0x1p-64f && ag <= 0x1p64f)) return E_INVALID_ARGUMENT;
    if (f->reserved != 0) return E_INVALID_ARGUMENT;
    rc = mel_check_arrays(d, f->win_length);
    if (rc) return rc;
    if (f->framing != ZFLAC_FRAMING_STFT && d->center) return E_INVALID_ARGUMENT;
    if (d->hop > f->win_length) return E_INVALID_ARGUMENT;
    MelPlan q;
    mel_plan_fill(d, q);
    const uint32_t N = q.n_fft, Nw = f->win_length;
    q.win_length = Nw;
    q.span = Nw + (Nw & 1);
    q.framing = f->framing;
    q.remove_dc = f->remove_dc;
    q.preemphasis = f->preemphasis;
    q.sample_scale = f->sample_scale;
    if (f->framing == ZFLAC_FRAMING_STFT) q.off = (int32_t)(q.center ? N / 2 : 0) - (int32_t)((N - Nw) / 2);
    else if (f->framing == ZFLAC_FRAMING_SNIP) q.off = 0;
    else q.off = (int32_t)(Nw / 2) - (int32_t)(q.hop / 2);
    rc = mel_plan_math(math, q);
    if (rc) return rc;
    p = q;
    return E_OK;
}

size_t mel_basis_index(const MelPlan& p, uint32_t n, uint32_t k, uint32_t im) {
    const size_t b = k / MEL_TILE, i = k % MEL_TILE, s = n / 2, h = n % 2;
    return (((b * (p.span / 2) + s) * 2 + im) * 2 + h) * MEL_TILE + i;
}

size_t mel_filter_index(const MelPlan& p, uint32_t m, uint32_t k) {
    const size_t b = k / MEL_TILE, row = k % MEL_TILE, q = m / MEL_TILE;
    const size_t h = (row >> 2) & 1;                    // rows 4..7 of every eight sit in lanes 32..63
    size_t r = 0;                                       // the register: mel_acc_row(r) + 4 h == row
    while (mel_acc_row((uint32_t)r) + 4 * h != row) r++;
    return ((b * 16 + r) * p.m_tiles + q) * 64 + 32 * h + m % MEL_TILE;
}

void mel_tables(const MelPlan& p, const float* window, const float* filters, std::vector<float>& basis,
                std::vector<float>& filt) {
    const uint32_t N = p.n_fft, K = p.K, Nw = p.win_length;
    basis.assign(p.basis_floats(), 0.0f);
    filt.assign(p.filter_floats(), 0.0f);
    std::vector<double> co(N), si(N);
    const double two_pi = 6.283185307179586476925286766559;
    for (uint32_t j = 0; j < N; j++) {
        co[j] = std::cos(two_pi * (double)j / (double)N);
        si[j] = (2 * j) % N == 0 ? 0.0 : std::sin(two_pi * (double)j / (double)N);  // s[.][0], s[.][N/2]: exactly 0
    }
    // column k of c and of s through the transpose of the frame operator; every step that is the
    // identity is skipped, so that (-0 included) nothing changes where there is no operator
    const double a = p.preemphasis, g = p.sample_scale;
    std::vector<double> u(Nw), v(Nw);
    for (uint32_t k = 0; k < K; k++)
        for (uint32_t im = 0; im < 2; im++) {
            for (uint32_t n = 0; n < Nw; n++) {
                const uint32_t j = (uint32_t)(((uint64_t)n * k) % N);
                const double w = window[n];
                u[n] = im ? -w * si[j] : w * co[j];
            }
            const double* t = u.data();
            if (a != 0.0) {
                for (uint32_t n = 0; n + 1 < Nw; n++) v[n] = u[n] - a * u[n + 1];
                v[Nw - 1] = u[Nw - 1];
                v[0] = Nw > 1 ? (1.0 - a) * u[0] - a * u[1] : (1.0 - a) * u[0];
                t = v.data();
            }
            if (p.remove_dc) {
                double sum = 0.0;
                for (uint32_t n = 0; n < Nw; n++) sum += t[n];
                const double mean = sum / (double)Nw;
                for (uint32_t n = 0; n < Nw; n++) v[n] = t[n] - mean;
                t = v.data();
            }
            if (g != 1.0) {
                for (uint32_t n = 0; n < Nw; n++) v[n] = t[n] * g;
                t = v.data();
            }
            for (uint32_t n = 0; n < Nw; n++) basis[mel_basis_index(p, n, k, im)] = (float)t[n];
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
    for (uint32_t n = 0; n < p.win_length; n++)
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
    if (p->off < 0 && (last + (uint32_t)(-p->off) + p->span) >> 63) return E_INVALID_ARGUMENT;  // (a framed plan)
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
    if (r->pad != ZFLAC_PAD_ZEROS && r->pad != ZFLAC_PAD_REFLECT && r->pad != ZFLAC_PAD_MIRROR) return E_INVALID_ARGUMENT;
    if (r->norm != ZFLAC_NORM_NONE && r->norm != ZFLAC_NORM_ROW_MAX) return E_INVALID_ARGUMENT;
    if (r->reserved != 0) return E_INVALID_ARGUMENT;
    if (r->reserved2 != 0) return E_INVALID_ARGUMENT;
    MelGrid shared;
    const int rc = mel_plan_run(p, reinterpret_cast<uintptr_t>(r->wave_device), r->rows, r->wave_frames, r->row_stride,
                                r->first_frame, r->frames, reinterpret_cast<uintptr_t>(r->dst_device), r->dst_bytes, shared);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(r->lengths_device) % sizeof(uint64_t)) return E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(r->row_max_device) % sizeof(float)) return E_INVALID_ARGUMENT;
    if (r->pad == ZFLAC_PAD_REFLECT && !p->center) return E_INVALID_ARGUMENT;  // (a centred plan is _STFT framed)
    if (r->pad == ZFLAC_PAD_MIRROR && p->framing != ZFLAC_FRAMING_KALDI_CENTER) return E_INVALID_ARGUMENT;
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

uint64_t mel_plan_frames(const MelPlan& p, uint64_t n) {
    if (!p.hop) return 0;
    if (p.framing == ZFLAC_FRAMING_SNIP) return n >= p.win_length ? (n - p.win_length) / p.hop + 1 : 0;
    if (p.framing == ZFLAC_FRAMING_KALDI_CENTER) return (uint64_t)(((unsigned __int128)n + p.hop / 2) / p.hop);
    return mel_frames(n, p.n_fft, p.hop, p.center);
}

int mel_plan_cmvn(const MelPlan* p, const zflac_mel_cmvn_desc* c, uint64_t& passes) {
    passes = 0;
    if (!p || !c) return E_INVALID_ARGUMENT;
    if (c->size != sizeof(zflac_mel_cmvn_desc)) return E_INVALID_ARGUMENT;
    if (c->mode != ZFLAC_CMVN_MEAN && c->mode != ZFLAC_CMVN_MEAN_VAR) return E_INVALID_ARGUMENT;
    if (c->ddof > 1) return E_INVALID_ARGUMENT;
    if (c->reserved != 0) return E_INVALID_ARGUMENT;
    if (!c->feat_device) return E_INVALID_ARGUMENT;
    if (c->frames == 0) return E_INVALID_ARGUMENT;
    unsigned __int128 bytes = (unsigned __int128)c->rows * p->n_bins;
    if (bytes >> 63) return E_INVALID_ARGUMENT;
    bytes *= c->frames;
    if (bytes >> 63) return E_INVALID_ARGUMENT;
    bytes *= p->elem_size();
    if (bytes >> 63) return E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(c->valid_device) % sizeof(uint64_t)) return E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(c->mean_device) % sizeof(float)) return E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(c->std_device) % sizeof(float)) return E_INVALID_ARGUMENT;
    if (!(std::isfinite(c->eps) && c->eps >= 0.0f)) return E_INVALID_ARGUMENT;
    if (!std::isfinite(c->pad_value)) return E_INVALID_ARGUMENT;
    passes = p->layout == ZFLAC_MEL_BINS_FIRST ? c->rows * p->n_bins : c->rows;
    return E_OK;
}

}  // namespace zflac
