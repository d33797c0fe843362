// mel_tile.h -- the device rules that k_mel, k_mel_ex (mel.hip) and k_mel_split (mel_bf16.hip)
// share, each written once: where a frame starts and how long its row is, the padded read of a
// sample outside the row, the second product (the filterbank over P = re^2 + im^2) and the
// epilogue (log, conversion, store, row maximum). What the kernels do not share, how the samples
// and the basis reach the first product's MFMAs, stays in their units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zflac_hip.h"
#include "common.h"
#include "export_tile.h"

namespace zflac {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));  // a 32 x 32 f32 accumulator, per lane

// Frame t starts at sample t * hop - mel_origin(). SIGNED: a framed plan, whose offset may be
// negative; the plans before them carry the unsigned N / 2 or 0.
template <bool SIGNED>
__device__ __forceinline__ int64_t mel_origin(const MelArgs& a) {
    return SIGNED ? (int64_t)a.off : (int64_t)(uint32_t)a.off;
}

// The row's own length: lengths[row] clamped to the rows' common length (uniform)
__device__ __forceinline__ uint64_t mel_row_length(const MelArgs& a, const uint64_t* lengths, uint64_t row) {
    if (!lengths) return a.wave_frames;
    const uint64_t n = lengths[row];
    return n < a.wave_frames ? n : a.wave_frames;
}

// Whether the launch pads by reflection at all. FR: a framed plan, which may also ask for _MIRROR.
template <bool FR>
__device__ __forceinline__ bool mel_pads(uint32_t pad) {
    return FR ? pad != ZFLAC_PAD_ZEROS : pad == ZFLAC_PAD_REFLECT;
}

// Whether every sample index of the workgroup's MEL_FRAMES frames, the first of them destination
// frame j0, lies inside [0, n_row): such a tile has nothing to pad (uniform).
__device__ __forceinline__ bool mel_tile_inside(const MelArgs& a, uint64_t j0, int64_t off, uint64_t n_row) {
    const int64_t lo = (int64_t)((a.first_frame + j0) * a.hop) - off;
    return lo >= 0 && (uint64_t)lo + (uint64_t)(MEL_FRAMES - 1) * a.hop + a.span <= n_row;
}

// x[s] of a zero-padded row, and nothing where `ok` is false
__device__ __forceinline__ float mel_read_zeros(const float* x, int64_t s, uint64_t n_row, bool ok) {
    return ok && s >= 0 && (uint64_t)s < n_row ? x[s] : 0.0f;
}

// The padding rule: x~[s] = x[rho(s)], one reflection about 0 or n_row - 1, zero beyond it.
//   _REFLECT  rho(s) = -s, 2 (n_row - 1) - s, inside the signal padded by `half` samples: half the
//             span, or half the DFT size (pad_half) for a framed plan (FR), whose span is shorter
//   _MIRROR   (FR only) repeats the edge sample (m = 1): rho(s) = -1 - s, 2 n_row - 1 - s, with no
//             bound but the row
// Built once per call site, outside its loop.
template <bool FR>
struct MelPad {
    int64_t nr, m, half;
    __device__ __forceinline__ MelPad(const MelArgs& a, uint64_t n_row, uint32_t pad, uint32_t pad_half)
        : nr((int64_t)n_row),
          m(FR && pad == ZFLAC_PAD_MIRROR),
          half(!FR ? (int64_t)(a.span / 2) : m ? (int64_t)1 << 62 : (int64_t)pad_half) {}
    __device__ __forceinline__ float read(const float* x, int64_t s, bool ok) const {
        const int64_t r = s < 0 ? -s - m : (s >= nr ? 2 * (nr - 1) + m - s : s);
        return ok && s >= -half && s < nr + half && r >= 0 && r < nr ? x[r] : 0.0f;
    }
};

// The second product for one bin tile: P = re^2 + im^2 register by register, each register as it
// stands the B operand of one MFMA (rows mel_acc_row(r) and + 4 in the two lane halves) against
// the filter table; fb is the bin tile's part of it at this lane.
template <int MT>
__device__ __forceinline__ void mel_filter(f32x16 (&V)[MT], const float* fb, const f32x16& re, const f32x16& im) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const float p = __builtin_fmaf(im[r], im[r], re[r] * re[r]);
#pragma unroll
        for (int q = 0; q < MT; q++) V[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[(r * MT + q) * 64], p, V[q], 0, 0, 0);
    }
}

// The epilogue: this lane's MT x 16 values of destination frame j (none if j is past the last):
// floor and log, the layout's address, the conversion. ROW_MAX: the maximum of the f32 values the
// lane stores, the wave's, then one atomic per wave on the float's bits (signed max for the
// non-negative, unsigned min for the negative: the larger negative float has the smaller bits)
// into row_max[row], -inf before the launch; row_max == NULL: not wanted.
template <int DT, int LAYOUT, int MT, bool ROW_MAX>
__device__ __forceinline__ void mel_store(const MelArgs& a, const f32x16 (&V)[MT], uint64_t row, uint64_t j, uint32_t lane,
                                          float* row_max) {
    using OT = typename Out<DT>::T;
    OT* const dst = static_cast<OT*>(a.dst);
    float mx = -__builtin_inff();
    if (j < a.frames) {
#pragma unroll
        for (int q = 0; q < MT; q++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const uint32_t m = q * MEL_TILE + mel_acc_row(r) + 4 * (lane >> 5);
                if (m >= a.n_bins) continue;
                float v = V[q][r];
                if (a.scale == ZFLAC_MEL_LOG10) v = log10f(fmaxf(v, a.floor));
                else if (a.scale == ZFLAC_MEL_LN) v = logf(fmaxf(v, a.floor));
                const uint64_t at = LAYOUT == ZFLAC_MEL_BINS_FIRST ? (row * a.n_bins + m) * a.frames + j
                                                                   : (row * a.frames + j) * a.n_bins + m;
                dst[at] = conv_f32<DT>(v);
                if constexpr (ROW_MAX) mx = fmaxf(mx, v);
            }
    }
    if constexpr (ROW_MAX) {
        if (row_max) {
#pragma unroll
            for (int o = 32; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            const uint32_t u = __float_as_uint(mx);
            if (lane == 0 && u != 0xFF800000u) {
                if (u >> 31) atomicMin(reinterpret_cast<unsigned int*>(row_max + row), u);
                else atomicMax(reinterpret_cast<int*>(row_max + row), (int)u);
            }
        }
    }
}

}  // namespace
}  // namespace zflac
