// mix_tile.h -- the device code of the mixed exports (k_export_mixed in export.hip,
// k_resample_mixed in resample.hip) for a row that has a matrix: output channel c of frame t is
//   v_c[t]: acc = +0; for j = 0 .. n - 1: acc = fmaf(m[c * n + j], x_j[t], acc)
// with x_j[t] the sample as ZFLAC_EXPORT_F32 has it, rounded to the output dtype by conv_f32().
// Frames past the stream's end are +0. Rows without a matrix never come here: they take
// export_tile() (export_tile.h) as it stands.
//
// The matrix lies in the call's coefficient table in device memory, written before the kernel
// starts and constant while it runs, and the workgroup's row is uniform: the coefficients are
// read through the constant address space, which makes every such read a scalar load into
// SGPRs, not a vector load per lane. The paths, picked uniformly for the workgroup:
//   vec      2-channel sources into C = 1 or 2 and 1-channel sources into C <= 2, destinations whose
//            rows are 16-byte aligned: 16-byte stores, a wave's stores covering consecutive
//            addresses (struct Units), every load of a sub-tile before its stores, as in
//            stereo_tile() / flat_tile(). A planar unit is 16 bytes of each plane; an interleaved
//            unit 16 bytes of the row, 16 / (C * element size) frames.
//   zero     tiles wholly past the stream's end on such destinations: export_tile()'s zero stores.
//   generic  everything else (3..8 source channels, C > 2, unaligned rows): a lane per frame, the
//            frame's n samples read once, the C chains run from registers.
// A unit that straddles the stream's end loads under the bound (load_unit), so nothing past the
// last sample of a stream is ever read. No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/zflac_hip.h"
#include "common.h"
#include "export_tile.h"

namespace zflac {
namespace {

#if defined(__HIP_DEVICE_COMPILE__)
#define ZFLAC_CONST __attribute__((address_space(4)))
#else
#define ZFLAC_CONST
#endif
typedef const ZFLAC_CONST float* MixCoef;

// the row's matrix: `coef` is the call's table, `at` the row's ExportRow::mix (nonzero)
__device__ __forceinline__ MixCoef mix_matrix(const float* coef, uint32_t at) {
    return (MixCoef)coef + at;
}

template <typename ST>
struct KindOf;
template <>
struct KindOf<int8_t> {
    static constexpr float scale = 0x1p-7f;
};
template <>
struct KindOf<int16_t> {
    static constexpr float scale = 0x1p-15f;
};
template <>
struct KindOf<int32_t> {
    static constexpr float scale = 0x1p-31f;
};

// Frames [f_tile, f_tile + EXPORT_TILE) of an N-channel stream (src at the window's first frame)
// into CO output channels, N and CO 1 or 2, on the 16-byte store paths.
template <int DT, int LAYOUT, typename ST, int N, int CO>
__device__ __forceinline__ void mix_vec_tile(typename Out<DT>::T* row, const ZFLAC_GLOBAL ST* src, MixCoef m, uint64_t T,
                                             uint64_t valid_f, uint64_t f_tile) {
    using OT = typename Out<DT>::T;
    using G = Units<OT>;
    constexpr bool IL = LAYOUT == ZFLAC_LAYOUT_INTERLEAVED;
    constexpr uint32_t FR = IL ? G::UNIT / CO : G::UNIT;  // frames of a unit
    constexpr uint32_t SUB = IL ? CO : 1;                 // the tile's frames are SUB sub-tiles of units
    constexpr float scale = KindOf<ST>::scale;
    float w[CO][N];
#pragma unroll
    for (int c = 0; c < CO; c++)
#pragma unroll
        for (int j = 0; j < N; j++) w[c][j] = m[c * N + j];
    const uint64_t E = T * (IL ? CO : 1);  // elements of the row (IL) or of a plane
    for (uint32_t k = 0; k < SUB; k++) {
        const uint64_t tile0 = f_tile * (IL ? CO : 1) + (uint64_t)k * EXPORT_TILE;
        if (tile0 >= E) break;
        int32_t v[G::UNITS][N * FR];
#pragma unroll
        for (uint32_t u = 0; u < G::UNITS; u++) {  // every load first, then the stores
            const uint64_t e0 = G::at(tile0, u);
            const uint64_t f0 = IL ? e0 / CO : e0;
            load_unit<ST, N * FR>(src + N * f0, e0 < E ? N * (int64_t)(valid_f - f0) : 0, v[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < G::UNITS; u++) {
            const uint64_t e0 = G::at(tile0, u);
            OT o[CO][FR];  // (IL: stored as o[frame][channel] below)
#pragma unroll
            for (uint32_t i = 0; i < FR; i++)
#pragma unroll
                for (int c = 0; c < CO; c++) {
                    float acc = 0.0f;
#pragma unroll
                    for (int j = 0; j < N; j++) acc = __builtin_fmaf(w[c][j], (float)v[u][N * i + j] * scale, acc);
                    if constexpr (IL) (&o[0][0])[i * CO + c] = conv_f32<DT>(acc);
                    else o[c][i] = conv_f32<DT>(acc);
                }
            if (e0 < E) {
                if constexpr (IL) {
                    store_unit(row + e0, &o[0][0]);
                } else {
#pragma unroll
                    for (int c = 0; c < CO; c++) store_unit(row + (uint64_t)c * T + e0, o[c]);
                }
            }
        }
    }
}

template <int DT, int LAYOUT, int N, int CO>
__device__ __forceinline__ void mix_vec_kind(typename Out<DT>::T* row, const ExportRow& r, MixCoef m, uint64_t T,
                                             uint64_t valid_f, uint64_t f_tile) {
    const uint64_t s0 = r.start * N;
    if (r.kind == ZFLAC_S8) mix_vec_tile<DT, LAYOUT, int8_t, N, CO>(row, (const ZFLAC_GLOBAL int8_t*)r.src + s0, m, T, valid_f, f_tile);
    else if (r.kind == ZFLAC_S16) mix_vec_tile<DT, LAYOUT, int16_t, N, CO>(row, (const ZFLAC_GLOBAL int16_t*)r.src + s0, m, T, valid_f, f_tile);
    else mix_vec_tile<DT, LAYOUT, int32_t, N, CO>(row, (const ZFLAC_GLOBAL int32_t*)r.src + s0, m, T, valid_f, f_tile);
}

// the N samples of frame `frame` of the row's stream as f32
template <int N>
__device__ __forceinline__ void mix_load_frame(const ExportRow& r, uint64_t frame, float scale, float* x) {
    const uint64_t s0 = frame * N;
    if (r.kind == ZFLAC_S8) {
#pragma unroll
        for (int j = 0; j < N; j++) x[j] = (float)((const ZFLAC_GLOBAL int8_t*)r.src)[s0 + j] * scale;
    } else if (r.kind == ZFLAC_S16) {
#pragma unroll
        for (int j = 0; j < N; j++) x[j] = (float)((const ZFLAC_GLOBAL int16_t*)r.src)[s0 + j] * scale;
    } else {
#pragma unroll
        for (int j = 0; j < N; j++) x[j] = (float)((const ZFLAC_GLOBAL int32_t*)r.src)[s0 + j] * scale;
    }
}

// output channel c of a frame whose N samples are x
template <int N>
__device__ __forceinline__ float mix_chain(MixCoef m, uint32_t c, const float* x) {
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < N; j++) acc = __builtin_fmaf(m[c * N + j], x[j], acc);
    return acc;
}

// A lane per frame, any shape and alignment.
template <int DT, int LAYOUT, int N>
__device__ __forceinline__ void mix_generic_tile(typename Out<DT>::T* row, const ExportRow& r, MixCoef m, uint32_t C,
                                                 uint64_t T, uint64_t valid_f, uint64_t f_tile, float scale) {
    for (uint32_t i = threadIdx.x; i < EXPORT_TILE; i += EXPORT_THREADS) {
        const uint64_t f = f_tile + i;
        if (f >= T) break;
        float x[N];
        if (f < valid_f) {
            mix_load_frame<N>(r, r.start + f, scale, x);
        } else {
#pragma unroll
            for (int j = 0; j < N; j++) x[j] = 0.0f;
        }
        for (uint32_t c = 0; c < C; c++) {
            const uint64_t at = LAYOUT == ZFLAC_LAYOUT_PLANAR ? (uint64_t)c * T + f : f * C + c;
            row[at] = conv_f32<DT>(mix_chain<N>(m, c, x));
        }
    }
}

// f(std::integral_constant<int, n>) for the row's channel count n = 1..8
template <typename F>
__device__ __forceinline__ void mix_by_channels(uint32_t nch, F f) {
    switch (nch) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 5: f(std::integral_constant<int, 5>()); break;
        case 6: f(std::integral_constant<int, 6>()); break;
        case 7: f(std::integral_constant<int, 7>()); break;
        default: f(std::integral_constant<int, 8>()); break;
    }
}

// export_tile() for a row with a matrix (r.mix != 0; C <= MIX_MAX_CH): frames
// [f_tile, f_tile + EXPORT_TILE) of `row` by the whole workgroup.
template <int DT, int LAYOUT>
__device__ __forceinline__ void mix_tile(typename Out<DT>::T* row, const ExportRow& r, const float* coef, uint32_t C,
                                         uint64_t T, uint32_t vec, uint64_t f_tile) {
    static_assert(DT != ZFLAC_EXPORT_I32, "a float dtype");
    const MixCoef m = mix_matrix(coef, r.mix);
    const uint64_t left = r.src ? r.n_frames - r.start : 0;
    const uint64_t valid_f = left < T ? left : T;
    const float scale = container_scale(r.kind);
    if (vec && f_tile >= valid_f) {  // store-only: every mixed value of this tile is +0
        if constexpr (LAYOUT == ZFLAC_LAYOUT_INTERLEAVED)
            flat_tile<DT, int8_t>(row, (const ZFLAC_GLOBAL int8_t*)nullptr, T * C, 0, f_tile * C, C, scale);
        else
            zero_planes(row, 0, C, T, f_tile);
    } else if (vec && C <= 2 && r.nch <= 2) {
        if (r.nch == 2) {
            if (C == 2) mix_vec_kind<DT, LAYOUT, 2, 2>(row, r, m, T, valid_f, f_tile);
            else mix_vec_kind<DT, LAYOUT, 2, 1>(row, r, m, T, valid_f, f_tile);
        } else {
            if (C == 2) mix_vec_kind<DT, LAYOUT, 1, 2>(row, r, m, T, valid_f, f_tile);
            else mix_vec_kind<DT, LAYOUT, 1, 1>(row, r, m, T, valid_f, f_tile);
        }
    } else {
        mix_by_channels(r.nch, [&](auto n) {
            mix_generic_tile<DT, LAYOUT, decltype(n)::value>(row, r, m, C, T, valid_f, f_tile, scale);
        });
    }
}

}  // namespace
}  // namespace zflac
