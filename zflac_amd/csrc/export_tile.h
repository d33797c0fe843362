// export_tile.h -- the device code of the dense export that k_export (export.hip) and k_resample
// (resample.hip) share: the conversion of a container sample (or an f32 value) to the output
// dtype, and export_tile(), one tile of EXPORT_TILE frames of one row by one workgroup of
// EXPORT_THREADS lanes. export.hip's head describes the paths.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zflac_hip.h"
#include "common.h"

namespace zflac {
namespace {

template <int DT>
struct Out;
template <>
struct Out<ZFLAC_EXPORT_F32> {
    using T = float;
};
template <>
struct Out<ZFLAC_EXPORT_F16> {
    using T = _Float16;
};
template <>
struct Out<ZFLAC_EXPORT_BF16> {
    using T = uint16_t;
};
template <>
struct Out<ZFLAC_EXPORT_I32> {
    using T = int32_t;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The sample pointers come out of the row table, so the compiler cannot see that they are
// global memory and would use flat loads; they always are (hipMalloc'ed batch output).
#if defined(__HIP_DEVICE_COMPILE__)
#define ZFLAC_GLOBAL __attribute__((address_space(1)))
#else
#define ZFLAC_GLOBAL
#endif

// An f32 value as the output dtype: f16 keeps subnormals (2^-15 = 0x0200); bf16 rounds the f32
// bit pattern to nearest-even (no NaNs here).
template <int DT>
__device__ __forceinline__ typename Out<DT>::T conv_f32(float f) {
    static_assert(DT != ZFLAC_EXPORT_I32, "a float dtype");
    if constexpr (DT == ZFLAC_EXPORT_F32) {
        return f;
    } else if constexpr (DT == ZFLAC_EXPORT_F16) {
        return (_Float16)f;
    } else {
        const uint32_t u = __float_as_uint(f);
        return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
    }
}

// Its inverse, exact: an element of the output dtype as f32
template <int DT>
__device__ __forceinline__ float widen_f32(typename Out<DT>::T e) {
    static_assert(DT != ZFLAC_EXPORT_I32, "a float dtype");
    if constexpr (DT == ZFLAC_EXPORT_F32) return e;
    else if constexpr (DT == ZFLAC_EXPORT_F16) return (float)e;
    else return __uint_as_float((uint32_t)e << 16);
}

// int -> float rounds to nearest-even (25..32-bit samples), the scale is exact
template <int DT>
__device__ __forceinline__ typename Out<DT>::T conv(int32_t v, float scale) {
    if constexpr (DT == ZFLAC_EXPORT_I32) {
        return v;
    } else {
        return conv_f32<DT>((float)v * scale);
    }
}

__device__ __forceinline__ float container_scale(uint32_t kind) {
    return kind == ZFLAC_S8 ? 0x1p-7f : (kind == ZFLAC_S16 ? 0x1p-15f : 0x1p-31f);
}

// M samples (at most 16 bytes) with the container's own alignment
template <typename ST, int M>
struct __attribute__((packed, aligned(sizeof(ST)))) Chunk {
    ST e[M];
};

// N consecutive samples: one load of N * sizeof(ST) <= 16 bytes, or whole 16-byte loads
template <typename ST, int N>
__device__ __forceinline__ void load_full(const ZFLAC_GLOBAL ST* p, int32_t* v) {
    constexpr int PER = N * sizeof(ST) >= 16 ? 16 / sizeof(ST) : N;
    static_assert(N % PER == 0, "whole chunks");
#pragma unroll
    for (int k = 0; k < N / PER; k++) {
        const Chunk<ST, PER> c = reinterpret_cast<const ZFLAC_GLOBAL Chunk<ST, PER>*>(p)[k];
#pragma unroll
        for (int j = 0; j < PER; j++) v[k * PER + j] = c.e[j];
    }
}

// the first nv (< N) samples, zeros after them
template <typename ST, int N>
__device__ __forceinline__ void load_part(const ZFLAC_GLOBAL ST* p, uint32_t nv, int32_t* v) {
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = (uint32_t)i < nv ? (int32_t)p[i] : 0;
}

// N samples from p of which the first `left` exist (left <= 0: none, nothing is read)
template <typename ST, int N>
__device__ __forceinline__ void load_unit(const ZFLAC_GLOBAL ST* p, int64_t left, int32_t* v) {
    if (left >= N) {
        load_full<ST, N>(p, v);
    } else if (left > 0) {
        load_part<ST, N>(p, (uint32_t)left, v);
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) v[i] = 0;
    }
}

// one 16-byte store of 16 / sizeof(OT) elements, dst 16-byte aligned
template <typename OT>
__device__ __forceinline__ void store_unit(OT* dst, const OT* o) {
    u32x4 w;
    __builtin_memcpy(&w, o, 16);
    *reinterpret_cast<u32x4*>(dst) = w;
}

// A lane's EXPORT_GROUP elements of a tile are UNITS units of UNIT = 16 bytes of output, unit j
// at element (j * EXPORT_THREADS + lane) * UNIT of the tile: every store instruction of a wave
// covers 1 KiB of consecutive addresses (and every load one consecutive range), instead of
// each lane walking its own 64 bytes. Rows on the 16-byte store paths hold whole units.
template <typename OT>
struct Units {
    static constexpr uint32_t UNIT = 16 / sizeof(OT);
    static constexpr uint32_t UNITS = EXPORT_GROUP / UNIT;
    __device__ static __forceinline__ uint64_t at(uint64_t tile0, uint32_t j) {
        return tile0 + ((uint64_t)j * EXPORT_THREADS + threadIdx.x) * UNIT;
    }
};

// Elements [e_tile, e_tile + K * EXPORT_TILE) of a row of E elements; element j comes from
// src[j] for j < valid_e and is zero after. (valid_e == 0: src is never read.)
template <int DT, typename ST>
__device__ __forceinline__ void flat_tile(typename Out<DT>::T* dst, const ZFLAC_GLOBAL ST* src, uint64_t E, uint64_t valid_e,
                                          uint64_t e_tile, uint32_t K, float scale) {
    using OT = typename Out<DT>::T;
    using G = Units<OT>;
    for (uint32_t k = 0; k < K; k++) {
        const uint64_t tile0 = e_tile + (uint64_t)k * EXPORT_TILE;
        if (tile0 >= E) break;
        int32_t v[G::UNITS][G::UNIT];
#pragma unroll
        for (uint32_t j = 0; j < G::UNITS; j++) {  // every load first, then the stores
            const uint64_t e0 = G::at(tile0, j);
            load_unit<ST, G::UNIT>(src + e0, e0 < E ? (int64_t)(valid_e - e0) : 0, v[j]);
        }
#pragma unroll
        for (uint32_t j = 0; j < G::UNITS; j++) {
            const uint64_t e0 = G::at(tile0, j);
            OT o[G::UNIT];
#pragma unroll
            for (uint32_t i = 0; i < G::UNIT; i++) o[i] = conv<DT>(v[j][i], scale);
            if (e0 < E) store_unit(dst + e0, o);
        }
    }
}

// Frames [f_tile, f_tile + EXPORT_TILE) of a 2-channel stream into plane0 and (C >= 2) plane1.
template <int DT, typename ST>
__device__ __forceinline__ void stereo_tile(typename Out<DT>::T* plane0, typename Out<DT>::T* plane1, const ZFLAC_GLOBAL ST* src,
                                            uint64_t T, uint64_t valid_f, uint64_t f_tile, float scale) {
    using OT = typename Out<DT>::T;
    using G = Units<OT>;
    int32_t v[G::UNITS][2 * G::UNIT];
#pragma unroll
    for (uint32_t j = 0; j < G::UNITS; j++) {
        const uint64_t f0 = G::at(f_tile, j);
        load_unit<ST, 2 * G::UNIT>(src + 2 * f0, f0 < T ? 2 * (int64_t)(valid_f - f0) : 0, v[j]);
    }
#pragma unroll
    for (uint32_t j = 0; j < G::UNITS; j++) {
        const uint64_t f0 = G::at(f_tile, j);
        OT l[G::UNIT], r[G::UNIT];
#pragma unroll
        for (uint32_t i = 0; i < G::UNIT; i++) {
            l[i] = conv<DT>(v[j][2 * i], scale);
            r[i] = conv<DT>(v[j][2 * i + 1], scale);
        }
        if (f0 < T) {
            store_unit(plane0 + f0, l);
            if (plane1) store_unit(plane1 + f0, r);
        }
    }
}

// Planes [c0, c1) of a planar row: this tile's frames are zero.
template <typename OT>
__device__ __forceinline__ void zero_planes(OT* row, uint32_t c0, uint32_t c1, uint64_t T, uint64_t f_tile) {
    using G = Units<OT>;
    OT z[G::UNIT];
#pragma unroll
    for (uint32_t i = 0; i < G::UNIT; i++) z[i] = (OT)0;
    for (uint32_t c = c0; c < c1; c++)
#pragma unroll
        for (uint32_t j = 0; j < G::UNITS; j++) {
            const uint64_t f0 = G::at(f_tile, j);
            if (f0 < T) store_unit(row + (uint64_t)c * T + f0, z);
        }
}

// A lane per frame, any shape and alignment.
template <int DT, int LAYOUT>
__device__ __forceinline__ void generic_tile(typename Out<DT>::T* row, const ExportRow& r, uint32_t C, uint64_t T,
                                             uint64_t valid_f, uint64_t f_tile, float scale) {
    const uint32_t nch = r.nch;
    for (uint32_t i = threadIdx.x; i < EXPORT_TILE; i += EXPORT_THREADS) {
        const uint64_t f = f_tile + i;
        if (f >= T) break;
        const bool in = f < valid_f;
        const uint64_t s0 = (r.start + f) * nch;
        for (uint32_t c = 0; c < C; c++) {
            int32_t v = 0;
            if (in && c < nch) {
                if (r.kind == ZFLAC_S8) v = ((const ZFLAC_GLOBAL int8_t*)r.src)[s0 + c];
                else if (r.kind == ZFLAC_S16) v = ((const ZFLAC_GLOBAL int16_t*)r.src)[s0 + c];
                else v = ((const ZFLAC_GLOBAL int32_t*)r.src)[s0 + c];
            }
            const uint64_t at = LAYOUT == ZFLAC_LAYOUT_PLANAR ? (uint64_t)c * T + f : f * C + c;
            row[at] = conv<DT>(v, scale);
        }
    }
}

// Frames [f_tile, f_tile + EXPORT_TILE) of the row `row` (C x T elements) whose record is r, by
// the whole workgroup; vec: the destination and its rows are 16-byte aligned.
template <int DT, int LAYOUT>
__device__ __forceinline__ void export_tile(typename Out<DT>::T* row, const ExportRow& r, uint32_t C, uint64_t T,
                                            uint32_t vec, uint64_t f_tile) {
    const uint64_t left = r.src ? r.n_frames - r.start : 0;  // frames of the stream from `start` on
    const uint64_t valid_f = left < T ? left : T;
    const float scale = container_scale(r.kind);
    const bool zero = f_tile >= valid_f;  // store-only: error row, or a tile wholly past the end
    if (!vec) {
        generic_tile<DT, LAYOUT>(row, r, C, T, valid_f, f_tile, scale);
    } else if constexpr (LAYOUT == ZFLAC_LAYOUT_INTERLEAVED) {
        const uint64_t E = T * C, e_tile = f_tile * C;
        if (zero) {
            flat_tile<DT, int8_t>(row, (const ZFLAC_GLOBAL int8_t*)nullptr, E, 0, e_tile, C, scale);
        } else if (r.nch == C) {
            const uint64_t valid_e = valid_f * C, s0 = r.start * C;
            if (r.kind == ZFLAC_S8) flat_tile<DT>(row, (const ZFLAC_GLOBAL int8_t*)r.src + s0, E, valid_e, e_tile, C, scale);
            else if (r.kind == ZFLAC_S16) flat_tile<DT>(row, (const ZFLAC_GLOBAL int16_t*)r.src + s0, E, valid_e, e_tile, C, scale);
            else flat_tile<DT>(row, (const ZFLAC_GLOBAL int32_t*)r.src + s0, E, valid_e, e_tile, C, scale);
        } else {
            generic_tile<DT, LAYOUT>(row, r, C, T, valid_f, f_tile, scale);
        }
    } else {
        if (zero) {
            zero_planes(row, 0, C, T, f_tile);
        } else if (r.nch == 1) {
            if (r.kind == ZFLAC_S8) flat_tile<DT>(row, (const ZFLAC_GLOBAL int8_t*)r.src + r.start, T, valid_f, f_tile, 1, scale);
            else if (r.kind == ZFLAC_S16) flat_tile<DT>(row, (const ZFLAC_GLOBAL int16_t*)r.src + r.start, T, valid_f, f_tile, 1, scale);
            else flat_tile<DT>(row, (const ZFLAC_GLOBAL int32_t*)r.src + r.start, T, valid_f, f_tile, 1, scale);
            zero_planes(row, 1, C, T, f_tile);
        } else if (r.nch == 2) {
            typename Out<DT>::T* plane1 = C >= 2 ? row + T : nullptr;
            const uint64_t s0 = r.start * 2;
            if (r.kind == ZFLAC_S8) stereo_tile<DT>(row, plane1, (const ZFLAC_GLOBAL int8_t*)r.src + s0, T, valid_f, f_tile, scale);
            else if (r.kind == ZFLAC_S16) stereo_tile<DT>(row, plane1, (const ZFLAC_GLOBAL int16_t*)r.src + s0, T, valid_f, f_tile, scale);
            else stereo_tile<DT>(row, plane1, (const ZFLAC_GLOBAL int32_t*)r.src + s0, T, valid_f, f_tile, scale);
            zero_planes(row, 2, C, T, f_tile);
        } else {
            generic_tile<DT, LAYOUT>(row, r, C, T, valid_f, f_tile, scale);
        }
    }
}

}  // namespace
}  // namespace zflac
