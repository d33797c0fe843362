// resample.hip -- k_resample: the dense export (export.hip) with every row brought to one
// sample rate by a polyphase Kaiser-windowed sinc (resample_plan.h has the filter).
//
// blockIdx.x = row * tiles + tile. The row's record (ResampleRow) picks the path, uniformly
// for the workgroup:
//   export   taps == nullptr: the stream already has the target rate, ended in an error, or the
//            window lies past its end. The workgroup's first EXPORT_THREADS lanes take tile `tile`
//            of EXPORT_TILE frames through export_tile(), k_export's own code, so such a row has
//            k_export's bits.
//   filter   the workgroup takes output frames [tile * r.tile, (tile + 1) * r.tile) of the window.
//            Those past the stream's end, and the channels the stream does not have, are zero
//            stores. For the others it stages the input span the tile reads,
//            [q(first) - W, q(last) + W], from the container samples into LDS as f32
//            (sample * 2^-(container bits - 1), as k_export converts), r.cg (1, 2 or 4) channels
//            at a time, a frame's channels side by side; frames outside the stream are staged as
//            zeros and never loaded. Then a lane per output frame sums its K products for the
//            staged channels from one read of each tap and one (4, 8 or 16 bytes) of each frame,
//            with fmaf in ascending k from 0: a given (row, frame, channel) has the same bits
//            whatever window or tile it falls in.
// LDS (dynamic, RESAMPLE_LDS_FLOATS): [the row's table h[L][K] when r.tab_lds, padded to 16 bytes]
// [the span]. Without
// tab_lds the taps are read from global memory (the table is then larger than its share of LDS;
// consecutive k of a phase are consecutive addresses). The host sizes r.tile and r.cg so that the
// span fits (resample_tile); the kernel checks it again before it writes LDS.
// All frame and element offsets are 64-bit.
//
// k_resample_mixed (zflac_hip_batch_export_resampled_mixed) is the same workgroup code with the
// call's coefficient table as a second argument. A row whose record names a matrix (r.e.mix) is
// mixed before it is filtered: its staging loop reads each input frame's n samples once and writes
// v_c (mix_tile.h) for the group's output channels into the frame's cg slots, so the span holds C
// channels (not min(n, C)) and the host sized the tile for C; on the export path such a row takes
// mix_tile(). filter_tile() is the same for both. k_resample has no matrix code in it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zflac_hip.h"
#include "common.h"
#include "dispatch.h"
#include "export_tile.h"
#include "launch.h"
#include "mix_tile.h"

namespace zflac {
namespace {

__device__ __forceinline__ int32_t load_sample(const void* src, uint32_t kind, uint64_t at) {
    if (kind == ZFLAC_S8) return ((const ZFLAC_GLOBAL int8_t*)src)[at];
    if (kind == ZFLAC_S16) return ((const ZFLAC_GLOBAL int16_t*)src)[at];
    return ((const ZFLAC_GLOBAL int32_t*)src)[at];
}

template <typename OT, int LAYOUT>
__device__ __forceinline__ OT* element(OT* row, uint32_t C, uint64_t T, uint64_t f, uint32_t c) {
    return row + (LAYOUT == ZFLAC_LAYOUT_PLANAR ? (uint64_t)c * T + f : f * C + c);
}

template <int NC>
struct Frame;  // NC staged channels of one input frame: one LDS read
template <>
struct Frame<1> {
    typedef float T;
    static __device__ __forceinline__ float at(T v, int) { return v; }
};
template <>
struct Frame<2> {
    typedef float T __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ float at(T v, int c) { return v[c]; }
};
template <>
struct Frame<4> {
    typedef float T __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ float at(T v, int c) { return v[c]; }
};

// An LDS read the compiler may not pair with its neighbour: it would merge the reads of taps k
// and k + 1 (and of their two frames) into ds_read2_b32 / ds_read2_b64, which this LDS serves at
// a quarter of the rate of single ds_read_b32 / _b64 / _b128 (MI355X: 8 and 16 cycles a wave
// against 2 and 4).
#if defined(__HIP_DEVICE_COMPILE__)
#define ZFLAC_LDS __attribute__((address_space(3)))
#else
#define ZFLAC_LDS
#endif
template <typename V>
__device__ __forceinline__ V lds_read(const V* p) {
    return *(const volatile ZFLAC_LDS V*)p;
}

// Output frames [f0, f0 + nv) of channels [c0, c0 + g), g <= NC: xs holds S staged frames of NC
// channels each, frame 0 = input frame q0 - W. TAPS_LDS: the taps are in LDS, else in global memory.
template <int DT, int LAYOUT, int NC, bool TAPS_LDS>
__device__ __forceinline__ void filter_tile(typename Out<DT>::T* row, const ResampleRow& r, uint32_t C, uint64_t T,
                                            uint64_t f0, uint32_t nv, uint32_t c0, uint32_t g, const float* xs,
                                            uint64_t q0, const float* taps) {
    using OT = typename Out<DT>::T;
    using F = Frame<NC>;
    const uint32_t K = r.K;
    for (uint32_t i = threadIdx.x; i < nv; i += RESAMPLE_THREADS) {
        const uint64_t p = (r.e.start + f0 + i) * r.M;  // < n_out * M <= n_frames * L + M
        const uint64_t q = p / r.L;
        const uint32_t ph = (uint32_t)(p - q * r.L);
        const typename F::T* x = reinterpret_cast<const typename F::T*>(xs) + (uint32_t)(q - q0);
        const float* h = taps + (size_t)ph * K;
        float acc[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = 0.0f;
#pragma unroll 8
        for (uint32_t k = 0; k < K; k++) {
            float t;
            if constexpr (TAPS_LDS) t = lds_read(h + k);
            else t = ((const ZFLAC_GLOBAL float*)h)[k];
            const typename F::T v = lds_read(x + k);
#pragma unroll
            for (int c = 0; c < NC; c++) acc[c] = __builtin_fmaf(t, F::at(v, c), acc[c]);
        }
#pragma unroll
        for (int c = 0; c < NC; c++)
            if ((uint32_t)c < g) *element<OT, LAYOUT>(row, C, T, f0 + i, c0 + c) = conv_f32<DT>(acc[c]);
    }
}

template <int DT, int LAYOUT, bool TAPS_LDS>
__device__ __forceinline__ void filter_group(uint32_t cg, typename Out<DT>::T* row, const ResampleRow& r, uint32_t C,
                                             uint64_t T, uint64_t f0, uint32_t nv, uint32_t c0, uint32_t g,
                                             const float* xs, uint64_t q0, const float* taps) {
    switch (cg) {
        case 1: filter_tile<DT, LAYOUT, 1, TAPS_LDS>(row, r, C, T, f0, nv, c0, g, xs, q0, taps); break;
        case 2: filter_tile<DT, LAYOUT, 2, TAPS_LDS>(row, r, C, T, f0, nv, c0, g, xs, q0, taps); break;
        default: filter_tile<DT, LAYOUT, 4, TAPS_LDS>(row, r, C, T, f0, nv, c0, g, xs, q0, taps); break;
    }
}
static_assert(RESAMPLE_THREADS >= EXPORT_THREADS, "export_tile() needs EXPORT_THREADS lanes");
static_assert(RESAMPLE_MAX_CG == 4, "filter_group dispatches 1, 2 or 4 channels");

// The span's frames for a row with a matrix: a lane per input frame reads the frame's N samples
// once and writes mixed channels [c0, c0 + g) to the frame's cg slots.
template <int N>
__device__ __forceinline__ void stage_mixed(float* xs, const ResampleRow& r, MixCoef m, uint32_t S, int64_t first,
                                            uint32_t c0, uint32_t g, float scale) {
    for (uint32_t fr = threadIdx.x; fr < S; fr += RESAMPLE_THREADS) {
        const int64_t at = first + fr;
        float x[N];
        if (at >= 0 && (uint64_t)at < r.e.n_frames) {
            mix_load_frame<N>(r.e, (uint64_t)at, scale, x);
        } else {
#pragma unroll
            for (int j = 0; j < N; j++) x[j] = 0.0f;
        }
        for (uint32_t c = 0; c < g; c++) xs[fr * r.cg + c] = mix_chain<N>(m, c0 + c, x);
    }
}

template <int DT, int LAYOUT>
__global__ __launch_bounds__(RESAMPLE_THREADS) void k_resample(ResampleArgs a) {
    using OT = typename Out<DT>::T;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t row_i = blockIdx.x / a.tiles;
    const uint32_t tile = blockIdx.x - row_i * a.tiles;
    if (row_i >= a.n_rows) return;
    const ResampleRow r = a.rows[row_i];
    const uint64_t T = a.frames;
    const uint32_t C = a.channels;
    OT* row = static_cast<OT*>(a.dst) + (uint64_t)row_i * C * T;
    if (!r.taps) {  // k_export's paths (the grid may hold more tiles than such a row has)
        const uint64_t f_tile = (uint64_t)tile * EXPORT_TILE;
        if (f_tile < T && threadIdx.x < EXPORT_THREADS) export_tile<DT, LAYOUT>(row, r.e, C, T, a.vec, f_tile);
        return;
    }
    const uint64_t f0 = (uint64_t)tile * r.tile;
    if (f0 >= T) return;
    const uint32_t n = (uint32_t)(T - f0 < r.tile ? T - f0 : r.tile);  // frames of this tile
    const uint64_t left = r.n_out - r.e.start;                         // (start < n_out with taps)
    const uint64_t valid_f = left < T ? left : T;
    const uint32_t nv = f0 < valid_f ? (uint32_t)(valid_f - f0 < n ? valid_f - f0 : n) : 0;  // ... with a value
    const uint32_t nst = r.e.nch < C ? r.e.nch : C;  // channels with a value
    // zero: frames past the stream's end, channels the stream does not have
    for (uint32_t i = threadIdx.x; i < n; i += RESAMPLE_THREADS)
        for (uint32_t c = i < nv ? nst : 0; c < C; c++) *element<OT, LAYOUT>(row, C, T, f0 + i, c) = (OT)0;
    if (!nv) return;

    const uint32_t K = r.K, nch = r.e.nch;
    const uint32_t tab = r.tab_lds ? (r.L * K + 3u) & ~3u : 0;  // the span 16-byte aligned behind the table
    float* xs = lds + tab;
    const uint64_t q0 = (r.e.start + f0) * r.M / r.L;
    const uint64_t q1 = (r.e.start + f0 + nv - 1) * r.M / r.L;
    const uint64_t span = q1 - q0 + K;
    if (span * r.cg > RESAMPLE_LDS_FLOATS - tab) return;  // (never: resample_tile sized the tile)
    const uint32_t S = (uint32_t)span;
    if (r.tab_lds)
        for (uint32_t i = threadIdx.x; i < r.L * K; i += RESAMPLE_THREADS) lds[i] = ((const ZFLAC_GLOBAL float*)r.taps)[i];
    const float scale = container_scale(r.e.kind);
    const int64_t first = (int64_t)q0 - (int64_t)r.W;  // input frame of span index 0 (may be negative)
    for (uint32_t c0 = 0; c0 < nst; c0 += r.cg) {
        const uint32_t g = nst - c0 < r.cg ? nst - c0 : r.cg;
        if (c0) __syncthreads();  // the last group's sums have read xs
        // the span's samples in memory order (frame, channel), those of this group to their frame's
        // r.cg slots (slots past g are summed but never stored, so they stay unwritten)
        for (uint32_t e = threadIdx.x; e < S * nch; e += RESAMPLE_THREADS) {
            const uint32_t fr = e / nch, ch = e - fr * nch;
            if (ch < c0 || ch >= c0 + g) continue;
            const int64_t at = first + fr;
            int32_t v = 0;
            if (at >= 0 && (uint64_t)at < r.e.n_frames) v = load_sample(r.e.src, r.e.kind, (uint64_t)at * nch + ch);
            xs[fr * r.cg + (ch - c0)] = (float)v * scale;
        }
        __syncthreads();
        if (r.tab_lds)
            filter_group<DT, LAYOUT, true>(r.cg, row, r, C, T, f0, nv, c0, g, xs, q0, lds);
        else
            filter_group<DT, LAYOUT, false>(r.cg, row, r, C, T, f0, nv, c0, g, xs, q0, r.taps);
    }
}

// k_resample with the call's coefficient table (zflac_hip_batch_export_resampled_mixed). The rows
// whose record names a matrix (r.e.mix) are mixed before they are filtered: the span holds v_c, C
// channels of it, in place of the source channels. Every other row is treated as k_resample treats
// it. (A kernel of its own, not a template parameter of k_resample's body: the compiler does not
// give the unmixed instantiation of a shared body k_resample's instructions.)
template <int DT, int LAYOUT>
__global__ __launch_bounds__(RESAMPLE_THREADS) void k_resample_mixed(ResampleArgs a, const float* coef) {
    using OT = typename Out<DT>::T;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t row_i = blockIdx.x / a.tiles;
    const uint32_t tile = blockIdx.x - row_i * a.tiles;
    if (row_i >= a.n_rows) return;
    const ResampleRow r = a.rows[row_i];
    const uint64_t T = a.frames;
    const uint32_t C = a.channels;
    OT* row = static_cast<OT*>(a.dst) + (uint64_t)row_i * C * T;
    const bool mixed = r.e.mix != 0;
    if (!r.taps) {  // k_export's paths (the grid may hold more tiles than such a row has)
        const uint64_t f_tile = (uint64_t)tile * EXPORT_TILE;
        if (f_tile < T && threadIdx.x < EXPORT_THREADS) {
            if (mixed) mix_tile<DT, LAYOUT>(row, r.e, coef, C, T, a.vec, f_tile);
            else export_tile<DT, LAYOUT>(row, r.e, C, T, a.vec, f_tile);
        }
        return;
    }
    const uint64_t f0 = (uint64_t)tile * r.tile;
    if (f0 >= T) return;
    const uint32_t n = (uint32_t)(T - f0 < r.tile ? T - f0 : r.tile);  // frames of this tile
    const uint64_t left = r.n_out - r.e.start;                         // (start < n_out with taps)
    const uint64_t valid_f = left < T ? left : T;
    const uint32_t nv = f0 < valid_f ? (uint32_t)(valid_f - f0 < n ? valid_f - f0 : n) : 0;  // ... with a value
    // channels with a value (a mixed row stages v_c: every output channel)
    const uint32_t nst = mixed ? C : (r.e.nch < C ? r.e.nch : C);
    // zero: frames past the stream's end, channels the stream does not have
    for (uint32_t i = threadIdx.x; i < n; i += RESAMPLE_THREADS)
        for (uint32_t c = i < nv ? nst : 0; c < C; c++) *element<OT, LAYOUT>(row, C, T, f0 + i, c) = (OT)0;
    if (!nv) return;

    const uint32_t K = r.K, nch = r.e.nch;
    const uint32_t tab = r.tab_lds ? (r.L * K + 3u) & ~3u : 0;  // the span 16-byte aligned behind the table
    float* xs = lds + tab;
    const uint64_t q0 = (r.e.start + f0) * r.M / r.L;
    const uint64_t q1 = (r.e.start + f0 + nv - 1) * r.M / r.L;
    const uint64_t span = q1 - q0 + K;
    if (span * r.cg > RESAMPLE_LDS_FLOATS - tab) return;  // (never: resample_tile sized the tile)
    const uint32_t S = (uint32_t)span;
    if (r.tab_lds)
        for (uint32_t i = threadIdx.x; i < r.L * K; i += RESAMPLE_THREADS) lds[i] = ((const ZFLAC_GLOBAL float*)r.taps)[i];
    const float scale = container_scale(r.e.kind);
    const int64_t first = (int64_t)q0 - (int64_t)r.W;  // input frame of span index 0 (may be negative)
    for (uint32_t c0 = 0; c0 < nst; c0 += r.cg) {
        const uint32_t g = nst - c0 < r.cg ? nst - c0 : r.cg;
        if (c0) __syncthreads();  // the last group's sums have read xs
        if (mixed) {
            const MixCoef m = mix_matrix(coef, r.e.mix);
            mix_by_channels(nch, [&](auto n) { stage_mixed<decltype(n)::value>(xs, r, m, S, first, c0, g, scale); });
        } else {
            // the span's samples in memory order (frame, channel), those of this group to their frame's
            // r.cg slots (slots past g are summed but never stored, so they stay unwritten)
            for (uint32_t e = threadIdx.x; e < S * nch; e += RESAMPLE_THREADS) {
                const uint32_t fr = e / nch, ch = e - fr * nch;
                if (ch < c0 || ch >= c0 + g) continue;
                const int64_t at = first + fr;
                int32_t v = 0;
                if (at >= 0 && (uint64_t)at < r.e.n_frames) v = load_sample(r.e.src, r.e.kind, (uint64_t)at * nch + ch);
                xs[fr * r.cg + (ch - c0)] = (float)v * scale;
            }
        }
        __syncthreads();
        if (r.tab_lds)
            filter_group<DT, LAYOUT, true>(r.cg, row, r, C, T, f0, nv, c0, g, xs, q0, lds);
        else
            filter_group<DT, LAYOUT, false>(r.cg, row, r, C, T, f0, nv, c0, g, xs, q0, r.taps);
    }
}

// coef == nullptr: k_resample, else k_resample_mixed
hipError_t launch_any(int dtype, int layout, const ResampleArgs& a, const float* coef, hipStream_t st) {
    const uint32_t blocks = a.n_rows * a.tiles;
    if (blocks == 0) return hipSuccess;
    const uint32_t lds_bytes = RESAMPLE_LDS_FLOATS * sizeof(float);
    return dispatch_float(dtype, [&](auto dt) {
        return dispatch_else<ZFLAC_LAYOUT_PLANAR, ZFLAC_LAYOUT_INTERLEAVED>(layout, [&](auto lay) {
            constexpr int DT = decltype(dt)::value, LAYOUT = decltype(lay)::value;
            // above the 64 KiB a kernel may ask for by default
            const void* k = coef ? reinterpret_cast<const void*>(&k_resample_mixed<DT, LAYOUT>)
                                 : reinterpret_cast<const void*>(&k_resample<DT, LAYOUT>);
            const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            if (e != hipSuccess) return e;
            const dim3 grid(blocks), block(RESAMPLE_THREADS);
            if (coef) hipLaunchKernelGGL((k_resample_mixed<DT, LAYOUT>), grid, block, lds_bytes, st, a, coef);
            else hipLaunchKernelGGL((k_resample<DT, LAYOUT>), grid, block, lds_bytes, st, a);
            return hipGetLastError();
        });
    });
}

}  // namespace

// a.n_rows * a.tiles workgroups (the caller keeps the product within gridDim.x's 2^31 - 1);
// dtype is F32, F16 or BF16
hipError_t launch_resample(int dtype, int layout, const ResampleArgs& a, hipStream_t st) {
    return launch_any(dtype, layout, a, nullptr, st);
}

// the same grid and LDS; a.channels at most MIX_MAX_CH, coef the call's table (not null)
hipError_t launch_resample_mixed(int dtype, int layout, const ResampleArgs& a, const float* coef, hipStream_t st) {
    if (!coef) return hipErrorInvalidValue;
    return launch_any(dtype, layout, a, coef, st);
}

}  // namespace zflac
