// cepstra.hip -- k_mel_dct and k_mel_delta: the projection of every frame's bins by a matrix (MFCC)
// and Kaldi's delta features (zflac_hip_cepstra_project / _deltas, include/zflac_hip.h).
//
// k_mel_dct. A workgroup pass takes CEPS_FRAMES = 64 frames of one row. Their n_in bins go to LDS
// as f32, x[m][f] at m * 64 + (f ^ (m & 63)): the bins-first tile is read with the frames on the
// lanes, the frames-first tile as the contiguous run of 64 n_in elements it is (consecutive lanes,
// consecutive bins of a frame), and the xor spreads either store and the reads below over the
// banks. Then a lane has one frame and a wave CEPS_KB = 4 rows of T at a time, rows 4 i .. 4 i + 3
// going to wave i % 4:
//     acc = 0;  acc = fma(T[k][m], x[m][f], acc)  for m = 0, 1, .. n_in - 1
// T[k][m] is the same for the whole wave and comes in by scalar loads (k and m are wave-uniform);
// x[m][f] is one LDS read for the four rows. The order of the sum is a function of n_in alone and
// the same in both layouts, and a frame's sum reads that frame's bins only: its bits depend neither
// on the tile it falls in nor on its neighbours. Bins-first stores have the frames on the lanes;
// frames-first stores are a lane's four consecutive features, n_out elements apart between lanes.
//
// k_mel_delta. One pass over the base features, the frame index clamped to [0, F - 1]:
//     acc = 0;  acc = fma(s_o[j], x[clamp(t + j)], acc)  for j = -oW, .. oW
// for every order o = 1 .. order, an order fixed by (o, W) alone; block 0 is the element itself.
// The taps come in by scalar loads. Bins-first: a pass takes 256 consecutive frames of one (row,
// feature), the frames on the lanes. Frames-first: a pass takes 256 / C frames of one row, thread t
// feature t % C of frame t / C (consecutive lanes, consecutive elements, as k_mel_cmvn). A lane
// reads its 2 o W + 1 neighbours straight from memory: they are the elements its neighbour lanes
// and the passes beside it read, so they come from the caches and HBM sees src once.
//
// No atomics, plain global loads and stores, at most 2^31 - 1 workgroups striding over the passes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zflac_hip.h"
#include "common.h"
#include "dispatch.h"
#include "export_tile.h"
#include "launch.h"

namespace zflac {
namespace {

// T and the delta taps are written once, before any launch, and read at wave-uniform addresses:
// the constant address space makes those reads scalar loads
#if defined(__HIP_DEVICE_COMPILE__)
#define CEPS_CONST __attribute__((address_space(4)))
#else
#define CEPS_CONST
#endif
typedef const CEPS_CONST float* UniformF32;

__device__ __forceinline__ uint32_t dct_lds_at(uint32_t m, uint32_t f) { return m * CEPS_FRAMES + (f ^ (m & (CEPS_FRAMES - 1))); }

template <int DI, int DO, int LAYOUT>
__global__ __launch_bounds__(CEPS_THREADS) void k_mel_dct(MelDctArgs a) {
    using IT = typename Out<DI>::T;
    using OT = typename Out<DO>::T;
    extern __shared__ float xs[];  // n_in x CEPS_FRAMES
    const IT* __restrict__ const src = static_cast<const IT*>(a.src);
    OT* __restrict__ const dst = static_cast<OT*>(a.dst);
    const UniformF32 T = (UniformF32)a.T;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t ni = a.n_in, no = a.n_out;
    for (uint64_t w = blockIdx.x; w < a.total; w += gridDim.x) {
        const uint64_t row = w / a.tiles, f0 = (w % a.tiles) * CEPS_FRAMES;
        const uint32_t nf = a.frames - f0 < CEPS_FRAMES ? (uint32_t)(a.frames - f0) : CEPS_FRAMES;
        // frames past the row's end are zeros: summed, never stored
        if constexpr (LAYOUT == ZFLAC_MEL_BINS_FIRST) {
            const IT* const p = src + row * ni * a.frames + f0;
            for (uint32_t m = tid >> 6; m < ni; m += CEPS_THREADS / 64)
                xs[dct_lds_at(m, lane)] = lane < nf ? widen_f32<DI>(p[(uint64_t)m * a.frames + lane]) : 0.0f;
        } else {
            const IT* const p = src + (row * a.frames + f0) * ni;
            const uint32_t n = nf * ni, q = CEPS_THREADS / ni, r = CEPS_THREADS % ni;
            uint32_t f = tid / ni, m = tid % ni;  // of element e; e + 256 is q frames and r bins on
            for (uint32_t e = tid; e < CEPS_FRAMES * ni; e += CEPS_THREADS) {
                xs[dct_lds_at(m, f)] = e < n ? widen_f32<DI>(p[e]) : 0.0f;
                f += q;
                m += r;
                if (m >= ni) {
                    m -= ni;
                    f++;
                }
            }
        }
        __syncthreads();
        for (uint32_t k0 = wave * CEPS_KB; k0 < no; k0 += CEPS_KB * (CEPS_THREADS / 64)) {
            // a row past n_out repeats the last one: computed, not stored
            UniformF32 t[CEPS_KB];
#pragma unroll
            for (uint32_t j = 0; j < CEPS_KB; j++) t[j] = T + (size_t)(k0 + j < no ? k0 + j : no - 1) * ni;
            float acc[CEPS_KB];
#pragma unroll
            for (uint32_t j = 0; j < CEPS_KB; j++) acc[j] = 0.0f;
#pragma unroll 4
            for (uint32_t m = 0; m < ni; m++) {
                const float x = xs[dct_lds_at(m, lane)];
#pragma unroll
                for (uint32_t j = 0; j < CEPS_KB; j++) acc[j] = __builtin_fmaf(t[j][m], x, acc[j]);
            }
            if (lane < nf) {
#pragma unroll
                for (uint32_t j = 0; j < CEPS_KB; j++)
                    if (k0 + j < no) {
                        const uint64_t at = LAYOUT == ZFLAC_MEL_BINS_FIRST ? (row * no + k0 + j) * a.frames + f0 + lane
                                                                           : (row * a.frames + f0 + lane) * no + k0 + j;
                        dst[at] = conv_f32<DO>(acc[j]);
                    }
            }
        }
        __syncthreads();  // the tile is free for the next pass
    }
}

template <int DT, int LAYOUT>
__global__ __launch_bounds__(CEPS_THREADS) void k_mel_delta(MelDeltaArgs a) {
    using OT = typename Out<DT>::T;
    const OT* __restrict__ const src = static_cast<const OT*>(a.src);
    OT* __restrict__ const dst = static_cast<OT*>(a.dst);
    const UniformF32 sc = (UniformF32)a.scales;
    const uint32_t tid = threadIdx.x, C = a.C, blocks = a.order + 1, W = a.window;
    const uint32_t G = CEPS_THREADS / C, cf = tid % C, g = tid / C;  // frames first: C <= CEPS_THREADS
    const OT padv = conv_f32<DT>(a.pad_value);
    for (uint64_t w = blockIdx.x; w < a.total; w += gridDim.x) {
        uint64_t row, t, stride, ostride;
        const OT* x;  // frame 0 of this lane's (row, feature)
        OT* out;      // block 0 of its frame t
        bool on;
        if constexpr (LAYOUT == ZFLAC_MEL_BINS_FIRST) {
            const uint64_t rc = w / a.tiles;
            const uint64_t c = rc % C;
            row = rc / C;
            t = (w % a.tiles) * CEPS_THREADS + tid;
            on = t < a.frames;
            x = src + rc * a.frames;
            stride = 1;
            out = dst + (row * blocks * C + c) * a.frames + t;
            ostride = (uint64_t)C * a.frames;
        } else {
            row = w / a.tiles;
            t = (w % a.tiles) * G + g;
            on = g < G && t < a.frames;
            x = src + row * a.frames * C + cf;
            stride = C;
            out = dst + (row * a.frames + t) * blocks * C + cf;
            ostride = C;
        }
        uint64_t F = a.frames;
        if (a.valid) {
            const uint64_t n = a.valid[row];
            F = n < a.frames ? n : a.frames;
        }
        if (!on) continue;
        if (t >= F) {
            for (uint32_t o = 0; o < blocks; o++) out[o * ostride] = padv;
            continue;
        }
        out[0] = x[t * stride];
        UniformF32 s = sc;
        for (uint32_t o = 1; o < blocks; o++) {
            const int64_t H = (int64_t)o * W;
            float acc = 0.0f;
            for (int64_t j = -H; j <= H; j++) {
                int64_t u = (int64_t)t + j;
                u = u < 0 ? 0 : (u > (int64_t)F - 1 ? (int64_t)F - 1 : u);
                acc = __builtin_fmaf(s[j + H], widen_f32<DT>(x[(uint64_t)u * stride]), acc);
            }
            out[o * ostride] = conv_f32<DT>(acc);
            s += 2 * H + 1;
        }
    }
}

}  // namespace

hipError_t launch_mel_dct(int in_dtype, int out_dtype, int layout, const MelDctArgs& a, hipStream_t st) {
    if (a.total == 0) return hipSuccess;
    if (a.n_in < 1 || a.n_in > 256 || a.n_out < 1 || a.n_out > 256) return hipErrorInvalidValue;
    const uint32_t blocks = a.total < 0x7FFFFFFFull ? (uint32_t)a.total : 0x7FFFFFFFu;
    const size_t lds = (size_t)a.n_in * CEPS_FRAMES * sizeof(float);  // at most 64 KiB
    return dispatch_float(in_dtype, [&](auto di) {
        return dispatch_float(out_dtype, [&](auto dout) {
            return dispatch<ZFLAC_MEL_BINS_FIRST, ZFLAC_MEL_FRAMES_FIRST>(layout, [&](auto lay) {
                constexpr int DI = decltype(di)::value, DO = decltype(dout)::value, LAYOUT = decltype(lay)::value;
                hipLaunchKernelGGL((k_mel_dct<DI, DO, LAYOUT>), dim3(blocks), dim3(CEPS_THREADS), lds, st, a);
                return hipGetLastError();
            });
        });
    });
}

hipError_t launch_mel_delta(int dtype, int layout, const MelDeltaArgs& a, hipStream_t st) {
    if (a.total == 0) return hipSuccess;
    if (a.C < 1 || a.C > CEPS_THREADS || a.order < 1 || a.order > CEPS_MAX_ORDER || a.window < 1 || a.window > CEPS_MAX_WINDOW)
        return hipErrorInvalidValue;
    const uint32_t blocks = a.total < 0x7FFFFFFFull ? (uint32_t)a.total : 0x7FFFFFFFu;
    return dispatch_float(dtype, [&](auto dt) {
        return dispatch<ZFLAC_MEL_BINS_FIRST, ZFLAC_MEL_FRAMES_FIRST>(layout, [&](auto lay) {
            constexpr int DT = decltype(dt)::value, LAYOUT = decltype(lay)::value;
            hipLaunchKernelGGL((k_mel_delta<DT, LAYOUT>), dim3(blocks), dim3(CEPS_THREADS), 0, st, a);
            return hipGetLastError();
        });
    });
}

}  // namespace zflac
