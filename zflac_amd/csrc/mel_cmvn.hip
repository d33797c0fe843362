// mel_cmvn.hip -- k_mel_cmvn: mean / variance normalisation of every (row, bin) of a feature
// tensor over the row's valid frames, in place (zflac_hip_mel_cmvn, include/zflac_hip.h).
//
// Three passes over the elements of a (row, bin): the sum, the sum of squared deviations from the
// mean (ZFLAC_CMVN_MEAN_VAR only), the normalised store. Both sums are f64 and their order is a
// function of the valid length F alone:
//   bins first    a workgroup pass takes one (row, bin), `frames` contiguous elements. They are cut
//                 into chunks of VEC = 16 bytes' worth; thread t sums chunks t, t + 256, ... in
//                 ascending order, element by element; the 64 partial sums of a wave meet in a
//                 butterfly (xor 32, 16, .. 1) and the four waves' sums are added in wave order.
//                 A chunk is one 16-byte load or store where the (row, bin) starts on a 16-byte
//                 boundary and single elements otherwise: the same elements on the same thread
//                 in the same order either way.
//   frames first  a workgroup pass takes one row, the bins on the lanes: thread t has bin
//                 t % n_bins and the frames g, g + G, ... with g = t / n_bins, G = 256 / n_bins
//                 (consecutive threads read consecutive elements); the G partial sums of a bin are
//                 added in ascending g.
// No atomics: a run repeats bit for bit, and a row's bits depend neither on the row count nor on
// where the row sits. Plain global loads and stores; the grid is at most 2^31 - 1 workgroups,
// each striding over the passes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zflac_hip.h"
#include "common.h"
#include "dispatch.h"
#include "export_tile.h"
#include "launch.h"

namespace zflac {
namespace {

// conv((l - mu32) * r): two f32 roundings, nothing fused
template <int DT>
__device__ __forceinline__ typename Out<DT>::T cmvn_norm1(typename Out<DT>::T e, float mu32, float r) {
#pragma clang fp contract(off)
    const float d = widen_f32<DT>(e) - mu32;
    return conv_f32<DT>(d * r);
}

// mu32, sigma and r of a (row, bin) from its two f64 sums
struct CmvnStat {
    float mu32, sigma32, r;
};
__device__ __forceinline__ CmvnStat cmvn_stat(const MelCmvnArgs& a, uint64_t F, double mu, double ss) {
    CmvnStat s;
    s.mu32 = (float)mu;
    s.sigma32 = 0.0f;
    s.r = 1.0f;
    if (a.mode == ZFLAC_CMVN_MEAN_VAR) {
        const uint64_t div = F > a.ddof ? F - a.ddof : 0;
        const double sigma = div ? sqrt(ss / (double)div) : 0.0;
        const double den = sigma + (double)a.eps;
        s.sigma32 = (float)sigma;
        s.r = den == 0.0 ? 0.0f : (float)(1.0 / den);
    }
    return s;
}

// The workgroup's sum of one f64 per thread: the waves' butterflies, then the waves in order.
// `red` is MEL_CMVN_THREADS / 64 doubles that no other sum in flight uses.
__device__ __forceinline__ double cmvn_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (uint32_t w = 1; w < MEL_CMVN_THREADS / 64; w++) s += red[w];
    return s;
}

template <int DT>
__global__ __launch_bounds__(MEL_CMVN_THREADS) void k_mel_cmvn_bins(MelCmvnArgs a) {
    using OT = typename Out<DT>::T;
    constexpr uint32_t VEC = 16 / sizeof(OT);
    __shared__ double red[2][MEL_CMVN_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    OT* const feat = static_cast<OT*>(a.feat);
    for (uint64_t w = blockIdx.x; w < a.total; w += gridDim.x) {
        const uint64_t row = w / a.n_bins;
        uint64_t F = a.frames;
        if (a.valid) {
            const uint64_t n = a.valid[row];
            F = n < a.frames ? n : a.frames;
        }
        OT* const p = feat + w * a.frames;
        const bool vec = reinterpret_cast<uintptr_t>(p) % 16 == 0;
        // chunk c of the row as f32, elements at or past `end` as 0 (they are not summed)
        auto load = [&](uint64_t c, uint64_t end, float (&l)[VEC]) {
            const uint64_t j = c * VEC;
            if (vec && j + VEC <= end) {
                const u32x4 q = *reinterpret_cast<const u32x4*>(p + j);
                OT e[VEC];
                __builtin_memcpy(e, &q, 16);
#pragma unroll
                for (uint32_t k = 0; k < VEC; k++) l[k] = widen_f32<DT>(e[k]);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < VEC; k++) l[k] = j + k < end ? widen_f32<DT>(p[j + k]) : 0.0f;
            }
        };
        const uint64_t chunks = (F + VEC - 1) / VEC;
        double s = 0.0;
        for (uint64_t c = tid; c < chunks; c += MEL_CMVN_THREADS) {
            float l[VEC];
            load(c, F, l);
#pragma unroll
            for (uint32_t k = 0; k < VEC; k++)
                if (c * VEC + k < F) s += (double)l[k];
        }
        const double mu = F ? cmvn_block_sum(s, red[0]) / (double)F : 0.0;
        double ss = 0.0;
        if (a.mode == ZFLAC_CMVN_MEAN_VAR && F) {  // (uniform)
            for (uint64_t c = tid; c < chunks; c += MEL_CMVN_THREADS) {
                float l[VEC];
                load(c, F, l);
#pragma unroll
                for (uint32_t k = 0; k < VEC; k++)
                    if (c * VEC + k < F) {
                        const double d = (double)l[k] - mu;
                        ss += d * d;
                    }
            }
            ss = cmvn_block_sum(ss, red[1]);
        }
        const CmvnStat st = cmvn_stat(a, F, mu, ss);
        if (tid == 0) {
            if (a.mean) a.mean[w] = F ? st.mu32 : 0.0f;
            if (a.std) a.std[w] = F ? st.sigma32 : 0.0f;
        }
        const OT padv = conv_f32<DT>(a.pad_value);
        const uint64_t all = (a.frames + VEC - 1) / VEC;
        for (uint64_t c = tid; c < all; c += MEL_CMVN_THREADS) {
            const uint64_t j = c * VEC;
            if (vec && j + VEC <= a.frames) {
                u32x4 q = *reinterpret_cast<const u32x4*>(p + j);
                OT e[VEC];
                __builtin_memcpy(e, &q, 16);
#pragma unroll
                for (uint32_t k = 0; k < VEC; k++) e[k] = j + k < F ? cmvn_norm1<DT>(e[k], st.mu32, st.r) : padv;
                __builtin_memcpy(&q, e, 16);
                *reinterpret_cast<u32x4*>(p + j) = q;
            } else {
                for (uint32_t k = 0; k < VEC && j + k < a.frames; k++)
                    p[j + k] = j + k < F ? cmvn_norm1<DT>(p[j + k], st.mu32, st.r) : padv;
            }
        }
        __syncthreads();  // red[] is free for the next pass
    }
}

template <int DT>
__global__ __launch_bounds__(MEL_CMVN_THREADS) void k_mel_cmvn_frames(MelCmvnArgs a) {
    using OT = typename Out<DT>::T;
    __shared__ double part[MEL_CMVN_THREADS];
    __shared__ double stat[MEL_CMVN_THREADS];  // per bin: the mean, then the sum of squares
    const uint32_t tid = threadIdx.x, nb = a.n_bins;  // nb <= MEL_CMVN_THREADS
    const uint32_t G = MEL_CMVN_THREADS / nb, b = tid % nb, g = tid / nb;
    const bool on = g < G;
    OT* const feat = static_cast<OT*>(a.feat);
    for (uint64_t row = blockIdx.x; row < a.total; row += gridDim.x) {
        uint64_t F = a.frames;
        if (a.valid) {
            const uint64_t n = a.valid[row];
            F = n < a.frames ? n : a.frames;
        }
        OT* const p = feat + row * a.frames * nb + b;
        // the bin's sum of one f64 per frame group, in ascending g; every thread of the bin gets it
        auto bin_sum = [&](double v) {
            __syncthreads();  // the last sum has been read
            part[tid] = v;
            __syncthreads();
            if (tid < nb) {
                double s = part[tid];
                for (uint32_t i = 1; i < G; i++) s += part[tid + i * nb];
                stat[tid] = s;
            }
            __syncthreads();
            return stat[b];
        };
        double s = 0.0;
        if (on)
            for (uint64_t j = g; j < F; j += G) s += (double)widen_f32<DT>(p[j * nb]);
        const double mu = F ? bin_sum(s) / (double)F : 0.0;
        double ss = 0.0;
        if (a.mode == ZFLAC_CMVN_MEAN_VAR && F) {  // (uniform)
            if (on)
                for (uint64_t j = g; j < F; j += G) {
                    const double d = (double)widen_f32<DT>(p[j * nb]) - mu;
                    ss += d * d;
                }
            ss = bin_sum(ss);
        }
        const CmvnStat st = cmvn_stat(a, F, mu, ss);
        if (tid < nb) {
            if (a.mean) a.mean[row * nb + b] = F ? st.mu32 : 0.0f;
            if (a.std) a.std[row * nb + b] = F ? st.sigma32 : 0.0f;
        }
        const OT padv = conv_f32<DT>(a.pad_value);
        if (on)
            for (uint64_t j = g; j < a.frames; j += G) p[j * nb] = j < F ? cmvn_norm1<DT>(p[j * nb], st.mu32, st.r) : padv;
    }
}

}  // namespace

// a.total passes over at most 2^31 - 1 workgroups
hipError_t launch_mel_cmvn(int dtype, int layout, const MelCmvnArgs& a, hipStream_t st) {
    if (a.total == 0) return hipSuccess;
    if (a.n_bins < 1 || a.n_bins > MEL_CMVN_THREADS) return hipErrorInvalidValue;
    const uint32_t blocks = a.total < 0x7FFFFFFFull ? (uint32_t)a.total : 0x7FFFFFFFu;
    return dispatch_float(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        const dim3 grid(blocks), block(MEL_CMVN_THREADS);
        if (layout == ZFLAC_MEL_BINS_FIRST) hipLaunchKernelGGL((k_mel_cmvn_bins<DT>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_mel_cmvn_frames<DT>), grid, block, 0, st, a);
        return hipGetLastError();
    });
}

}  // namespace zflac
