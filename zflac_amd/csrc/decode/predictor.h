// decode/predictor.h -- Pred: the predictor history and coefficients (packed i16 pairs, or i64
// sums for 32-bit containers).
#pragma once
#include "config.h"

namespace zflac {

// ----------------------------------------------------------------------------------
// Predictor state. 16-bit and 8-bit containers: every subframe value fits i16 inside
// zflac's domain (src/zflac.zig:494,537 @intCast), so the order-M sum is M/2
// v_dot2c_i32_i16 over packed sample pairs; pair P[t mod M] = (lo s[t-1], hi s[t]) and
// coefficient pair m = (lo c[2m+1], hi c[2m]) where c[j] multiplies s[i-1-j]. For odd t,
// P[t] is also the little-endian i16 PCM pair (s[t-1], s[t]) the packed stores need.
// 32-bit containers: i64 sums of i32 products (InterType i64).
// ----------------------------------------------------------------------------------
typedef short short2v __attribute__((ext_vector_type(2)));

// History ring length of a bucket: the largest order M rounded up to a power of two that
// divides the chunk, so history slots line up from chunk to chunk (bucket 12: order 9..12,
// a 16-slot ring but 12 products per sample instead of 16).
template <int M>
__host__ __device__ constexpr int hist_len() { return M == 12 ? 16 : M; }

template <int KIND, int M, bool PAIRS = (KIND != 2)>
struct Pred;

template <int KIND, int M>
struct Pred<KIND, M, true> {
    static constexpr int H = hist_len<M>();
    uint32_t P[H];
    uint32_t CP[M / 2];
    int32_t last;
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < H; j++) P[j] = 0;
#pragma unroll
        for (int m = 0; m < M / 2; m++) CP[m] = 0;
        last = 0;
    }
    template <int J>
    __device__ __forceinline__ void set_coef(int32_t c) {
        if constexpr ((J & 1) == 0) CP[J >> 1] = (CP[J >> 1] & 0xFFFFu) | ((uint32_t)c << 16);
        else CP[J >> 1] = (CP[J >> 1] & 0xFFFF0000u) | ((uint32_t)c & 0xFFFFu);
    }
    template <int U>
    __device__ __forceinline__ void push(int32_t s) {
        P[U % H] = __builtin_amdgcn_perm((uint32_t)s, (uint32_t)last, 0x05040100u);  // lo last, hi s
        last = s;
    }
    template <int U>
    __device__ __forceinline__ uint32_t pair() const { return P[U % H]; }
    template <int U>
    __device__ __forceinline__ int32_t value() const {  // s at slot U (prologue warm-up)
        return (int32_t)(int16_t)(P[U % H] >> 16);
    }
    template <int U>
    __device__ __forceinline__ int64_t predict(int shift) const {
        // oldest pairs first: the newest pair (holding s[i-1], just computed) enters last,
        // so the recurrence's dependency chain is one dot2 + shift + add + pack per sample
        // (wrapping i32 / i16 sums: the order does not change the result)
        // the oldest pair starts the sum as v_dot2_i32_i16 with an inline 0 accumulator (the
        // builtin's VOP2 form needs a zeroed register: one v_mov per sample)
        int32_t acc;
        asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(acc) : "v"(P[(((U - 1 - 2 * (M / 2 - 1)) % H) + H) % H]), "v"(CP[M / 2 - 1]));
#pragma unroll
        for (int m = M / 2 - 2; m >= 0; m--) {
            const uint32_t a = P[(((U - 1 - 2 * m) % H) + H) % H];
            acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, CP[m]), acc,
                                         false);
        }
        if constexpr (Kind<KIND>::W == 16) acc = (int16_t)acc;
        return acc >> shift;
    }
    // Every product and partial sum of the prediction of slot U fits the InterType, in
    // zflac's accumulation order: oldest sample first (src/zflac.zig:527-532). Only for
    // `unsafe` lanes (large coefficients); history values fit the SampleType here.
    template <int U>
    __device__ __forceinline__ bool partials_fit(int order) const {
        constexpr int64_t HI = Kind<KIND>::W == 16 ? 0x7FFF : 0x7FFFFFFF;
        int64_t p = 0;
        bool ok = true;
#pragma unroll
        for (int j = M - 1; j >= 0; j--) {
            if (j < order) {
                const int64_t sv = (int16_t)(P[(((U - 1 - j) % H) + H) % H] >> 16);
                const int64_t cv = (j & 1) ? (int16_t)(CP[j >> 1] & 0xFFFFu) : (int16_t)(CP[j >> 1] >> 16);
                const int64_t prod = sv * cv;
                p += prod;
                ok = ok && prod >= -HI - 1 && prod <= HI && p >= -HI - 1 && p <= HI;
            }
        }
        return ok;
    }
};

template <int KIND, int M>
struct Pred<KIND, M, false> {
    static constexpr int H = hist_len<M>();
    int32_t R[H];
    int32_t C[M];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < H; j++) R[j] = 0;
#pragma unroll
        for (int j = 0; j < M; j++) C[j] = 0;
    }
    template <int J>
    __device__ __forceinline__ void set_coef(int32_t c) {
        C[J] = c;
    }
    template <int U>
    __device__ __forceinline__ void push(int32_t s) {
        R[U % H] = s;
    }
    template <int U>
    __device__ __forceinline__ int32_t value() const {
        return R[U % H];
    }
    template <int U>
    __device__ __forceinline__ int64_t predict(int shift) const {
        // ACC independent i64 accumulators over interleaved terms, the newest term (s[i-1])
        // last in accumulator 0: wrapping i64 sums, so any order gives zflac's result; more
        // accumulators shorten the chain of dependent v_mad_i64_i32 per sample
        constexpr int ACC = 1;
        int64_t acc[ACC];
#pragma unroll
        for (int a = 0; a < ACC; a++) acc[a] = 0;
#pragma unroll
        for (int j = M - 1; j >= 1; j--) acc[j % ACC] += (int64_t)C[j] * (int64_t)R[(((U - 1 - j) % H) + H) % H];
#pragma unroll
        for (int a = 1; a < ACC; a++) acc[0] += acc[a];
        acc[0] += (int64_t)C[0] * (int64_t)R[(((U - 1) % H) + H) % H];  // s[i-1] last
        return acc[0] >> shift;
    }
};

template <int KIND>
__device__ __forceinline__ int32_t add_inter(int64_t r, int64_t p) {
    if constexpr (Kind<KIND>::W == 16) return (int16_t)(r + p);
    else if constexpr (Kind<KIND>::W == 32) return (int32_t)((uint32_t)r + (uint32_t)p);
    else return (int32_t)(r + p);
}

template <int KIND>
__device__ __forceinline__ int32_t wrap_st(int64_t v) {
    if constexpr (Kind<KIND>::SB == 8) return (int32_t)(int8_t)v;
    else if constexpr (Kind<KIND>::SB == 16) return (int32_t)(int16_t)v;
    else return (int32_t)v;
}

}  // namespace zflac
