// mel.hip -- k_mel: log-mel features of dense f32 rows in one launch (zflac_hip_mel_run); k_mel_ex
// and k_mel_norm: the same with per-row lengths, reflect padding, the row maximum and the clamp to
// it (zflac_hip_mel_run_ex).
//
// Two chained f32 matrix products on the matrix cores (v_mfma_f32_32x32x2_f32, bit for bit an
// f32 fmaf chain), per tile of frames:
//   X[2 K x frames] = basis^T [2 K x N] . frames [N x frames]      (re and im of every bin)
//   V[n_bins x frames] = filters [n_bins x K] . P [K x frames]      P = re^2 + im^2
// A workgroup of MEL_WAVES waves takes MEL_FRAMES = 128 frames of one row (blockIdx.x =
// row * tiles + tile), a wave MEL_TILE = 32 of them: the frame is on the lane (l & 31) of every
// tile the wave holds, bins and filters are on the accumulators' rows. The wave keeps V for all
// MT filter tiles (MT x 16 registers) and walks the bin tiles; for one bin tile it sums a re and
// an im accumulator over all N samples, squares them element by element into P, and feeds P's 16
// registers, each as it stands the B operand of one MFMA (rows r and r + 4 in the two lane
// halves), into V against the filter table, whose k order mel_plan.cpp has permuted to that map.
// Nothing crosses lanes and P never leaves the registers.
//
// Both operands of the first product come from LDS, in slabs of MEL_SLAB samples:
//   basis   the slab of the bin tile as mel_plan.cpp laid it out (64 lanes of re, 64 of im per
//           sample pair): a plain 16-byte copy, read back one float per lane, conflict free. The
//           four waves share it: every float fetched from L2 feeds 128 frames.
//   frames  expanded: E[pair][frame][sample of the pair], the frames' samples x[t hop - off + n]
//           read from the row (zero outside it and for frames past the last) by 8 consecutive
//           samples of 8 frames per wave and written with MEL_PAIR_STRIDE = 2 * 128 + 16 floats
//           per pair, which spreads those 64 writes over the 64 banks; a wave's MFMA operand is
//           then 64 consecutive floats. Expanding costs N / hop times the row's bytes from L1 / L2
//           and nothing else: it is what lets any hop up to N through one path (a span of
//           31 hop + N samples does not fit LDS at hop = N = 2048).
// Every frame's sums run in the same order (n ascending in pairs, bin tiles ascending, registers
// ascending), whatever lane, wave or workgroup it falls in, so its bits depend on nothing but
// its samples. Frames past the destination's end are computed from zeros and not stored.
//
// zflac_hip_mel_run_ex launches k_mel_ex, the same tile with three additions that leave every
// sum as it is: the row's own length n_i (one uniform load), reflect padding, and the row
// maximum. Only the staging of E knows about padding: a workgroup decides once whether its tile is
// interior (every sample index of its 128 frames inside [0, n_i)) and then stages exactly as
// k_mel does; the first tile, the tiles around a row's end and those past it take a second loop
// that reads x[rho(s)]. The epilogue takes the maximum of the f32 values a lane stores, a wave
// reduces it and one atomic per wave goes to row_max[row] (-inf before the launch). k_mel_norm is
// the elementwise pass behind it (ZFLAC_NORM_ROW_MAX).
//
// The frame origin, the row length, rho, the second product and the epilogue are mel_tile.h's,
// which k_mel_split (mel_bf16.hip) shares; this unit owns the staging through LDS and the f32
// MFMA loop.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zflac_hip.h"
#include "common.h"
#include "dispatch.h"
#include "export_tile.h"
#include "launch.h"
#include "mel_tile.h"

namespace zflac {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// One workgroup's tile. EX = false is zflac_hip_mel_run's kernel; EX = true (zflac_hip_mel_run_ex)
// adds the row's own length, reflect padding and the row maximum. FR (with EX): a framed plan,
// with mel_tile.h's signed origin and its padding rule for such plans. FR is a template flag, not
// a run-time one, so that the plans without a frame of their own run the code they always had.
template <int DT, int LAYOUT, int MT, bool EX, bool FR>
__device__ __forceinline__ void mel_tile(const MelArgs& a, const uint64_t* lengths, float* row_max, uint32_t pad,
                                         uint32_t pad_half) {
    __shared__ __attribute__((aligned(16))) float lds[MEL_LDS_FLOATS];
    float* const lb = lds;                               // basis slab
    float* const lf = lds + MEL_SLAB * 2 * MEL_TILE;     // frames slab
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t row = blockIdx.x / a.tiles;
    const uint64_t j0 = (uint64_t)(blockIdx.x - row * a.tiles) * MEL_FRAMES;  // first destination frame
    const float* const x = a.wave + row * a.row_stride;
    const uint32_t N = a.span;
    // the row's length, and whether this tile needs the reflection: both uniform, decided once.
    // An interior tile stages as ever.
    uint64_t n_row = a.wave_frames;
    bool edge = false;
    const int64_t off = mel_origin<!EX || FR>(a);
    if constexpr (EX) {
        n_row = mel_row_length(a, lengths, row);
        if (mel_pads<FR>(pad)) edge = !mel_tile_inside(a, j0, off, n_row);
    }

    // staging of the frames: this thread's sample of every eight and its frame of every 32
    const uint32_t st_n = tid & 7, st_j = tid >> 3;
    int64_t st_base[MEL_WAVES];  // sample index of n = 0 of frame st_j + 32 g, or "no frame"
    bool st_ok[MEL_WAVES];
#pragma unroll
    for (uint32_t g = 0; g < MEL_WAVES; g++) {
        const uint64_t j = j0 + st_j + MEL_TILE * g;
        st_ok[g] = j < a.frames;
        st_base[g] = st_ok[g] ? (int64_t)((a.first_frame + j) * a.hop) - off : 0;
    }

    f32x16 V[MT];
#pragma unroll
    for (int q = 0; q < MT; q++)
#pragma unroll
        for (int r = 0; r < 16; r++) V[q][r] = 0.0f;

    for (uint32_t b = 0; b < a.bin_tiles; b++) {
        f32x16 re, im;
#pragma unroll
        for (int r = 0; r < 16; r++) re[r] = im[r] = 0.0f;
        const float* const bb = a.basis + (size_t)b * N * (2 * MEL_TILE);
        for (uint32_t n0 = 0; n0 < N; n0 += MEL_SLAB) {
            const uint32_t ns = N - n0 < MEL_SLAB ? N - n0 : MEL_SLAB;  // even
            __syncthreads();  // the last slab has been read
            const float* const bs = bb + (size_t)n0 * (2 * MEL_TILE);
            for (uint32_t i = tid * 4; i < ns * (2 * MEL_TILE); i += MEL_THREADS * 4)
                *reinterpret_cast<f32x4*>(lb + i) = *reinterpret_cast<const f32x4*>(bs + i);
            if (EX && edge) {
                const MelPad<FR> padded(a, n_row, pad, pad_half);
                for (uint32_t n = st_n; n < ns; n += 8) {
                    float v[MEL_WAVES];
#pragma unroll
                    for (uint32_t g = 0; g < MEL_WAVES; g++) v[g] = padded.read(x, st_base[g] + (int64_t)(n0 + n), st_ok[g]);
#pragma unroll
                    for (uint32_t g = 0; g < MEL_WAVES; g++)
                        lf[(n >> 1) * MEL_PAIR_STRIDE + 2 * (st_j + MEL_TILE * g) + (n & 1)] = v[g];
                }
            } else {
                for (uint32_t n = st_n; n < ns; n += 8) {
                    float v[MEL_WAVES];
#pragma unroll
                    for (uint32_t g = 0; g < MEL_WAVES; g++)
                        v[g] = mel_read_zeros(x, st_base[g] + (int64_t)(n0 + n), n_row, st_ok[g]);
#pragma unroll
                    for (uint32_t g = 0; g < MEL_WAVES; g++)
                        lf[(n >> 1) * MEL_PAIR_STRIDE + 2 * (st_j + MEL_TILE * g) + (n & 1)] = v[g];
                }
            }
            __syncthreads();
            const float* const pa = lb + lane;
            const float* const pf = lf + 2 * (wv * MEL_TILE + (lane & 31)) + (lane >> 5);
            auto pair = [&](uint32_t s) {
                const float xb = pf[s * MEL_PAIR_STRIDE];
                re = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[s * 4 * MEL_TILE], xb, re, 0, 0, 0);
                im = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[s * 4 * MEL_TILE + 2 * MEL_TILE], xb, im, 0, 0, 0);
            };
            if (ns == MEL_SLAB) {  // (the same order either way)
#pragma unroll 8
                for (uint32_t s = 0; s < MEL_SLAB / 2; s++) pair(s);
            } else {
                for (uint32_t s = 0; s < ns / 2; s++) pair(s);
            }
        }
        mel_filter<MT>(V, a.filters + (size_t)b * (16 * MT * 64) + lane, re, im);
    }

    const uint64_t j = j0 + wv * MEL_TILE + (lane & 31);
    if constexpr (!EX) {
        if (j >= a.frames) return;
    }
    mel_store<DT, LAYOUT, MT, EX>(a, V, row, j, lane, row_max);
}

template <int DT, int LAYOUT, int MT>
__global__ __launch_bounds__(MEL_THREADS) void k_mel(MelArgs a) {
    mel_tile<DT, LAYOUT, MT, false, false>(a, nullptr, nullptr, 0, 0);
}

template <int DT, int LAYOUT, int MT, bool FR>
__global__ __launch_bounds__(MEL_THREADS) void k_mel_ex(MelExArgs e) {
    mel_tile<DT, LAYOUT, MT, true, FR>(e.a, e.lengths, e.row_max, e.pad, e.pad_half);
}

// k_mel_norm: (max(l, M_row - range) + add) * mul over the destination in place, every operation
// one f32 rounding. A row's n_bins * frames elements are contiguous in either layout; a workgroup
// pass takes MEL_NORM_CHUNK of them: elements up to the first 16-byte boundary one by one, then
// 16-byte vectors, then the rest one by one (all one by one where dst is not element aligned).
template <int DT>
__device__ __forceinline__ typename Out<DT>::T mel_norm1(typename Out<DT>::T e, float thr, float add, float mul) {
#pragma clang fp contract(off)
    const float c = fmaxf(widen_f32<DT>(e), thr);
    const float s = c + add;
    return conv_f32<DT>(s * mul);
}

template <int DT>
__global__ __launch_bounds__(MEL_NORM_THREADS) void k_mel_norm(MelNormArgs a) {
    using OT = typename Out<DT>::T;
    constexpr uint32_t ES = sizeof(OT), VEC = 16 / ES;
    const uint32_t tid = threadIdx.x;
    for (uint64_t w = blockIdx.x; w < a.total; w += gridDim.x) {
        const uint64_t row = w / a.chunks, start = (w - row * a.chunks) * MEL_NORM_CHUNK;
        const uint32_t cnt = a.row_elems - start < MEL_NORM_CHUNK ? (uint32_t)(a.row_elems - start) : MEL_NORM_CHUNK;
        float thr;
        {
#pragma clang fp contract(off)
            thr = a.row_max[row] - a.range;
        }
        OT* const p = static_cast<OT*>(a.dst) + (row * a.row_elems + start);
        const uintptr_t ad = reinterpret_cast<uintptr_t>(p);
        uint32_t head = cnt;
        if (ad % ES == 0) {
            head = (uint32_t)((16 - ad % 16) % 16) / ES;
            if (head > cnt) head = cnt;
        }
        const uint32_t body = (cnt - head) / VEC, tail = cnt - head - body * VEC;
        for (uint32_t i = tid; i < head; i += MEL_NORM_THREADS) p[i] = mel_norm1<DT>(p[i], thr, a.add, a.mul);
        u32x4* const vp = reinterpret_cast<u32x4*>(p + head);
        for (uint32_t v = tid; v < body; v += MEL_NORM_THREADS) {
            u32x4 q = vp[v];
            OT e[VEC];
            __builtin_memcpy(e, &q, 16);
#pragma unroll
            for (uint32_t k = 0; k < VEC; k++) e[k] = mel_norm1<DT>(e[k], thr, a.add, a.mul);
            __builtin_memcpy(&q, e, 16);
            vp[v] = q;
        }
        OT* const tp = p + head + body * VEC;
        for (uint32_t i = tid; i < tail; i += MEL_NORM_THREADS) tp[i] = mel_norm1<DT>(tp[i], thr, a.add, a.mul);
    }
}

// EX: 0 k_mel, 1 k_mel_ex, 2 k_mel_ex of a framed plan
template <int EX, typename A>
hipError_t launch_any(int dtype, int layout, uint32_t m_tiles, const A& a, uint64_t blocks, hipStream_t st) {
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    return dispatch_float(dtype, [&](auto dt) {
        return dispatch_else<ZFLAC_MEL_BINS_FIRST, ZFLAC_MEL_FRAMES_FIRST>(layout, [&](auto lay) {
            return dispatch<1, 2, 4, 8>(m_tiles, [&](auto mt) {
                constexpr int DT = decltype(dt)::value, LAYOUT = decltype(lay)::value, MT = decltype(mt)::value;
                const dim3 grid((uint32_t)blocks), block(MEL_THREADS);
                if constexpr (EX) hipLaunchKernelGGL((k_mel_ex<DT, LAYOUT, MT, EX == 2>), grid, block, 0, st, a);
                else hipLaunchKernelGGL((k_mel<DT, LAYOUT, MT>), grid, block, 0, st, a);
                return hipGetLastError();
            });
        });
    });
}

}  // namespace

// rows * a.tiles workgroups (mel_plan_run keeps the product within gridDim.x's 2^31 - 1)
hipError_t launch_mel(int dtype, int layout, uint32_t m_tiles, const MelArgs& a, uint64_t rows, hipStream_t st) {
    return launch_any<0>(dtype, layout, m_tiles, a, rows * a.tiles, st);
}

hipError_t launch_mel_ex(int dtype, int layout, uint32_t m_tiles, bool framed, const MelExArgs& e, uint64_t rows,
                         hipStream_t st) {
    return framed ? launch_any<2>(dtype, layout, m_tiles, e, rows * e.a.tiles, st)
                  : launch_any<1>(dtype, layout, m_tiles, e, rows * e.a.tiles, st);
}

// a.total passes of MEL_NORM_CHUNK elements, over at most 2^31 - 1 workgroups
hipError_t launch_mel_norm(int dtype, const MelNormArgs& a, hipStream_t st) {
    if (a.total == 0) return hipSuccess;
    const uint32_t blocks = a.total < 0x7FFFFFFFull ? (uint32_t)a.total : 0x7FFFFFFFu;
    return dispatch_float(dtype, [&](auto dt) {
        hipLaunchKernelGGL((k_mel_norm<decltype(dt)::value>), dim3(blocks), dim3(MEL_NORM_THREADS), 0, st, a);
        return hipGetLastError();
    });
}

}  // namespace zflac
