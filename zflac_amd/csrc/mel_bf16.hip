// mel_bf16.hip -- k_mel_split: k_mel_ex's tile (mel.hip) with the first product, the DFT, on the
// bf16 matrix cores (ZFLAC_MEL_MATH_BF16X6 / _BF16X3, include/zflac_hip.h).
//
// v_mfma_f32_32x32x2_f32 runs at 1/16 of the rate of v_mfma_f32_32x32x16_bf16. An f32 value is
// the exact sum of three bf16 pieces (v0 = b(v), v1 = b(v - v0), v2 = b(v - v0 - v1)), a product of
// two pieces is exact in f32, and of the nine piece products of c * x only those of level
// i + j <= 2 (TERMS = 6) or <= 1 (TERMS = 3) are kept: the rest lies 3 * 2^-24 (2^-14) below
// |c| |x|. So
//   X[2 K x frames] = sum over (i, j) kept of  basis_i^T [2 K x N] . frames_j [N x frames]
// with f32 accumulation inside the matrix cores, and everything behind it is k_mel's: P = re^2 +
// im^2 element by element in the accumulators' registers, P's registers as the B operand of the
// f32 MFMA against the filter table (the accumulator layout of the bf16 instruction is the f32
// one's), the log, the conversion, the row maximum.
//
// The tile is k_mel's: a workgroup of MEL_WAVES waves takes MEL_FRAMES frames of one row, a wave
// MEL_TILE of them, the frame on the lane (l & 31). The loop order is not: the samples go in
// blocks of MEL_BF16_K = 16 (one MFMA's k) on the outside, the bin tiles in groups of
// MEL_BF16_GROUP on the inside, with the group's re and im accumulators live together.
//   samples  B operand: lane l holds x[k = 8 (l >> 5) + j][frame l & 31], j = 0..7, which are eight
//            consecutive samples of the lane's own frame. The lane loads them itself from the row
//            (zero or reflected outside it, zero at n >= N and for frames past the last), a block
//            ahead of their use, and splits them in registers (v_cvt_pk_bf16_f32 and a
//            subtraction per piece): no LDS, no barrier, once per block and group instead of once
//            per bin tile.
//   basis    A operand: the pieces as mel_plan.cpp laid them out, one 16-byte LDS read per lane
//            and operand, conflict free (64 lanes x 16 consecutive bytes). What a block of a group
//            needs is contiguous in the table: a plain 16-byte copy into one of two LDS buffers,
//            loaded a block ahead into registers and stored behind the block's MFMAs; one
//            barrier per block. The four waves share it.
// MEL_BF16_GROUP = 2 and two waves per SIMD (up to four filter tiles; eight need 355 registers and
// run one): with four bin tiles per group and one wave per SIMD (433 registers at four filter
// tiles) a block's MFMAs, 1,536 cycles, were shorter than the L2 latency of the next block's loads
// and nothing else was there to run: 4.77 ms against 3.85 ms on the benchmark shape.
// Every frame's sums run in the same order (blocks ascending; per block the kept terms from the
// smallest level up; then bin tiles and registers as in k_mel), whatever lane, wave or workgroup
// it falls in, so its bits depend on nothing but the N values under it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zflac_hip.h"
#include "common.h"
#include "export_tile.h"
#include "launch.h"

namespace zflac {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// FR: a framed plan (a frame shorter than the DFT or a Kaldi framing). FR = false is the kernel as
// it was before framed plans, statement for statement: the start offset is the unsigned N / 2 or 0,
// the reflect bound is half the span and there is no mirror, so the plans that existed compile to
// the code they had (a shared body cost k_mel_split 1 % on Whisper's shape).
template <int DT, int LAYOUT, int MT, int TERMS, bool FR>
__global__ __launch_bounds__(MEL_THREADS, MT <= 4 ? 2 : 1) void k_mel_split(MelSplitArgs sa) {
    using OT = typename Out<DT>::T;
    constexpr uint32_t NP = TERMS == 6 ? 3 : 2;                  // pieces of an operand in use
    constexpr uint32_t OPS = 2 * NP * 64;                        // 16-byte vectors of a bin tile's A operands
    constexpr uint32_t SLAB = MEL_BF16_GROUP * OPS;              // ... of a group, per sample block
    constexpr uint32_t PER = (SLAB + MEL_THREADS - 1) / MEL_THREADS;
    __shared__ u32x4 lds[2][SLAB];
    const MelArgs& a = sa.e.a;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t row = blockIdx.x / a.tiles;
    const uint64_t j0 = (uint64_t)(blockIdx.x - row * a.tiles) * MEL_FRAMES;  // first destination frame
    const float* const x = a.wave + row * a.row_stride;
    const uint32_t N = a.n_fft;  // the frame span: the DFT size, or a framed plan's frame length
    uint64_t n_row = a.wave_frames;
    if (sa.e.lengths) {
        const uint64_t n = sa.e.lengths[row];
        n_row = n < a.wave_frames ? n : a.wave_frames;
    }
    const bool reflect = FR ? sa.e.pad != ZFLAC_PAD_ZEROS : sa.e.pad == ZFLAC_PAD_REFLECT;  // FR: or _MIRROR
    const int64_t off = FR ? (int64_t)a.off : (int64_t)(uint32_t)a.off;
    // this lane's frame, and sample 8 (l >> 5) of it: where its eight samples of block 0 start
    const uint64_t j = j0 + wv * MEL_TILE + (lane & 31);
    const bool ok = j < a.frames;
    const uint32_t n_lane = 8 * (lane >> 5);
    const int64_t base = ok ? (int64_t)((a.first_frame + j) * a.hop) - off + n_lane : 0;
    // interior (uniform): every frame of the tile exists and every sample index the workgroup
    // forms lies in [0, n_row), blocks of padding (n >= N) included: nothing to decide per sample
    const int64_t lo = (int64_t)((a.first_frame + j0) * a.hop) - off;
    const bool interior = N % MEL_BF16_K == 0 && j0 + MEL_FRAMES <= a.frames && lo >= 0 &&
                          (uint64_t)lo + (uint64_t)(MEL_FRAMES - 1) * a.hop + N <= n_row;

    auto fetch = [&](uint32_t kb, float (&v)[8]) {
        const int64_t s0 = base + (int64_t)(kb * MEL_BF16_K);
        if (interior) {
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = x[s0 + i];
        } else if (reflect) {  // x~[s] = x[rho(s)]: one reflection about 0 or n_row - 1, zero beyond it
            // (k_mel_ex's rule: _MIRROR repeats the edge sample, m = 1, and has no bound but the row)
            const int64_t nr = (int64_t)n_row, m = FR && sa.e.pad == ZFLAC_PAD_MIRROR;
            const int64_t half = !FR ? (int64_t)(N / 2) : m ? (int64_t)1 << 62 : (int64_t)sa.e.pad_half;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int64_t s = s0 + i;
                const int64_t r = s < 0 ? -s - m : (s >= nr ? 2 * (nr - 1) + m - s : s);
                const bool in = ok && kb * MEL_BF16_K + n_lane + i < N && s >= -half && s < nr + half && r >= 0 && r < nr;
                v[i] = in ? x[r] : 0.0f;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int64_t s = s0 + i;
                const bool in = ok && kb * MEL_BF16_K + n_lane + i < N && s >= 0 && (uint64_t)s < n_row;
                v[i] = in ? x[s] : 0.0f;
            }
        }
    };

    f32x16 V[MT];
#pragma unroll
    for (int q = 0; q < MT; q++)
#pragma unroll
        for (int r = 0; r < 16; r++) V[q][r] = 0.0f;

    const u32x4* const table = reinterpret_cast<const u32x4*>(sa.pieces);
    for (uint32_t b0 = 0; b0 < a.bin_tiles; b0 += MEL_BF16_GROUP) {
        const uint32_t tg = a.bin_tiles - b0 < MEL_BF16_GROUP ? a.bin_tiles - b0 : MEL_BF16_GROUP;
        const uint32_t cnt = tg * OPS;  // vectors per block of this group
        const u32x4* const src = table + (size_t)b0 * sa.k_blocks * OPS;
        f32x16 re[MEL_BF16_GROUP], im[MEL_BF16_GROUP];
#pragma unroll
        for (uint32_t g = 0; g < MEL_BF16_GROUP; g++)
#pragma unroll
            for (int r = 0; r < 16; r++) re[g][r] = im[g][r] = 0.0f;

        // block 0 of the group (every wave is behind the last block's barrier: both buffers are free)
        u32x4 pre[PER];
        float xv[8];
#pragma unroll
        for (uint32_t i = 0; i < PER; i++)
            if (tid + i * MEL_THREADS < cnt) lds[0][tid + i * MEL_THREADS] = src[tid + i * MEL_THREADS];
        fetch(0, xv);
        __syncthreads();

        for (uint32_t kb = 0; kb < sa.k_blocks; kb++) {
            const bool more = kb + 1 < sa.k_blocks;
            float xn[8];
            if (more) {  // the next block's operands, in flight behind this block's MFMAs
                const u32x4* const nx = src + (size_t)(kb + 1) * cnt;
#pragma unroll
                for (uint32_t i = 0; i < PER; i++)
                    if (tid + i * MEL_THREADS < cnt) pre[i] = nx[tid + i * MEL_THREADS];
                fetch(kb + 1, xn);
            }
            bf16x8 xp[NP];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                float r = xv[i];
#pragma unroll
                for (uint32_t p = 0; p < NP; p++) {
                    const __bf16 h = (__bf16)r;  // round to nearest-even
                    xp[p][i] = h;
                    r -= (float)h;               // exact
                }
            }
            const u32x4* const pa = lds[kb & 1] + lane;
#pragma unroll
            for (uint32_t g = 0; g < MEL_BF16_GROUP; g++) {
                if (g < tg) {
                    bf16x8 c[NP], s[NP];
#pragma unroll
                    for (uint32_t p = 0; p < NP; p++) {
                        c[p] = __builtin_bit_cast(bf16x8, pa[g * OPS + p * 64]);
                        s[p] = __builtin_bit_cast(bf16x8, pa[g * OPS + (NP + p) * 64]);
                    }
                    auto term = [&](uint32_t i, uint32_t jx) {
                        re[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(c[i], xp[jx], re[g], 0, 0, 0);
                        im[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(s[i], xp[jx], im[g], 0, 0, 0);
                    };
                    if constexpr (TERMS == 6) {
                        term(2, 0);
                        term(1, 1);
                        term(0, 2);
                    }
                    term(1, 0);
                    term(0, 1);
                    term(0, 0);
                }
            }
            if (more) {
                u32x4* const nb = lds[(kb + 1) & 1];
#pragma unroll
                for (uint32_t i = 0; i < PER; i++)
                    if (tid + i * MEL_THREADS < cnt) nb[tid + i * MEL_THREADS] = pre[i];
#pragma unroll
                for (int i = 0; i < 8; i++) xv[i] = xn[i];
            }
            __syncthreads();  // the next block is in LDS, and this one has been read
        }

#pragma unroll
        for (uint32_t g = 0; g < MEL_BF16_GROUP; g++) {
            if (g < tg) {
                const float* const fb = a.filters + (size_t)(b0 + g) * (16 * MT * 64) + lane;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float p = __builtin_fmaf(im[g][r], im[g][r], re[g][r] * re[g][r]);
#pragma unroll
                    for (int q = 0; q < MT; q++)
                        V[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[(r * MT + q) * 64], p, V[q], 0, 0, 0);
                }
            }
        }
    }

    // k_mel_ex's epilogue
    OT* const dst = static_cast<OT*>(a.dst);
    float mx = -__builtin_inff();  // of the f32 values this lane stores
    if (ok) {
#pragma unroll
        for (int q = 0; q < MT; q++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const uint32_t m = q * MEL_TILE + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m >= a.n_bins) continue;
                float v = V[q][r];
                if (a.scale == ZFLAC_MEL_LOG10) v = log10f(fmaxf(v, a.floor));
                else if (a.scale == ZFLAC_MEL_LN) v = logf(fmaxf(v, a.floor));
                const uint64_t at = LAYOUT == ZFLAC_MEL_BINS_FIRST ? (row * a.n_bins + m) * a.frames + j
                                                                   : (row * a.frames + j) * a.n_bins + m;
                dst[at] = conv_f32<DT>(v);
                mx = fmaxf(mx, v);
            }
    }
    // the row maximum: the wave's, then one atomic on the float's bits (signed max for the
    // non-negative, unsigned min for the negative: the larger negative float has the smaller bits)
    float* const row_max = sa.e.row_max;
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

template <int DT, int LAYOUT, int TERMS, bool FR>
hipError_t launch_mt(uint32_t m_tiles, const MelSplitArgs& s, uint32_t blocks, hipStream_t st) {
#define ZFLAC_MEL_LAUNCH(MT) \
    hipLaunchKernelGGL((k_mel_split<DT, LAYOUT, MT, TERMS, FR>), dim3(blocks), dim3(MEL_THREADS), 0, st, s); \
    break
    switch (m_tiles) {
        case 1: ZFLAC_MEL_LAUNCH(1);
        case 2: ZFLAC_MEL_LAUNCH(2);
        case 4: ZFLAC_MEL_LAUNCH(4);
        case 8: ZFLAC_MEL_LAUNCH(8);
        default: return hipErrorInvalidValue;
    }
#undef ZFLAC_MEL_LAUNCH
    return hipGetLastError();
}

template <int DT, int TERMS, bool FR>
hipError_t launch_layout(int layout, uint32_t m_tiles, const MelSplitArgs& s, uint32_t blocks, hipStream_t st) {
    return layout == ZFLAC_MEL_BINS_FIRST ? launch_mt<DT, ZFLAC_MEL_BINS_FIRST, TERMS, FR>(m_tiles, s, blocks, st)
                                          : launch_mt<DT, ZFLAC_MEL_FRAMES_FIRST, TERMS, FR>(m_tiles, s, blocks, st);
}

template <int TERMS, bool FR>
hipError_t launch_dt(int dtype, int layout, uint32_t m_tiles, const MelSplitArgs& s, uint32_t blocks, hipStream_t st) {
    switch (dtype) {
        case ZFLAC_EXPORT_F32: return launch_layout<ZFLAC_EXPORT_F32, TERMS, FR>(layout, m_tiles, s, blocks, st);
        case ZFLAC_EXPORT_F16: return launch_layout<ZFLAC_EXPORT_F16, TERMS, FR>(layout, m_tiles, s, blocks, st);
        case ZFLAC_EXPORT_BF16: return launch_layout<ZFLAC_EXPORT_BF16, TERMS, FR>(layout, m_tiles, s, blocks, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

// rows * tiles workgroups, as k_mel (mel_plan_run keeps the product within gridDim.x's 2^31 - 1)
hipError_t launch_mel_split(int dtype, int layout, uint32_t m_tiles, uint32_t terms, bool framed, const MelSplitArgs& s,
                            uint64_t rows, hipStream_t st) {
    const uint64_t blocks = rows * s.e.a.tiles;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull || !s.pieces) return hipErrorInvalidValue;
    if (terms == 6) return framed ? launch_dt<6, true>(dtype, layout, m_tiles, s, (uint32_t)blocks, st)
                                  : launch_dt<6, false>(dtype, layout, m_tiles, s, (uint32_t)blocks, st);
    if (terms == 3) return framed ? launch_dt<3, true>(dtype, layout, m_tiles, s, (uint32_t)blocks, st)
                                  : launch_dt<3, false>(dtype, layout, m_tiles, s, (uint32_t)blocks, st);
    return hipErrorInvalidValue;
}

}  // namespace zflac
