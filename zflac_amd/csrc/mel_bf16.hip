// mel_bf16.hip -- k_mel_split: k_mel_ex's tile (mel.hip) with the first product, the DFT, on the
// bf16 matrix cores (ZFLAC_MEL_MATH_BF16X6 / _BF16X3, include/zflac_hip.h).
//
// v_mfma_f32_32x32x2_f32 runs at 1/16 of the rate of v_mfma_f32_32x32x16_bf16. An f32 value is
// the exact sum of three bf16 pieces (v0 = b(v), v1 = b(v - v0), v2 = b(v - v0 - v1)), a product of
// two pieces is exact in f32, and of the nine piece products of c * x only those of level
// i + j <= 2 (TERMS = 6) or <= 1 (TERMS = 3) are kept: the rest lies 3 * 2^-24 (2^-14) below
// |c| |x|. So
//   X[2 K x frames] = sum over (i, j) kept of  basis_i^T [2 K x N] . frames_j [N x frames]
// with f32 accumulation inside the matrix cores, and everything behind it is mel_tile.h's, the
// code k_mel_ex runs: P = re^2 + im^2 element by element in the accumulators' registers, P's
// registers as the B operand of the f32 MFMA against the filter table (the accumulator layout of
// the bf16 instruction is the f32 one's), the log, the conversion, the row maximum. So are the
// frame origin, the row length and the padding rule in front of it. This unit owns how the samples
// and the pieces reach the bf16 MFMAs.
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
#include "dispatch.h"
#include "export_tile.h"
#include "launch.h"
#include "mel_tile.h"

namespace zflac {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// FR: a framed plan (a frame shorter than the DFT or a Kaldi framing), with mel_tile.h's signed
// origin and its padding rule for such plans. A template flag, not a run-time one: a shared body
// cost the plans without a frame of their own 1 % on Whisper's shape.
template <int DT, int LAYOUT, int MT, int TERMS, bool FR>
__global__ __launch_bounds__(MEL_THREADS, MT <= 4 ? 2 : 1) void k_mel_split(MelSplitArgs sa) {
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
    const uint32_t N = a.span;
    const uint64_t n_row = mel_row_length(a, sa.e.lengths, row);
    const bool reflect = mel_pads<FR>(sa.e.pad);
    const int64_t off = mel_origin<FR>(a);
    // this lane's frame, and sample 8 (l >> 5) of it: where its eight samples of block 0 start
    const uint64_t j = j0 + wv * MEL_TILE + (lane & 31);
    const bool ok = j < a.frames;
    const uint32_t n_lane = 8 * (lane >> 5);
    const int64_t base = ok ? (int64_t)((a.first_frame + j) * a.hop) - off + n_lane : 0;
    // interior (uniform): every frame of the tile exists and every sample index the workgroup
    // forms lies in [0, n_row), blocks of padding (n >= N) included: nothing to decide per sample
    const bool interior = N % MEL_BF16_K == 0 && j0 + MEL_FRAMES <= a.frames && mel_tile_inside(a, j0, off, n_row);

    auto fetch = [&](uint32_t kb, float (&v)[8]) {
        const int64_t s0 = base + (int64_t)(kb * MEL_BF16_K);
        if (interior) {
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = x[s0 + i];
        } else if (reflect) {
            const MelPad<FR> padded(a, n_row, sa.e.pad, sa.e.pad_half);
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = padded.read(x, s0 + i, ok && kb * MEL_BF16_K + n_lane + i < N);
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = mel_read_zeros(x, s0 + i, n_row, ok && kb * MEL_BF16_K + n_lane + i < N);
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
                mel_filter<MT>(V, a.filters + (size_t)(b0 + g) * (16 * MT * 64) + lane, re[g], im[g]);
            }
        }
    }
    mel_store<DT, LAYOUT, MT, true>(a, V, row, j, lane, sa.e.row_max);
}

}  // namespace

// rows * tiles workgroups, as k_mel (mel_plan_run keeps the product within gridDim.x's 2^31 - 1)
hipError_t launch_mel_split(int dtype, int layout, uint32_t m_tiles, uint32_t terms, bool framed, const MelSplitArgs& s,
                            uint64_t rows, hipStream_t st) {
    const uint64_t blocks = rows * s.e.a.tiles;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull || !s.pieces) return hipErrorInvalidValue;
    return dispatch<6, 3>(terms, [&](auto tm) {
        return dispatch<true, false>(framed, [&](auto fr) {
            return dispatch_float(dtype, [&](auto dt) {
                return dispatch_else<ZFLAC_MEL_BINS_FIRST, ZFLAC_MEL_FRAMES_FIRST>(layout, [&](auto lay) {
                    return dispatch<1, 2, 4, 8>(m_tiles, [&](auto mt) {
                        hipLaunchKernelGGL((k_mel_split<decltype(dt)::value, decltype(lay)::value, decltype(mt)::value,
                                                        decltype(tm)::value, decltype(fr)::value>),
                                           dim3((uint32_t)blocks), dim3(MEL_THREADS), 0, st, s);
                        return hipGetLastError();
                    });
                });
            });
        });
    });
}

}  // namespace zflac
