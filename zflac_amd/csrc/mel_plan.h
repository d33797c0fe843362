// mel_plan.h -- host planning of the log-mel features (zflac_hip_mel_create / _run, k_mel): the
// argument checks of both calls, the tables in the layout the kernel reads, the grid rule and the
// frame count. Plain C++ (mel_plan.cpp), no HIP.
//
// The definition is include/zflac_hip.h's: N = n_fft, K = N / 2 + 1,
//   re[k] = sum_n c[n][k] x[t hop - off + n],  im[k] = sum_n s[n][k] x[...],  P = re^2 + im^2,
//   v[m] = sum_k filters[m][k] P[k].
// k_mel computes both sums with the f32 MFMA v_mfma_f32_32x32x2_f32 (a 32 x 32 tile, two terms
// of the sum per instruction: lanes 0..31 carry the first, lanes 32..63 the second), so the
// tables are cut into tiles of MEL_TILE = 32 and laid out lane by lane:
//
//   basis    [bin tile b][sample pair s][re, im][h = sample of the pair][i = bin of the tile]
//            = c or s [2 s + h][32 b + i], zero for bins >= K. The 64 floats of one (b, s, re/im)
//            are the A operand of one MFMA, lane l = 32 h + i; a tile's N / 2 pairs are
//            contiguous, so a slab of it goes to LDS as a plain copy. N is even: no padding in n.
//   filters  [bin tile b][register r][filter tile q][lane l]
//            = filters[32 q + (l & 31)][32 b + mel_acc_row(r) + 4 (l >> 5)], zero for filters
//            >= n_bins and bins >= K. Register r of a 32 x 32 accumulator holds row mel_acc_row(r)
//            of the tile in lanes 0..31 and that row + 4 in lanes 32..63: P's register r is the
//            B operand of one MFMA as it stands, against this A operand.
//            The filter tiles are m_tiles = 1, 2, 4 or 8 (the least that holds n_bins).
//
// A framed plan (zflac_hip_mel_create_framed) sums over the Nw samples of its frame instead of N:
// the basis has p.span = Nw + (Nw & 1) sample rows (n >= Nw: zeros) and the pieces 16 ceil(Nw / 16),
// while the bin tiles still follow K = N / 2 + 1 of the DFT size.
//
// A split plan (ZFLAC_MEL_MATH_BF16X6 / _BF16X3, k_mel_split) has no f32 basis table. Its first
// product runs on v_mfma_f32_32x32x16_bf16 (16 terms of the sum per instruction: lane l holds
// A[row l & 31][k = 8 (l >> 5) + j], j = 0..7, eight bf16 = 16 bytes), over the bf16 pieces
// v0 = b(v), v1 = b(v - v0), v2 = b(v - v0 - v1) of the f32 entries of c and s:
//
//   pieces   [group g][sample block kb][bin tile bi of the group][re, im][piece][lane l][j]
//            = piece of c or s [16 kb + 8 (l >> 5) + j][32 (G g + bi) + (l & 31)], G = MEL_BF16_GROUP,
//            zero for samples >= N (N is padded to a multiple of 16) and bins >= K. A group holds
//            G bin tiles, the last the rest, and nothing is stored for the tiles it lacks: the
//            512 bf16 of one (bin tile, re/im, piece) are the A operand of one MFMA, one 16-byte
//            read per lane, and everything one sample block of a group needs is contiguous, so
//            it goes to LDS as a plain copy. BF16X6 stores three pieces, BF16X3 the two it uses.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/zflac_hip.h"
#include "common.h"

namespace zflac {

constexpr uint32_t MEL_MAX_FFT = 2048;
constexpr uint32_t MEL_MAX_BINS = 256;
constexpr uint64_t MEL_MAX_GRID = 0x7FFFFFFFull;  // gridDim.x

struct MelPlan {
    uint8_t dtype = 0, layout = 0, scale = 0, center = 0;
    uint32_t n_fft = 0, hop = 0, n_bins = 0;
    float floor = 0;
    uint32_t K = 0;          // N / 2 + 1
    uint32_t bin_tiles = 0;  // ceil(K / MEL_TILE)
    uint32_t m_tiles = 0;    // filter tiles: 1, 2, 4 or 8
    uint32_t math = ZFLAC_MEL_MATH_F32;
    uint32_t k_blocks = 0;   // ceil(N / MEL_BF16_K): sample blocks of a split plan
    uint32_t n_pieces = 0;   // bf16 pieces of a basis entry in the table: 3 (BF16X6), 2 (BF16X3), 0 (F32)
    // The frame (zflac_hip_mel_create_framed; n_fft, STFT, the centring offset and no operator otherwise)
    uint32_t win_length = 0; // Nw: samples of a frame
    uint32_t span = 0;       // sample rows of the f32 basis table: Nw, or Nw + 1 (a zero row) when Nw is odd
    int32_t off = 0;         // frame t starts at sample t * hop - off
    uint8_t framing = ZFLAC_FRAMING_STFT, remove_dc = 0;
    float preemphasis = 0, sample_scale = 1;
    // whether the kernels need what framed plans added (a frame that is not the DFT's, a Kaldi
    // framing); a folded operator alone does not: such a plan runs the kernels as they were
    bool framed() const { return win_length != n_fft || framing != ZFLAC_FRAMING_STFT; }
    size_t basis_floats() const { return (size_t)bin_tiles * span * 2 * MEL_TILE; }
    size_t piece_elems() const { return (size_t)bin_tiles * k_blocks * 2 * n_pieces * MEL_BF16_OPERAND; }
    size_t filter_floats() const { return (size_t)bin_tiles * 16 * m_tiles * 64; }
    size_t elem_size() const { return dtype == ZFLAC_EXPORT_F32 ? 4 : 2; }
};

// zflac_hip_mel_create's checks, in this order: d and out (out_ptr: the caller's `out`, only
// compared with NULL); size; dtype, layout, scale, center; n_fft; hop; n_bins; reserved; floor;
// window and filters (NULL, then every value finite). E_OK fills p; nothing else is touched.
int mel_plan_create(const zflac_mel_desc* d, const void* out_ptr, MelPlan& p);
// zflac_hip_mel_create_ex's: everything above, in that order, then math (a known ZFLAC_MEL_MATH_*)
int mel_plan_create_ex(const zflac_mel_desc* d, uint32_t math, const void* out_ptr, MelPlan& p);
// zflac_hip_mel_create_framed's, in this order: mel_plan_create's up to and including floor; f,
// size, win_length, framing, remove_dc, preemphasis, sample_scale, reserved; window (Nw floats) and
// filters (NULL, then every value finite); framing against center; hop <= Nw; math
int mel_plan_create_framed(const zflac_mel_desc* d, const zflac_mel_frame_desc* f, uint32_t math, const void* out_ptr,
                           MelPlan& p);

// Where the kernel's tables hold c[n][k] (im = 0) or s[n][k] (im = 1), and filters[m][k]
size_t mel_basis_index(const MelPlan& p, uint32_t n, uint32_t k, uint32_t im);
size_t mel_filter_index(const MelPlan& p, uint32_t m, uint32_t k);
// Both tables, p.basis_floats() and p.filter_floats() long, zero wherever no (n, k) or (m, k) lands.
// A framed plan's c and s are the folded c' and s' of include/zflac_hip.h: column k of the window
// times the DFT row, u[m] (double), taken through the transpose of the frame operator in O(Nw):
//   v[0] = (1 - a) u[0] - a u[1];  v[n] = u[n] - a u[n + 1], 0 < n < Nw - 1;  v[Nw - 1] = u[Nw - 1]
//   (Nw = 1: v[0] = (1 - a) u[0]);  v -= mean(v) if remove_dc;  v *= g;  rounded to f32 once.
// Each step is skipped when it is the identity (a = 0, no DC removal, g = 1), so such a plan's
// tables are mel_create_ex's byte for byte.
void mel_tables(const MelPlan& p, const float* window, const float* filters, std::vector<float>& basis,
                std::vector<float>& filt);

// bf16 rounded to nearest-even from an f32 (ties to the even bf16; no NaNs here), and its f32 value
uint16_t mel_bf16_round(float v);
float mel_bf16_value(uint16_t h);
// The pieces of an f32: h[i] = b(v - h[0] - .. - h[i - 1]); the three sum to v exactly
void mel_bf16_split(float v, uint16_t h[3]);
// Where a split plan's table holds piece `piece` (< p.n_pieces) of c[n][k] (im = 0) or s[n][k]
// (im = 1), n < 16 p.k_blocks, k < 32 p.bin_tiles: the layout's single definition
size_t mel_bf16_basis_index(const MelPlan& p, uint32_t k, uint32_t n, uint32_t im, uint32_t piece);
// A split plan's tables: p.piece_elems() bf16 pieces of the entries mel_tables gives the f32 plan
// of the same descriptor, and its filter table unchanged
void mel_bf16_tables(const MelPlan& p, const float* window, const float* filters, std::vector<uint16_t>& pieces,
                     std::vector<float>& filt);

struct MelGrid {
    uint32_t tiles = 0;   // workgroups per row: ceil(frames / MEL_FRAMES)
    uint64_t blocks = 0;  // rows * tiles
};
// zflac_hip_mel_run's checks, in this order: p (the plan, NULL = no plan), wave, dst; wave's
// alignment; row_stride; frames; dst_bytes; (first_frame + frames) * hop; the grid. rows == 0 is
// E_OK with g.blocks == 0 once the checks that do not involve rows have passed.
int mel_plan_run(const MelPlan* p, uintptr_t wave, uint64_t rows, uint64_t wave_frames, uint64_t row_stride,
                 uint64_t first_frame, uint64_t frames, uintptr_t dst, size_t dst_bytes, MelGrid& g);

// zflac_hip_mel_run_ex's checks, in this order: p (the plan, NULL = no plan) and r; size; pad, then
// norm (known values); reserved, then reserved2; everything mel_plan_run checks, in its order, on
// the fields of the same names (its arithmetic: this calls it); lengths_device's alignment (8);
// row_max_device's alignment (4); ZFLAC_PAD_REFLECT with an uncentred plan, then ZFLAC_PAD_MIRROR
// with a plan that is not ZFLAC_FRAMING_KALDI_CENTER; ZFLAC_NORM_ROW_MAX:
// row_max_device, a log scale, range (finite, >= 0), add (finite), mul (finite, != 0);
// ZFLAC_NORM_NONE: range, add, mul all 0. g is mel_plan_run's; rows == 0 is E_OK with
// g.blocks == 0 once every check has passed (none of the added ones involves rows).
int mel_plan_run_ex(const MelPlan* p, const zflac_mel_run_desc* r, MelGrid& g);
// The descriptor that is zflac_hip_mel_run: zeros, no lengths, no row maximum, no normalisation
bool mel_run_is_plain(const zflac_mel_run_desc& r);

uint64_t mel_frames(uint64_t n_samples, uint32_t n_fft, uint32_t hop, int center);
// zflac_hip_mel_plan_frames: the frame count of the plan's framing
uint64_t mel_plan_frames(const MelPlan& p, uint64_t n_samples);

// zflac_hip_mel_cmvn's checks, in this order: p and c; size; mode; ddof; reserved; feat_device;
// frames; the tensor's bytes (63 bits); valid_device's alignment (8), mean_device's and
// std_device's (4); eps (finite, >= 0); pad_value (finite). passes: workgroup passes of k_mel_cmvn
// (rows * n_bins bins first, rows frames first); rows == 0 is E_OK with passes == 0.
int mel_plan_cmvn(const MelPlan* p, const zflac_mel_cmvn_desc* c, uint64_t& passes);

}  // namespace zflac
