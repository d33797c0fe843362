// cepstra_plan.h -- host planning of the cepstra plans (zflac_hip_cepstra_create / _project / _cmvn
// / _deltas; k_mel_dct, k_mel_cmvn, k_mel_delta): every argument check of the four calls in the
// order include/zflac_hip.h documents, the delta scale tables and the grids. Plain C++
// (cepstra_plan.cpp), no HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/zflac_hip.h"
#include "common.h"

namespace zflac {

constexpr uint32_t CEPS_MAX_DIM = 256;            // n_in, n_out
constexpr uint64_t CEPS_MAX_GRID = 0x7FFFFFFFull;  // gridDim.x

struct CepstraPlan {
    uint8_t in_dtype = 0, out_dtype = 0, layout = 0;
    bool has_matrix = false;
    uint32_t n_in = 0, n_out = 0;
    uint32_t delta_order = 0, delta_window = 0;
    uint32_t features() const { return n_out * (delta_order + 1); }
    size_t in_size() const { return in_dtype == ZFLAC_EXPORT_F32 ? 4 : 2; }
    size_t out_size() const { return out_dtype == ZFLAC_EXPORT_F32 ? 4 : 2; }
};

// zflac_hip_cepstra_create's checks, in this order: d and out (out_ptr: the caller's `out`, only
// compared with NULL); size; in_dtype, out_dtype; layout; delta_order; n_in, n_out; delta_window;
// reserved; without a matrix: n_out == n_in, in_dtype == out_dtype, delta_order > 0; with one:
// every value finite. E_OK fills p; nothing else is touched.
int cepstra_plan_create(const zflac_cepstra_desc* d, const void* out_ptr, CepstraPlan& p);

// The taps of order o (0..CEPS_MAX_ORDER) for window W (1..CEPS_MAX_WINDOW), j = -oW..oW: s_0 = [1],
// s_o = s_{o-1} * [j / sum i^2], in double
std::vector<double> cepstra_delta_scales(uint32_t order, uint32_t window);
// Where order o's taps start in the table k_mel_delta reads (orders 1, 2, .. back to back), and
// the table itself, each tap rounded to f32 once
uint32_t cepstra_scale_offset(uint32_t order, uint32_t window);
std::vector<float> cepstra_scale_table(uint32_t max_order, uint32_t window);

struct CepstraGrid {
    uint64_t tiles = 0;   // passes per row (k_mel_dct; k_mel_delta frames first) or per (row, feature)
    uint64_t passes = 0;  // workgroup passes of the kernel
    uint32_t blocks = 0;  // gridDim.x: min(passes, CEPS_MAX_GRID), each striding over the passes
};
// The grid of `passes` workgroup passes
uint32_t cepstra_grid_blocks(uint64_t passes);

// zflac_hip_cepstra_project's checks, in this order: p (the plan, NULL = no plan) and r; size;
// reserved; the plan's matrix; src_device, dst_device (NULL); src == dst; their alignments; frames;
// the source's, then the destination's bytes (63 bits). rows == 0 is E_OK with g.passes == 0.
int cepstra_plan_project(const CepstraPlan* p, const zflac_cepstra_project_desc* r, CepstraGrid& g);
// zflac_hip_cepstra_deltas's, in this order: p and r; size; reserved, reserved2; the plan's delta
// order; src_device, dst_device (NULL); src == dst; their alignments; frames; the destination's
// bytes (63 bits); valid_device's alignment (8); pad_value (finite). rows == 0 as above.
int cepstra_plan_deltas(const CepstraPlan* p, const zflac_cepstra_delta_desc* r, CepstraGrid& g);
// zflac_hip_cepstra_cmvn's: mel_plan_cmvn's (this calls it) for n_out bins of out_dtype in the layout
int cepstra_plan_cmvn(const CepstraPlan* p, const zflac_mel_cmvn_desc* c, uint64_t& passes);

}  // namespace zflac
