// export_plan.h -- host planning of the four dense exports (zflac_hip_batch_export, _export_mixed,
// _export_resampled, _export_resampled_mixed): which error an argument draws, which of the
// kernel's paths a row takes, a filtered row's tile, the grid, and the coefficient table's layout;
// then the row records themselves. Plain C++ (export_plan.cpp), no HIP: export_host.cpp builds
// the stream views, stages the records and launches.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/zflac_hip.h"
#include "common.h"
#include "resample_plan.h"

namespace zflac {

// A stream as the planner sees it. samples == nullptr: no usable samples (its result is an error,
// it has no channels, or nothing was decoded); n_frames, rate and nch are then 0. (A stream
// without an error and with channels always has its device pointer, so "no samples" and "no
// frames to count" are one state: see export_views, export_host.cpp.)
struct ExportStream {
    const void* samples = nullptr;  // device pointer, never read here
    uint64_t n_frames = 0;
    uint32_t rate = 0;
    uint8_t nch = 0;
    uint8_t kind = 0;  // ZFLAC_S8 / ZFLAC_S16 / ZFLAC_S32 container (also of a stream without samples)
};

// One call, from zflac_export_desc or zflac_resample_desc (d == NULL: a call every check refuses)
struct ExportCall {
    uint32_t size = 0, want_size = 1;
    int dtype = 0, max_dtype = 0;  // max_dtype: the last dtype the call takes
    int layout = 0;
    uint64_t channels = 0, frames = 0;
    const uint64_t* starts = nullptr;
    bool resampled = false;  // then:
    uint32_t sample_rate = 0, zeros = 0, reserved = 0;
    double rolloff = 0, beta = 0;
};
ExportCall export_call(const zflac_export_desc* d);
ExportCall export_call(const zflac_resample_desc* d);

// bytes of n row records with the coefficient table behind them (16-byte aligned)
inline size_t mix_table_offset(size_t row_bytes) { return (row_bytes + 15) & ~(size_t)15; }

struct ExportPlan {
    size_t n = 0;
    uint64_t C = 0, T = 0;
    uint64_t tiles = 0;  // workgroups per row: ceil(T / EXPORT_TILE), or ceil(T / tile) of a filtered row if more
    uint32_t vec = 0;    // the destination and its rows are 16-byte aligned
    const uint64_t* starts = nullptr;  // the call's (host array or NULL)
    // The matrices of a mixed export, checked and laid out as the kernels read them: at[n] is where
    // the C x n matrix of the n-channel streams starts in `table` (0: none, the fit rule), table[0]
    // is unused. mixed: the call has a matrix and launches the mixed kernel.
    bool mixed = false;
    uint16_t at[MIX_MAX_CH + 1] = {};
    std::vector<float> table;
    // The resampled call. needs: the distinct (source rate, ratio) pairs of the filtered rows;
    // ratio_of[i] < 0: row i takes k_export's paths (same rate, no samples, rate 0), else its index
    // in `needs`; n_out[i]: frames of the resampled stream. All empty in the plain call.
    struct Need {
        uint32_t fin;
        ResampleRatio ratio;
    };
    std::vector<Need> needs;
    std::vector<int> ratio_of;
    std::vector<uint64_t> n_out;
    uint64_t need_floats = 0;  // of all the tables in `needs`

    // ExportRow::mix of a stream of nch channels
    uint16_t mix_at(uint32_t nch) const { return nch <= MIX_MAX_CH ? at[nch] : 0; }
    // channels of a stream that k_resample stages: min(its own, C), or C when it is mixed first
    uint32_t staged(const ExportStream& s) const { return (uint32_t)(mix_at(s.nch) ? C : std::min<uint64_t>(s.nch, C)); }
};

// The checks of all four calls in one order, then the plan. dst and dst_bytes are numbers only.
// Returns E_OK, E_INVALID_ARGUMENT or E_OUT_OF_MEMORY (the plan's own vectors); valid_frames (may
// be NULL) is written with E_OK only, so before any device work and also when n == 0. Every
// non-NULL matrix is read here, so the caller may free it when the call returns.
int plan_export(const ExportStream* streams, size_t n, const ExportCall& call, const zflac_mix_desc* mix,
                uintptr_t dst, size_t dst_bytes, uint64_t* valid_frames, ExportPlan& plan);

// The records of a planned call, written straight into rows[n]. taps[k]: the device table of
// plan.needs[k].
void write_export_rows(const ExportPlan& plan, const ExportStream* streams, ExportRow* rows);
void write_resample_rows(const ExportPlan& plan, const ExportStream* streams, const float* const* taps,
                         ResampleRow* rows);

}  // namespace zflac
