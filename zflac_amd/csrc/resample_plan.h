// resample_plan.h -- host planning of the resampled export (zflac_hip_batch_export_resampled,
// k_resample): the rational ratio, the filter's width, the polyphase tap tables, the length
// arithmetic and the kernel's tile rule. Plain C++ (resample_plan.cpp), no HIP.
//
// A stream of rate fin goes to rate fout: g = gcd(fin, fout), M = fin / g, L = fout / g. With
// `zeros` Z, `rolloff` and `beta` the filter is a Kaiser-windowed sinc of cutoff
// s = min(1, L / M) * rolloff, half width W = ceil(Z / s) input frames, K = 2 W + 1 taps.
// Output frame m sits at input time m M / L = q + r / L (q = floor(m M / L), r = (m M) mod L):
//   y[m] = sum_{k < K} h[r][k] * x[q - W + k]           (x = 0 outside the stream)
//   u[r][k] = s sinc(t) kaiser(t),  t = s ((k - W) - r / L)
//   kaiser(t) = I0(beta sqrt(1 - (t / Z)^2)) / I0(beta) for |t| < Z, else 0
//   h[r][k] = u[r][k] / sum_k u[r][k]                   (unit DC gain in every phase)
// computed in double and rounded once to float.
#pragma once
#include <cstdint>
#include <vector>

#include "common.h"

namespace zflac {

constexpr uint32_t RESAMPLE_MAX_RATE = 1048575;       // 20 bits, STREAMINFO's limit
constexpr uint32_t RESAMPLE_MAX_TAPS = 4096;          // K of any one row
constexpr uint64_t RESAMPLE_MAX_TABLE_FLOATS = 4ull << 20;  // all the tables one call needs

struct ResampleRatio {
    uint32_t L = 0, M = 0;  // fout / g, fin / g
    uint32_t W = 0;         // half width, input frames
    uint64_t K = 0;         // 2 W + 1 (64-bit: callers compare it with RESAMPLE_MAX_TAPS)
    double s = 0;           // min(1, L / M) * rolloff
    uint64_t table_floats() const { return (uint64_t)L * K; }
};

// zeros >= 1, 0 < rolloff <= 1, beta >= 0 (and finite)
bool resample_params_ok(uint32_t zeros, double rolloff, double beta);
// false when a rate is 0 or above RESAMPLE_MAX_RATE (r is then untouched)
bool resample_ratio(uint32_t fin, uint32_t fout, uint32_t zeros, double rolloff, ResampleRatio& r);
// ceil(n_frames * L / M); 0 when either rate is 0
uint64_t resampled_frames(uint64_t n_frames, uint32_t fin, uint32_t fout);
// h[L][K]; r.K <= RESAMPLE_MAX_TAPS
void resample_taps(const ResampleRatio& r, uint32_t zeros, double beta, std::vector<float>& h);

// How k_resample tiles a row of `channels` staged channels (min(stream channels, C) >= 1): whether
// the table goes into LDS, the channels staged together (1, 2 or 4: 3..8 channels go in fours)
// and the output frames per workgroup.
// A tile of n output frames spans at most ceil((n - 1) M / L) + K input frames, and `cg` times
// that many floats fit the span's share of the LDS. tile is a multiple of the workgroup's
// RESAMPLE_THREADS where it can be (a lane per output frame, no pass left part idle), else of 64
// (whole waves), at most RESAMPLE_MAX_TILE.
struct ResampleTile {
    uint32_t tile = 0;
    uint8_t cg = 0, tab_lds = 0;
};
ResampleTile resample_tile(const ResampleRatio& r, uint32_t channels);

}  // namespace zflac
