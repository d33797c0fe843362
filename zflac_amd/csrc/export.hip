// export.hip -- k_export: the batch's decoded samples as one dense tensor.
//
// One streaming pass from every stream's decoded output (interleaved, left-justified, in an
// i8 / i16 / i32 container; StreamState::dev_samples) into a caller-owned buffer of
// B x C x T elements: PLANAR [row][channel][frame] or INTERLEAVED [row][frame][channel], as
// f32 / f16 / bf16 (sample * 2^-(container bits - 1), an exact power of two) or i32 (the
// container value). Row i is the window [start_i, start_i + T) of stream i: frames past the
// stream's end, channels the stream does not have and rows of error streams are zero, so every
// element of the destination is written.
//
// A workgroup takes one tile of EXPORT_TILE frames of one row (blockIdx.x = row * tiles + tile),
// a lane EXPORT_GROUP frames of it, as 16-byte units of output interleaved with the other
// lanes' (struct Units). The row's record picks the path, uniformly for the workgroup:
//   flat    interleaved output of a stream with exactly C channels, or the one plane of a mono
//           stream: element j of the window maps to element j of the row. 16-byte stores;
//           the loads are the same elements (16 bytes where the container is as wide as the
//           output, less where it is narrower).
//   stereo  planar output of a 2-channel stream: loads of L R L R .. (16 bytes for 16-bit
//           samples into f32, 2 x 16 for f16), one 16-byte store stream per plane.
//   zero    tiles wholly past the stream's end, error rows, planes past the stream's channels:
//           16-byte stores, no loads.
//   generic everything else (3..8 channels into planes, channel counts that differ from C into
//           interleaved rows, destinations whose rows are not 16-byte aligned): a lane per
//           frame, so the wave's loads are contiguous and its stores coalesce per channel.
// The loads carry only the container's alignment: an arbitrary window start (or a
// stream at an odd offset of the batch's output) leaves them unaligned, which the hardware
// serves as narrower accesses, while the stores stay aligned. A unit that straddles the
// stream's end loads element by element under a bound, so nothing past the last sample of a
// stream is ever read. No LDS, no scratch; all element offsets are 64-bit. The device code is
// in export_tile.h, which k_resample (resample.hip) shares for the rows it does not filter.
//
// k_export_mixed is the kernel of zflac_hip_batch_export_mixed: the same grid and the same row
// records, with the call's coefficient table as a second argument. A row whose record names a
// matrix (ExportRow::mix) takes mix_tile() (mix_tile.h), every other row export_tile() as above.
// k_export itself knows nothing of matrices: the unmixed call launches it as before.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zflac_hip.h"
#include "common.h"
#include "dispatch.h"
#include "export_tile.h"
#include "launch.h"
#include "mix_tile.h"

namespace zflac {
namespace {

template <int DT, int LAYOUT>
__global__ __launch_bounds__(EXPORT_THREADS) void k_export(ExportArgs a) {
    using OT = typename Out<DT>::T;
    const uint32_t row_i = blockIdx.x / a.tiles;
    const uint32_t tile = blockIdx.x - row_i * a.tiles;
    if (row_i >= a.n_rows) return;
    const ExportRow r = a.rows[row_i];
    OT* row = static_cast<OT*>(a.dst) + (uint64_t)row_i * a.channels * a.frames;
    export_tile<DT, LAYOUT>(row, r, a.channels, a.frames, a.vec, (uint64_t)tile * EXPORT_TILE);
}

template <int DT, int LAYOUT>
__global__ __launch_bounds__(EXPORT_THREADS) void k_export_mixed(ExportArgs a, const float* coef) {
    using OT = typename Out<DT>::T;
    const uint32_t row_i = blockIdx.x / a.tiles;
    const uint32_t tile = blockIdx.x - row_i * a.tiles;
    if (row_i >= a.n_rows) return;
    const ExportRow r = a.rows[row_i];
    OT* row = static_cast<OT*>(a.dst) + (uint64_t)row_i * a.channels * a.frames;
    if (r.mix) mix_tile<DT, LAYOUT>(row, r, coef, a.channels, a.frames, a.vec, (uint64_t)tile * EXPORT_TILE);
    else export_tile<DT, LAYOUT>(row, r, a.channels, a.frames, a.vec, (uint64_t)tile * EXPORT_TILE);
}

}  // namespace

// a.n_rows * a.tiles workgroups (the caller keeps the product within gridDim.x's 2^31 - 1)
hipError_t launch_export(int dtype, int layout, const ExportArgs& a, hipStream_t st) {
    const uint32_t blocks = a.n_rows * a.tiles;
    if (blocks == 0) return hipSuccess;
    return dispatch_else<ZFLAC_EXPORT_F32, ZFLAC_EXPORT_F16, ZFLAC_EXPORT_BF16, ZFLAC_EXPORT_I32>(dtype, [&](auto dt) {
        return dispatch_else<ZFLAC_LAYOUT_PLANAR, ZFLAC_LAYOUT_INTERLEAVED>(layout, [&](auto lay) {
            hipLaunchKernelGGL((k_export<decltype(dt)::value, decltype(lay)::value>), dim3(blocks), dim3(EXPORT_THREADS), 0,
                               st, a);
            return hipGetLastError();
        });
    });
}

// the same grid; dtype is F32, F16 or BF16, a.channels at most MIX_MAX_CH, coef the call's table
hipError_t launch_export_mixed(int dtype, int layout, const ExportArgs& a, const float* coef, hipStream_t st) {
    const uint32_t blocks = a.n_rows * a.tiles;
    if (blocks == 0) return hipSuccess;
    return dispatch_float(dtype, [&](auto dt) {
        return dispatch_else<ZFLAC_LAYOUT_PLANAR, ZFLAC_LAYOUT_INTERLEAVED>(layout, [&](auto lay) {
            hipLaunchKernelGGL((k_export_mixed<decltype(dt)::value, decltype(lay)::value>), dim3(blocks),
                               dim3(EXPORT_THREADS), 0, st, a, coef);
            return hipGetLastError();
        });
    });
}

}  // namespace zflac
