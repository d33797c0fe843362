// launch.h -- every launch_* entry of the .hip units, declared once: the unit that defines
// one and the host units that call it include this header, so a signature that drifts
// between the two is a compile error.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

namespace zflac {

// scan.hip
hipError_t launch_scan(const ScanArgs& a, hipStream_t st);
hipError_t launch_scan_chunks(const uint32_t* cnt, const unsigned long long* units, uint32_t n, uint32_t* off,
                              unsigned long long* uoff, uint32_t* n_frames, hipStream_t st);
hipError_t launch_compact(const CompactArgs& a, hipStream_t st);
hipError_t launch_sync_list(const SyncListArgs& a, hipStream_t st);
hipError_t launch_verify(const VerifyArgs& a, uint32_t max_items, hipStream_t st);

// hop.hip: the frame table in place of launch_scan + launch_scan_chunks + launch_compact
hipError_t launch_hop(const HopArgs& a, hipStream_t st);

// decode_k{0,1,2}_{stereo,mono,multi}.hip: the bucket launches of one (container kind, layout);
// each ends with its _mix unit's (constant / verbatim subframes). launch_walk_k*: k_walk of the
// container (defined in the stereo unit).
using DecodeLaunch = hipError_t(const DecodeArgs& a, uint32_t max_frames, hipStream_t st);
DecodeLaunch launch_decode_k0_stereo, launch_decode_k0_mono, launch_decode_k0_multi;
DecodeLaunch launch_decode_k1_stereo, launch_decode_k1_mono, launch_decode_k1_multi;
DecodeLaunch launch_decode_k2_stereo, launch_decode_k2_mono, launch_decode_k2_multi;
DecodeLaunch launch_decode_k0_stereo_mix, launch_decode_k0_mono_mix, launch_decode_k0_multi_mix;
DecodeLaunch launch_decode_k1_stereo_mix, launch_decode_k1_mono_mix, launch_decode_k1_multi_mix;
DecodeLaunch launch_decode_k2_stereo_mix, launch_decode_k2_mono_mix, launch_decode_k2_multi_mix;
DecodeLaunch launch_walk_k0, launch_walk_k1, launch_walk_k2;

// walk_wave.hip
hipError_t launch_walk_wave(int kind, const DecodeArgs& a, uint32_t max_frames, hipStream_t st);

// crc16.hip
hipError_t launch_crc16(const Crc16Args& a, uint32_t max_frames, hipStream_t st);

// md5.hip. coop_mode: the Md5Mode every job shares with 16-byte aligned samples (the
// cooperative-load kernel), or -1 (lane-per-stream loads). *kernel (optional): the Md5Kernel
// launched, k_md5_multi where the device refuses k_md5_coop's LDS; 0 when there was no job.
hipError_t launch_md5(const Md5Job* jobs, uint32_t n_jobs, uint32_t* digests, hipStream_t st, int coop_mode,
                      uint32_t* kernel = nullptr);
hipError_t launch_md5_multi(const Md5Segs& sg, hipStream_t st, int coop_mode, uint32_t* kernel = nullptr);

// export.hip
hipError_t launch_export(int dtype, int layout, const ExportArgs& a, hipStream_t st);
// k_export_mixed: coef is the call's coefficient table (MIX_TABLE_FLOATS floats at most) on the device
hipError_t launch_export_mixed(int dtype, int layout, const ExportArgs& a, const float* coef, hipStream_t st);

// resample.hip
hipError_t launch_resample(int dtype, int layout, const ResampleArgs& a, hipStream_t st);
hipError_t launch_resample_mixed(int dtype, int layout, const ResampleArgs& a, const float* coef, hipStream_t st);

// mel.hip: k_mel over rows * a.tiles workgroups; m_tiles is the plan's filter tile count (1, 2, 4 or 8)
hipError_t launch_mel(int dtype, int layout, uint32_t m_tiles, const MelArgs& a, uint64_t rows, hipStream_t st);
// k_mel_ex (lengths, reflect padding, the row maximum) over the same grid (framed: as for
// launch_mel_split below); k_mel_norm over a.total passes
hipError_t launch_mel_ex(int dtype, int layout, uint32_t m_tiles, bool framed, const MelExArgs& e, uint64_t rows,
                         hipStream_t st);
hipError_t launch_mel_norm(int dtype, const MelNormArgs& a, hipStream_t st);

// mel_bf16.hip: k_mel_split, the tile of k_mel_ex with the first product on split bf16 operands;
// terms is 6 (ZFLAC_MEL_MATH_BF16X6) or 3 (_BF16X3). Serves both run calls (the plain one passes
// no lengths, no row maximum and ZFLAC_PAD_ZEROS). framed: the plan's frame is not the whole
// DFT in STFT framing (MelPlan::framed): the instantiations with a signed start offset, the DFT
// size's reflect bound and ZFLAC_PAD_MIRROR; the others are the kernel as it was.
hipError_t launch_mel_split(int dtype, int layout, uint32_t m_tiles, uint32_t terms, bool framed, const MelSplitArgs& s,
                            uint64_t rows, hipStream_t st);

// mel_cmvn.hip: k_mel_cmvn over a.total passes, at most 2^31 - 1 workgroups
hipError_t launch_mel_cmvn(int dtype, int layout, const MelCmvnArgs& a, hipStream_t st);

// cepstra.hip: k_mel_dct and k_mel_delta over a.total passes, at most 2^31 - 1 workgroups
hipError_t launch_mel_dct(int in_dtype, int out_dtype, int layout, const MelDctArgs& a, hipStream_t st);
hipError_t launch_mel_delta(int dtype, int layout, const MelDeltaArgs& a, hipStream_t st);

}  // namespace zflac
