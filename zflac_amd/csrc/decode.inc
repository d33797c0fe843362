// decode.inc -- the hot path: subframe decode kernels, lane per subframe.
//
// Included by decode_k{0,1,2}_{stereo,mono,multi}.hip: one translation unit per SampleType
// container (i8 / i16 / i32; src/zflac.zig:255-265) and channel layout; the stereo units
// also instantiate k_walk.
//
// Wave mapping: 64 lanes = F frames x C channels (F = 64 / C): lane = c * F + j.
// Stereo: lanes 0-31 channel 0, lanes 32-63 channel 1 of the same 32 frames, so the
// partner of a lane is lane ^ 32 and stereo decorrelation is one v_permlane32_swap.
//
// Two kernels per frame batch: (1) k_walk, one lane per frame: subframe c+1 starts where
// subframe c ends, so the lane parses subframes 0..C-2 without producing samples and
// records where each later subframe starts (DecodeArgs::sub_start); (2) k_decode, every
// lane decodes its subframe: header, warm-up, Rice / escape residuals (two Rice codes per
// window step while k <= PAIR_KMAX), fixed / LPC rollback in registers (packed i16 LPC via
// v_dot2), wasted bits, decorrelation, left-justify, packed stores.
//
// Lane input: a per-lane 64-word ring in LDS holding the stream byte-swapped (MSB first); a
// peek reads the two ring words around the bit position and joins them with one v_alignbit,
// and the position is one register (Rdr::nb), so a consume is one subtraction. The ring is
// topped up at chunk starts (CHUNK = 32 samples): the buffer loads staged by the previous
// top-up are stored into the ring and the next ones issued, so every load has a chunk or
// more to land and the per-sample work is ALU + LDS reads. A lane that would run its ring
// dry redoes the chunk on the generic path (synchronous refills).

// Ring quads per lane: 16 (64 words, 16 KiB per wave) by default; the 32-bit-container units
// (decode_k2_*.hip) define 32 (128 words, 32 KiB per wave): at 17..32 bits per sample a chunk
// reads up to ~24 words, which a 64-word ring cannot keep stored ahead while the next top-up is
// in flight (the 32-bit row redid 87 % of its chunks on the generic path, dry).
#ifndef ZFLAC_RING_Q
#define ZFLAC_RING_Q 16
#endif

#include "decode/config.h"        // constants, enums, Kind<> (device_common.h), static_for
#include "decode/lane_reader.h"   // Rdr: bit reader over the LDS ring, top-up
#include "decode/pcm_stage.h"     // Pend, Stage, decorrelation, topup_st
#include "decode/predictor.h"     // Pred
#include "decode/subframe.h"      // LaneCtx, headers, generic Rice reads, walk_subframe
#include "decode/chunk.h"         // slow_chunk, rice_step, walk_chunk, fast_chunk and its forms
#include "decode/run_subframe.h"  // the chunk loop and its dispatch, ChunkProbe
#include "decode/kernels.h"       // setup_frame, k_walk, k_decode, launch_*
