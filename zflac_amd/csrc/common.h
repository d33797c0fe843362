// common.h -- descriptors shared by the host units (stream_plan.cpp, pipeline.cpp,
// seq_planner.cpp, md5_host.cpp, abi.cpp) and the HIP kernels (the .hip units). Plain
// structs, identical layout on both sides; no HIP header, so plain C++ can include it.
#pragma once
#include <cstdint>

// Functions the host and the kernels share: both under hipcc, plain C++ elsewhere.
#ifdef __HIPCC__
#define ZFLAC_HD __host__ __device__
#else
#define ZFLAC_HD
#endif

namespace zflac {

enum Err : int {
    E_OK = 0,
    E_INVALID_SIGNATURE = 1,
    E_INVALID_METADATA_HEADER = 2,
    E_MISSING_STREAMINFO = 3,
    E_UNIMPLEMENTED = 4,
    E_INVALID_CHECKSUM = 5,
    E_INVALID_FRAME_HEADER = 6,
    E_INCONSISTENT_PARAMETERS = 7,
    E_INVALID_CODED_NUMBER = 8,
    E_INVALID_SUBFRAME_HEADER = 9,
    E_INVALID_RESIDUAL_CODING = 10,
    E_END_OF_STREAM = 11,
    E_OUT_OF_MEMORY = 12,
    E_DEVICE = 13,
    E_INVALID_ARGUMENT = 14,
    E_OUT_OF_DOMAIN = 15,
    E_FRAME_CRC = 16,  // frame CRC-16 mismatch: only with ZFLAC_FLAG_CHECK_CRC16 (zflac never checks it)
};

// One stream of a batch, as the kernels see it. Byte offsets are absolute in the
// batch's input buffer; sample offsets are absolute element indices in the batch's
// output buffer (one SampleType per element).
struct StreamDesc {
    uint64_t in_begin;     // first frame header (right after the metadata blocks)
    uint64_t in_end;       // end of the stream bytes
    uint64_t out_base;     // first output element of this stream
    uint64_t out_cap;      // output elements reserved for this stream
    uint64_t total;        // STREAMINFO total samples * channels (0 when unknown)
    uint32_t rate_hz;      // sample rate of the first frame (consistency filter)
    uint32_t si_rate;      // STREAMINFO sample rate (frame rate code 0)
    uint32_t first_chunk;  // chunk range of this stream in the sync-scan chunk table
    uint32_t end_chunk;    // one past the last chunk
    uint8_t byte1;         // 0xF8 / 0xF9 of the first frame (blocking strategy)
    uint8_t nch;           // channel count of the first frame (== STREAMINFO)
    uint8_t dcode;         // bit-depth code of the first frame
    uint8_t si_bps;        // STREAMINFO bits per sample
    uint8_t valid_total;   // STREAMINFO total samples > 0
    uint8_t justify;       // left-justify shift applied at pack-out (src/zflac.zig:287-306)
    uint8_t pad_[2];
};

struct ChunkDesc {
    uint64_t begin;   // absolute byte range scanned for frame-sync candidates
    uint64_t end;
    uint32_t stream;
    uint32_t pad_;
};

// c_info packing for a decoded candidate frame
//   bits  0..15  block size - 1
//   bits 16..19  channel assignment code
//   bits 20..22  bit-depth code
//   bit  28      the frame error arose in the header before the consistency checks
//   bit  29      the header's CRC-8 byte is missing (EndOfStream after the checks)
constexpr uint32_t INFO_PRE_ERR = 1u << 28;
constexpr uint32_t INFO_CRC_EOF = 1u << 29;

constexpr int SCAN_THREADS = 256;
#ifndef ZFLAC_SCAN_BPT
#define ZFLAC_SCAN_BPT 128
#endif
constexpr int SCAN_BYTES_PER_THREAD = ZFLAC_SCAN_BPT;
constexpr uint64_t CHUNK_BYTES = (uint64_t)SCAN_THREADS * SCAN_BYTES_PER_THREAD;  // 32 KiB by default
constexpr int CHUNK_CAP = 64;           // candidates kept per chunk by the scan pass
constexpr uint64_t INPUT_PAD = 4096;    // zero bytes after the last stream
constexpr int MAX_CH = 8;               // FLAC channel limit; k_walk's per-frame record stride
// Launches walking fewer (frames x leading subframes) than this use k_walk_wave (a wave per
// frame) instead of k_walk (a lane per frame): below it k_walk leaves most SIMDs idle.
#ifndef ZFLAC_WAVE_WALK_MAX_FRAMES
#define ZFLAC_WAVE_WALK_MAX_FRAMES 16384
#endif
constexpr uint64_t WAVE_WALK_MAX_FRAMES = ZFLAC_WAVE_WALK_MAX_FRAMES;
constexpr uint64_t DUMMY_BYTES = 64 * 64 * 32;  // 64 wave slots x 64 lanes x 2 quads
constexpr uint64_t PROBE_BYTES = 256;           // after the dummy region: timing-probe builds only

struct ScanArgs {
    const uint8_t* in;
    const StreamDesc* streams;
    const ChunkDesc* chunks;
    uint32_t n_chunks;
    uint32_t* chunk_cnt;        // candidates per chunk (exact)
    unsigned long long* chunk_units;  // sum of block_size*channels per chunk
    uint64_t* chunk_slots;      // CHUNK_CAP positions per chunk
    uint32_t* chunk_slot_units; // CHUNK_CAP units per chunk
    // the run's per-stream status words and its 4 counters, zeroed by k_scan (instead of two
    // fill launches per run); k_verify and later kernels of the run accumulate into them
    uint32_t* status;
    uint32_t n_status;
    uint32_t* misc;
};

// k_hop (hop.hip): the frame table of a class of many short fixed-blocking streams with known
// totals, found by hopping from header to header (one entry per stream, beside StreamDesc).
struct HopDesc {
    uint32_t n_frames;  // ceil(total / block): the frames zflac reads (src/zflac.zig:341)
    uint32_t f0;        // the stream's first index in the class's frame table
    uint32_t units;     // block size * channels: output elements of every frame but the last
    uint32_t guess;     // the first hop's size guess: frame bytes / n_frames
};
static_assert(sizeof(HopDesc) == 16, "HopDesc is the 16-byte record host and kernel share");

// A class takes the hop front when every stream has at most HOP_MAX_FRAMES frames and the class
// at least HOP_MIN_STREAMS streams (stream_plan.h: plan_hop); measured, DESIGN.md §5.3.
#ifndef ZFLAC_HOP_MAX_FRAMES
#define ZFLAC_HOP_MAX_FRAMES 64
#endif
#ifndef ZFLAC_HOP_MIN_STREAMS
#define ZFLAC_HOP_MIN_STREAMS 768
#endif
constexpr uint32_t HOP_MAX_FRAMES = ZFLAC_HOP_MAX_FRAMES;
constexpr uint32_t HOP_MIN_STREAMS = ZFLAC_HOP_MIN_STREAMS;

struct HopArgs {
    const uint8_t* in;
    const StreamDesc* streams;
    const HopDesc* hop;
    uint32_t n_streams;
    uint32_t total_frames;  // sum of n_frames: the run's frame count, written to misc[0]
    uint32_t cap;           // candidate table capacity
    uint32_t epoch;         // nonzero, new for every run: misc[3] == epoch means a hop of this run failed
    uint64_t* c_pos;
    uint32_t* c_stream;
    uint64_t* c_out;
    uint32_t* chunk_off;    // [first_chunk] and [end_chunk] of every stream: its table range (k_verify)
    uint32_t* status;       // per stream: 0, or 2 where the hop failed
    uint32_t* misc;         // the run's 4 counters: [0] frames, [1] overflow = 0, [2] buckets = 0, [3] see epoch
};

struct CompactArgs {
    const uint8_t* in;
    const StreamDesc* streams;
    const ChunkDesc* chunks;
    uint32_t n_chunks;
    const uint32_t* chunk_cnt;
    const uint64_t* chunk_slots;
    const uint32_t* chunk_slot_units;
    const uint32_t* chunk_off;             // exclusive scan of chunk_cnt (n_chunks + 1)
    const unsigned long long* chunk_uoff;  // exclusive scan of chunk_units (n_chunks + 1)
    uint32_t cap;                          // candidate table capacity
    uint64_t* c_pos;
    uint32_t* c_stream;
    uint64_t* c_out;
    uint32_t* overflow;                    // set when the table is too small
};

struct DecodeArgs {
    const uint8_t* in;
    uint64_t in_size;          // bytes of `in`, INPUT_PAD included
    void* out;
    const StreamDesc* streams;
    const uint64_t* c_pos;
    const uint32_t* c_stream;
    const uint64_t* c_out;
    const uint32_t* n_frames;  // device count (fast path) ...
    uint32_t n_frames_host;    // ... or host count when n_frames == nullptr
    uint32_t cap;
    uint64_t* c_end;
    int32_t* c_err;
    uint32_t* c_info;
    uint32_t* c_rate;
    int nch;
    int write;
    void* dummy;  // DUMMY_BYTES: target of masked-off / pending-less packed stores
    uint32_t* sub_start;  // [frame][MAX_CH]: bit offset of subframe c >= 1 (k_walk -> k_decode)
    uint32_t* group_mb;   // [frame group of a k_decode wave]: its history bucket, written by the
                          // first bucket launch so the later launches skip other groups cheaply
    uint32_t* bucket_used;  // optional: the first bucket launch ORs in bucket_bit() of every group
    uint32_t full_mask;     // host only: bucket_bit()s that get their own launch, with a grid
                            // covering every frame group (the order-8 launch, which classifies
                            // every group, and the buckets the host predicts from the input
                            // bytes); 0 = every bucket
    uint32_t rest;          // set on the `rest` launch (of the most general kernel, order 32 with
                            // constant / verbatim lanes) that decodes the frame groups of every
                            // bucket outside full_mask
    uint32_t rest_only;     // host only: launch nothing but the rest kernel (no walk, no bucket
                            // kernels). The normal launch never includes it: the host issues it
                            // after a run whose order-8 launch reported a bucket outside
                            // full_mask (bucket_used), so a correct prediction costs no launch
    uint32_t wb_bytes;      // bytes of `out` (16-byte aligned, at most WB_RSRC_MAX) that the staged 16-bit
                            // write-back may address through a buffer resource; 0: through the pointer
                            // (larger outputs, the sequential path's sub-ranges, ZFLAC_STAGE_WB=ptr)
};
// A masked row of the resource write-back stores at an offset with bit 31 set, which must lie
// past the resource for the buffer unit to drop it.
constexpr uint64_t WB_RSRC_MAX = 0x80000000ull;

// Grid (workgroups) of the `rest` launch: a few waves striding over the frame groups (the
// groups of unpredicted buckets; a misprediction costs time, never correctness).
constexpr uint32_t SPARSE_DECODE_BLOCKS = 256;

// Bit of a k_decode launch (history bucket MB, MIX kernels) in DecodeArgs::bucket_used /
// full_mask: 8 -> 1, 4 -> 2, 16 -> 4, 32 -> 8, MIX 8 -> 16, MIX 32 -> 32, 12 -> 64. The order-8 launch
// always runs (it classifies every wave).
ZFLAC_HD inline constexpr uint32_t bucket_bit(uint32_t mb, bool mix) {
    return mix ? (mb <= 8 ? 16u : 32u)
               : (mb == 8 ? 1u : (mb == 4 ? 2u : (mb == 16 ? 4u : (mb == 12 ? 64u : 8u))));
}
constexpr uint32_t BUCKET_MASK_ALL = 127u;

// One stream for k_md5 (md5.hip): the message is the decoded samples before left-justify,
// rebuilt from the justified device samples (src/zflac.zig:267-280).
enum Md5Mode : uint32_t {
    MD5_RAW = 0,        // bytes as stored (8-bit, 16-bit, 32-bit containers with no justify)
    MD5_S16_SHIFT = 1,  // i16 samples >> js (9..15-bit)
    MD5_S32_SHIFT = 2,  // i32 samples >> js, 4 bytes each (25..31-bit)
    MD5_S24 = 3,        // i32 samples >> js, 3 low bytes each (17..24-bit)
};

struct Md5Job {
    const uint8_t* data;     // device samples of the stream
    uint64_t n;              // samples
    uint32_t mode;           // Md5Mode
    uint32_t js;             // justify shift to undo
    uint32_t width;          // message bytes per sample (1, 2, 3 or 4)
    uint32_t pad_;
    const uint32_t* status;  // optional: the stream's k_verify status; nonzero = not certified by
                             // this run (the sequential planner decodes it later), no hash
};

// The hash kernel a launch took (launch_md5, launch_md5_multi), as zflac_hip_batch_md5_stats
// reports it: ZFLAC_MD5_K_* of zflac_hip.h.
enum Md5Kernel : uint32_t {
    MD5_K_COOP = 1,   // k_md5_coop<MODE>
    MD5_K_MULTI = 2,  // k_md5_multi
    MD5_K_LANE = 4,   // k_md5
};

// Jobs of several runs for one k_md5_multi launch (the md5 hub, md5_host.cpp): segment s is
// jobs[s][0 .. start[s+1] - start[s]), its digests go to dig[s].
constexpr int MD5_MAX_SEGS = 16;
struct Md5Segs {
    const Md5Job* jobs[MD5_MAX_SEGS];
    uint32_t* dig[MD5_MAX_SEGS];
    uint32_t start[MD5_MAX_SEGS + 1];
    uint32_t nseg;
};

struct VerifyArgs {
    const StreamDesc* streams;
    uint32_t n_streams;
    const uint32_t* chunk_off;  // per-chunk candidate offsets (n_chunks + 1)
    const uint64_t* c_pos;
    const uint32_t* c_stream;
    const uint64_t* c_out;
    const uint32_t* n_frames;
    uint32_t cap;
    const uint64_t* c_end;
    const int32_t* c_err;
    const uint32_t* c_info;
    const uint32_t* c_rate;
    uint32_t* status;           // per stream: nonzero => take the sequential path
    uint64_t* units;            // per stream, STREAMINFO total unknown: the chain's output elements
                                // (written by its last frame; nullptr when every total is known)
};

// k_sync_list (scan.hip): sync codes in [lo, hi) with a parseable header matching the
// stream's first frame (channels, depth code, rate), for the sequential planner.
struct SyncListArgs {
    const uint8_t* in;
    uint64_t lo, hi;       // absolute byte range to search
    uint64_t in_end;       // end of the stream's bytes
    uint32_t si_rate;      // STREAMINFO rate (rate code 0)
    uint32_t rate_hz;      // the first frame's rate
    uint32_t nch, dcode;   // the first frame's channel count and depth code
    uint64_t* pos;         // out: positions (unordered)
    uint32_t* count;       // out: number found (may exceed cap)
    uint32_t cap;
};

// k_crc16 (crc16.hip): frame f covers bytes [pos[f], end[f] - 2) with its CRC-16 trailer at
// end[f] - 2 (c_end as k_decode records it). Frames with err[f] != 0 are skipped.
struct Crc16Args {
    const uint8_t* in;
    uint64_t in_size;
    const uint64_t* pos;
    const uint64_t* end;
    const int32_t* err;        // optional
    // optional (the parallel pass): candidates at or past their stream's STREAMINFO total are
    // not checked (zflac stops reading there, src/zflac.zig:341)
    const StreamDesc* streams;
    const uint32_t* c_stream;
    const uint64_t* c_out;
    const uint32_t* n_frames;  // device count ...
    uint32_t n_frames_host;    // ... or host count when n_frames == nullptr
    uint32_t cap;
    uint32_t* bad;             // per frame: 1 when the stored CRC-16 differs
};

// k_export (export.hip): one row of the dense destination. Row i takes frames
// [start, start + T) of its stream; src == nullptr (an error stream, no frames, or a window
// wholly past the end) makes the row all zero.
struct ExportRow {
    const void* src;    // the stream's decoded samples: interleaved, left-justified, container-typed
    uint64_t n_frames;  // frames of the stream
    uint64_t start;     // first frame of the window (< n_frames when src != nullptr)
    uint8_t nch;        // channels of the stream
    uint8_t kind;       // ZFLAC_S8 / ZFLAC_S16 / ZFLAC_S32 container
    uint16_t mix;       // the mixed exports: where the row's matrix (C x nch floats, row-major) starts in
                        // the call's coefficient table, in floats; 0 = none (the fit rule)
    uint8_t pad_[4];
};
static_assert(sizeof(ExportRow) == 32, "ExportRow is the 32-byte record host and kernel share");

constexpr uint32_t EXPORT_THREADS = 256;
constexpr uint32_t EXPORT_GROUP = 16;  // frames (or flat elements) per lane
constexpr uint64_t EXPORT_TILE = (uint64_t)EXPORT_THREADS * EXPORT_GROUP;  // frames of a row per workgroup

struct ExportArgs {
    const ExportRow* rows;
    void* dst;             // B x C x T elements of the export's dtype
    uint64_t frames;       // T
    uint32_t channels;     // C
    uint32_t n_rows;       // B
    uint32_t tiles;        // tiles per row: ceil(T / EXPORT_TILE); grid = n_rows * tiles
    uint32_t vec;          // dst and its rows are 16-byte aligned: the 16-byte store paths apply
};

// The coefficient table of a mixed export (k_export_mixed, k_resample_mixed): float 0 is unused
// (offset 0 means "no matrix"), then one C x n matrix for every channel count n = 1..8 that has
// one: at most 1 + 36 * 8 floats. It lies behind the row records in the same device buffer.
constexpr uint32_t MIX_MAX_CH = 8;  // C and n of a matrix, at most
constexpr uint32_t MIX_TABLE_FLOATS = 1 + 36 * MIX_MAX_CH;

// k_resample (resample.hip): one row of the resampled dense destination. `e` is the row as
// k_export sees it, with e.start and the window counted in frames of the RESAMPLED stream and
// e.n_frames in frames of the source. taps == nullptr: the row is not filtered (its stream
// already has the target rate, ended in an error, or the window lies past its end) and takes
// k_export's paths on `e` as it stands. Otherwise output frame m is
//   sum_k taps[((m * M) mod L) * K + k] * x[floor(m * M / L) - W + k]      (resample_plan.h)
// and a workgroup takes `tile` output frames of the row, `cg` channels at a time (a frame's cg
// channels lie side by side in LDS: one 4-, 8- or 16-byte read).
struct ResampleRow {
    ExportRow e;
    const float* taps;  // h[L][K] in device memory
    uint64_t n_out;     // frames of the resampled stream: ceil(e.n_frames * L / M)
    uint32_t L, M;      // target rate / gcd, source rate / gcd
    uint32_t W, K;      // half width and tap count, K = 2 W + 1
    uint32_t tile;      // output frames per workgroup (resample_tile)
    uint8_t cg;         // channels staged and summed together: 1, 2 or 4 (RESAMPLE_MAX_CG)
    uint8_t tab_lds;    // the workgroup copies the table into LDS (else it reads taps from global memory)
    uint8_t pad_[2];
};
static_assert(sizeof(ResampleRow) == 72, "ResampleRow is the 72-byte record host and kernel share");

// LDS of a k_resample workgroup, in floats: 80 KiB, so that two workgroups (16 waves) share a CU's
// 160 KiB.
// A table of at most RESAMPLE_LDS_TABLE floats is kept there, in front of the staged input span,
// which takes the rest (at least 14 KiB; all 80 KiB when the taps are read from global memory).
constexpr uint32_t RESAMPLE_THREADS = 512;  // (the rows on k_export's paths use the first EXPORT_THREADS)
constexpr uint32_t RESAMPLE_LDS_FLOATS = 20480;
constexpr uint32_t RESAMPLE_LDS_TABLE = 16896;
constexpr uint32_t RESAMPLE_MAX_TILE = 2048;  // output frames of a row per workgroup, at most
constexpr uint32_t RESAMPLE_MAX_CG = 4;

struct ResampleArgs {
    const ResampleRow* rows;
    void* dst;             // B x C x T elements of the export's dtype
    uint64_t frames;       // T, in frames of the resampled streams
    uint32_t channels;     // C
    uint32_t n_rows;       // B
    uint32_t tiles;        // workgroups per row: the most any row needs (ceil(T / its tile))
    uint32_t vec;          // as ExportArgs::vec, for the rows on k_export's paths
};

// k_mel (mel.hip): log-mel features of dense f32 rows. A workgroup of MEL_WAVES waves takes
// MEL_FRAMES feature frames of one row, a wave MEL_TILE of them (the lanes of its MFMA tiles);
// the frames' samples and the basis go through LDS in slabs of MEL_SLAB samples. The tables'
// layouts and the grid rule are mel_plan.h's.
constexpr uint32_t MEL_TILE = 32;                            // edge of an MFMA tile: bins, filters, frames
constexpr uint32_t MEL_WAVES = 4;
constexpr uint32_t MEL_THREADS = 64 * MEL_WAVES;
constexpr uint32_t MEL_FRAMES = MEL_TILE * MEL_WAVES;        // feature frames of a row per workgroup
constexpr uint32_t MEL_SLAB = 64;                            // samples of every frame staged at a time
constexpr uint32_t MEL_PAIR_STRIDE = 2 * MEL_FRAMES + 16;    // floats of LDS per sample pair of the staged frames
constexpr uint32_t MEL_LDS_FLOATS = MEL_SLAB * 2 * MEL_TILE + (MEL_SLAB / 2) * MEL_PAIR_STRIDE;

// Row of a 32 x 32 MFMA accumulator that register r holds in lanes 0..31 (lanes 32..63: + 4).
// The kernels' epilogue (mel_tile.h) and the filter table's layout (mel_plan.cpp) both go by it.
constexpr uint32_t mel_acc_row(uint32_t r) { return (r & 3) + 8 * (r >> 2); }

struct MelArgs {
    const float* wave;     // rows of row_stride floats
    const float* basis;    // mel_plan.h: [bin tile][sample pair][re, im][sample of the pair][bin]
    const float* filters;  // mel_plan.h: [bin tile][accumulator register][filter tile][lane]
    void* dst;             // rows x n_bins x frames (or rows x frames x n_bins) elements of the dtype
    uint64_t wave_frames;  // samples of a row; zero outside
    uint64_t row_stride;
    uint64_t first_frame;  // feature frame of destination frame 0
    uint64_t frames;       // destination frames per row
    uint32_t tiles;        // workgroups per row: ceil(frames / MEL_FRAMES); grid = rows * tiles
    uint32_t span, hop;    // samples of a frame the sums run over (N; a framed plan: Nw, padded as its table), hop
    int32_t off;           // frame t starts at sample t * hop - off (center ? N / 2 : 0; a framed plan: mel_plan.h)
    uint32_t n_bins;       // rows of the filterbank
    uint32_t bin_tiles;    // ceil((N / 2 + 1) / MEL_TILE), N the DFT size
    uint32_t scale;        // ZFLAC_MEL_POWER / _LOG10 / _LN
    float floor;
};

// What zflac_hip_mel_run_ex adds to a launch of k_mel (its EX instantiations), and k_mel_norm.
struct MelExArgs {
    MelArgs a;
    const uint64_t* lengths;  // per row, clamped to a.wave_frames; NULL = a.wave_frames
    float* row_max;           // per row, -inf before the launch; NULL = not wanted
    uint32_t pad;             // ZFLAC_PAD_ZEROS / _REFLECT / _MIRROR
    uint32_t pad_half;        // _REFLECT: the padded signal is [-pad_half, n_i + pad_half): half the DFT size
};

// k_mel_split (mel_bf16.hip): the first product on the bf16 matrix cores with both operands split
// into bf16 pieces (ZFLAC_MEL_MATH_BF16X6 / _BF16X3). The tile is k_mel's (MEL_FRAMES frames, a
// wave MEL_TILE of them); the samples go in blocks of MEL_BF16_K, the bin tiles in groups of
// MEL_BF16_GROUP whose accumulators are live together. The piece table's layout is mel_plan.h's.
constexpr uint32_t MEL_BF16_K = 16;                          // samples per v_mfma_f32_32x32x16_bf16
constexpr uint32_t MEL_BF16_GROUP = 2;                       // bin tiles per pass over the samples
constexpr uint32_t MEL_BF16_OPERAND = 64 * 8;                // bf16 of one A operand: 64 lanes x 8

struct MelSplitArgs {
    MelExArgs e;              // e.a.basis is unused (NULL): a split plan has no f32 basis table
    const uint16_t* pieces;   // mel_plan.h: [group][sample block][bin tile of the group][re, im][piece][lane][8]
    uint32_t k_blocks;        // ceil(N / MEL_BF16_K)
};

constexpr uint32_t MEL_NORM_THREADS = 256;
constexpr uint32_t MEL_NORM_CHUNK = 4096;  // elements of one row per workgroup pass

struct MelNormArgs {
    void* dst;             // rows x row_elems elements of the dtype (either layout: a row is contiguous)
    const float* row_max;
    uint64_t row_elems;    // n_bins * frames
    uint64_t chunks;       // per row: ceil(row_elems / MEL_NORM_CHUNK)
    uint64_t total;        // rows * chunks
    float range, add, mul;
};

// k_mel_cmvn (mel_cmvn.hip): per (row, bin) mean / variance normalisation over the valid frames,
// in place. Bins-first: a workgroup pass takes one (row, bin), frames contiguous elements.
// Frames-first: a pass takes one row, the bins on the lanes.
constexpr uint32_t MEL_CMVN_THREADS = 256;

struct MelCmvnArgs {
    void* feat;             // rows x n_bins x frames (or rows x frames x n_bins) elements of the dtype
    const uint64_t* valid;  // per row, clamped to frames; NULL = frames
    float* mean;            // rows x n_bins, or NULL
    float* std;             // rows x n_bins, or NULL
    uint64_t rows, frames;
    uint64_t total;         // passes: rows * n_bins (bins first) or rows (frames first)
    uint32_t n_bins;
    uint32_t mode, ddof;    // ZFLAC_CMVN_*; 0 or 1
    float eps, pad_value;
};

// k_mel_dct (cepstra.hip): every frame's n_in bins projected by T to n_out features. A workgroup
// pass takes CEPS_FRAMES frames of one row: the frames' bins go to LDS as f32, then a lane has one
// frame and a wave CEPS_KB output rows at a time, T coming in by scalar loads.
constexpr uint32_t CEPS_THREADS = 256;
constexpr uint32_t CEPS_FRAMES = 64;  // frames of a row per workgroup pass: the lanes of a wave
constexpr uint32_t CEPS_KB = 4;       // rows of T a wave carries at once

struct MelDctArgs {
    const void* src;   // rows x n_in x frames (or rows x frames x n_in) elements of the input dtype
    void* dst;         // rows x n_out x frames (or rows x frames x n_out) elements of the output dtype
    const float* T;    // n_out x n_in, row-major
    uint64_t frames;
    uint64_t tiles;    // passes per row: ceil(frames / CEPS_FRAMES)
    uint64_t total;    // rows * tiles
    uint32_t n_in, n_out;
};

// k_mel_delta (cepstra.hip): Kaldi's deltas of every (row, feature) over the row's valid frames.
// Bins-first: a workgroup pass takes CEPS_THREADS frames of one (row, feature). Frames-first: a
// pass takes CEPS_THREADS / C frames of one row, the features on the lanes (as k_mel_cmvn).
constexpr uint32_t CEPS_MAX_ORDER = 3;
constexpr uint32_t CEPS_MAX_WINDOW = 5;

struct MelDeltaArgs {
    const void* src;        // rows x C x frames (or rows x frames x C) elements of the dtype
    void* dst;              // rows x (order + 1) C x frames (or rows x frames x (order + 1) C)
    const float* scales;    // the taps of order 1, then 2, .. (2 o W + 1 each)
    const uint64_t* valid;  // per row, clamped to frames; NULL = frames
    uint64_t frames;
    uint64_t tiles;         // passes per (row, feature) (bins first) or per row (frames first)
    uint64_t total;         // passes
    uint32_t C, order, window;
    float pad_value;
};

}  // namespace zflac
