/*
 * zflac_hip.h -- C ABI of the MI355X FLAC decode path (libzflac_hip.so).
 *
 * Drop-in boundary for Senryoku/zflac `pub fn decode(allocator, reader) !DecodedFLAC`
 * (src/zflac.zig:216-217). zflac's only entry point reads a whole stream through a
 * std reader and returns caller-owned samples; here the caller hands over the stream
 * bytes and receives the samples in memory it allocated itself (two-phase: open ->
 * size -> read), so a Zig shim can keep `DecodedFLAC` and its allocator contract
 * (src/zflac.zig:18-28, :331). See INTEGRATION.md for the shim.
 *
 * All decode work (frame sync scan, subframe decode, fixed/LPC rollback, wasted bits,
 * stereo decorrelation, left-justify, PCM pack-out) runs in HIP kernels on gfx950.
 * MD5 verification (src/zflac.zig:267-280) runs on the host over the PCM copied back,
 * or, for batches created with ZFLAC_FLAG_DEVICE_MD5, in a HIP kernel (k_md5).
 * There is no CPU decode fallback: without a usable GPU every call returns
 * ZFLAC_E_DEVICE.
 *
 * Thread safety: handles are independent; a handle must not be used by two threads
 * at once. No global mutable state besides a lazily initialised per-device context.
 */
#ifndef ZFLAC_HIP_H
#define ZFLAC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Error codes, 1:1 with zflac's error set. */
#define ZFLAC_OK 0
#define ZFLAC_E_INVALID_SIGNATURE 1         /* src/zflac.zig:220 */
#define ZFLAC_E_INVALID_METADATA_HEADER 2   /* src/zflac.zig:248 */
#define ZFLAC_E_MISSING_STREAMINFO 3        /* src/zflac.zig:309 */
#define ZFLAC_E_UNIMPLEMENTED 4             /* src/zflac.zig:263 */
#define ZFLAC_E_INVALID_CHECKSUM 5          /* src/zflac.zig:280 */
#define ZFLAC_E_INVALID_FRAME_HEADER 6      /* src/zflac.zig:352,357,361,372,405 */
#define ZFLAC_E_INCONSISTENT_PARAMETERS 7   /* src/zflac.zig:386,391 */
#define ZFLAC_E_INVALID_CODED_NUMBER 8      /* src/zflac.zig:206 */
#define ZFLAC_E_INVALID_SUBFRAME_HEADER 9   /* src/zflac.zig:431,471,542 */
#define ZFLAC_E_INVALID_RESIDUAL_CODING 10  /* src/zflac.zig:618 */
#define ZFLAC_E_END_OF_STREAM 11            /* std.io reader EndOfStream */
#define ZFLAC_E_OUT_OF_MEMORY 12            /* allocator OutOfMemory */
#define ZFLAC_E_DEVICE 13                   /* HIP runtime failure / no GPU (no zflac equivalent) */
#define ZFLAC_E_INVALID_ARGUMENT 14         /* bad handle, index or buffer size */
#define ZFLAC_E_OUT_OF_DOMAIN 15            /* input on which Debug zflac traps */
#define ZFLAC_E_FRAME_CRC 16                /* frame CRC-16 mismatch, only with ZFLAC_FLAG_CHECK_CRC16 */

/* Arm of zflac's `Samples` union (src/zflac.zig:12-16). */
#define ZFLAC_S8 0
#define ZFLAC_S16 1
#define ZFLAC_S32 2

/* Mirrors the scalar fields of zflac.DecodedFLAC (src/zflac.zig:18-23). */
typedef struct zflac_info {
    uint8_t channels;        /* DecodedFLAC.channels */
    uint8_t bits_per_sample; /* DecodedFLAC.bits_per_sample */
    uint8_t sample_kind;     /* ZFLAC_S8 / ZFLAC_S16 / ZFLAC_S32 */
    uint8_t reserved;
    uint32_t sample_rate;    /* DecodedFLAC.sample_rate (u24 in zflac) */
    uint64_t n_samples;      /* samples.len: interleaved channel-samples */
    uint64_t samples_bytes;  /* n_samples * sizeof(SampleType) */
} zflac_info;

/* One input stream: a complete FLAC byte stream in host memory. */
typedef struct zflac_stream {
    const uint8_t *data;
    size_t len;
} zflac_stream;

/* Per-kernel device time of the last zflac_hip_batch_run (HIP events on the
 * library's stream). */
typedef struct zflac_timings {
    double scan_ms;     /* frame-sync scan + candidate compaction */
    double decode_ms;   /* subframe decode kernel k_decode (the hot path) */
    double verify_ms;   /* chain verification */
    double total_ms;    /* first launch -> last event */
    uint64_t frames;        /* frames decoded */
    uint64_t input_bytes;   /* compressed frame bytes of decoded frames */
    uint64_t output_bytes;  /* PCM bytes written */
    uint64_t samples;       /* channel-samples written */
    double walk_ms;     /* subframe-start walk k_walk (2+ channels; runs before k_decode) */
    double md5_ms;      /* batched STREAMINFO MD5 k_md5 (ZFLAC_FLAG_DEVICE_MD5), else 0 */
    /* host wall-clock times (steady clock), recorded whether or not ZFLAC_FLAG_TIMING is set */
    double plan_ms;     /* batch_create / open: metadata and first-frame parse */
    double upload_ms;   /* batch_create / open: staging + H2D of the compressed bytes, allocations */
    double run_wall_ms; /* last batch_run, launch to results (kernels + read-backs) */
    double read_ms;     /* last batch_read / read: D2H of the samples (+ MD5 overlapped) */
    double host_md5_ms; /* last batch_read / read: host STREAMINFO MD5 (overlapped with the D2H) */
    double crc16_ms;    /* k_crc16 of the last run (ZFLAC_FLAG_CHECK_CRC16 with ZFLAC_FLAG_TIMING), else 0 */
    /* (ABI 4) synchronous `rest` decode launches of the last run: frame groups of a k_decode
     * history bucket the batch's launch plan had not predicted; the bucket is then added to
     * the plan, so a later run of the same batch has none */
    uint32_t rest_launches;
    /* (ABI 5) streams of the last run finished by the sequential chain planner, because the
     * parallel pass's chain check (k_verify) did not certify them: a stream that ends in an
     * error (a broken or truncated frame, frames that disagree with STREAMINFO), candidates
     * that do not form one chain up to the STREAMINFO total (false syncs the check could not
     * rule out, missing or extra frames), or a batch created with ZFLAC_FLAG_FORCE_SLOW. A
     * stream whose STREAMINFO total is unknown is certified by the parallel pass like any
     * other; it reaches the planner only through a broken chain, bytes after its last frame,
     * or an output reservation dropped at creation (a flood of false syncs, the memory cap).
     * 0 when the parallel pass certified every stream */
    uint32_t sequential_streams;
} zflac_timings;

typedef struct zflac_batch zflac_batch;

/* ---- single stream: the decode(allocator, reader) replacement --------------- */
/* Decode `buf` on `device`. On success *out_batch holds the decoded stream and
 * *info its shape (allocate info->samples_bytes, 32-byte aligned as zflac does,
 * then call zflac_hip_read). The returned code is the zflac error of the stream
 * (MD5 is checked by zflac_hip_read). */
int zflac_hip_open(const uint8_t *buf, size_t len, int device, zflac_batch **out_batch, zflac_info *info);
/* zflac_hip_open with batch flags (ZFLAC_FLAG_CHECK_CRC16, ZFLAC_FLAG_TIMING). */
int zflac_hip_open_ex(const uint8_t *buf, size_t len, int device, int flags, zflac_batch **out_batch,
                      zflac_info *info);
/* Copy the samples into caller memory, verify the STREAMINFO MD5
 * (ZFLAC_E_INVALID_CHECKSUM on mismatch, as src/zflac.zig:279-280), left-justify is
 * already applied on the device (src/zflac.zig:287-306). Long streams are copied back in
 * chunks while a host thread hashes the chunks already landed (MD5 is one serial chain per
 * stream, so it bounds this call). */
int zflac_hip_read(zflac_batch *b, void *out_samples, size_t out_bytes);
void zflac_hip_close(zflac_batch *b);

/* ---- batches of independent streams (C5 shard) ------------------------------- */
/* Parse metadata on the host, upload all compressed bytes to HBM and allocate the
 * device output. Streams are referenced, not copied, until this call returns. */
int zflac_hip_batch_create(const zflac_stream *streams, size_t n, int device, int flags, zflac_batch **out);
/* One device-resident decode of every stream of the batch (inputs already in HBM,
 * outputs left in HBM). Synchronous. Returns ZFLAC_OK or ZFLAC_E_DEVICE; per-stream
 * zflac errors are reported by zflac_hip_batch_info. */
int zflac_hip_batch_run(zflac_batch *b);
/* zflac_hip_batch_run in two halves, so that runs of different batches overlap on the
 * device: _submit enqueues the run's kernels on the next of the device's run streams
 * (ZFLAC_RUN_STREAMS, default 3) and returns; with ZFLAC_FLAG_DEVICE_MD5 the run's hash
 * goes to the device's md5 hub (one launch over several runs, streams of its own);
 * _wait blocks until they finish and produces the per-stream results (the sequential
 * planner, CRC-16 and MD5 legs run here). A batch has at most one run in flight: _submit
 * on a submitted batch and _wait without one return ZFLAC_E_INVALID_ARGUMENT, and results
 * (_info, _read, ...) are unavailable between the two. Destroying a submitted batch waits
 * for its kernels. */
/* With ZFLAC_FLAG_DEVICE_MD5, _wait of a run whose hash is still queued in the md5 hub
 * flushes the hub: one launch hashes every pending run (up to ZFLAC_MD5_RUNS) and waits on
 * each of their decodes, so the digests of the waited run arrive with the slowest of those
 * runs, and md5_ms reports that shared launch's time. */
int zflac_hip_batch_submit(zflac_batch *b);
int zflac_hip_batch_wait(zflac_batch *b);
/* (ABI 4) Non-blocking: 1 when the device work of the submitted run has finished (so
 * _wait returns without waiting on the GPU), 0 while it runs, -ZFLAC_E_INVALID_ARGUMENT
 * without a submitted run, -ZFLAC_E_DEVICE on a device error. With ZFLAC_FLAG_DEVICE_MD5
 * the run's hash counts as device work (a pending md5 hub launch is flushed when the hub is
 * idle). A caller with several batches
 * in flight waits for whichever is ready instead of the oldest. */
int zflac_hip_batch_ready(zflac_batch *b);
/* Per-stream result of the last run: zflac error code, and shape when OK.
 * Before the first completed run: ZFLAC_E_INVALID_ARGUMENT (as for _read, _md5 and
 * _device_samples, which returns NULL). */
int zflac_hip_batch_info(zflac_batch *b, size_t i, zflac_info *info);
/* Copy stream i's samples to host memory; verify_md5 != 0 checks STREAMINFO MD5. */
int zflac_hip_batch_read(zflac_batch *b, size_t i, void *out, size_t out_bytes, int verify_md5);
/* Device MD5 digest of stream i's samples as zflac hashes them (before left-justify,
 * src/zflac.zig:267-277), computed by the last run when the batch was created with
 * ZFLAC_FLAG_DEVICE_MD5; ZFLAC_E_INVALID_ARGUMENT otherwise. */
int zflac_hip_batch_md5(zflac_batch *b, size_t i, uint8_t *digest16);
/* Device pointer of stream i's samples (valid until the next run / destroy). */
const void *zflac_hip_batch_device_samples(zflac_batch *b, size_t i);
/* Timings of the last run / read. ZFLAC_OK when device timings were recorded
 * (ZFLAC_FLAG_TIMING); the host wall-clock fields are filled either way.
 * _ex copies min(size, sizeof(zflac_timings)) bytes (pass sizeof *t) and zero-fills the
 * rest of a longer struct, so callers built against another version of this header stay
 * within their struct. The legacy entry point writes only the first-version layout
 * (ZFLAC_TIMINGS_V1_SIZE bytes: scan_ms .. md5_ms). */
int zflac_hip_batch_timings(zflac_batch *b, zflac_timings *t);
int zflac_hip_batch_timings_ex(zflac_batch *b, zflac_timings *t, size_t size);
#define ZFLAC_TIMINGS_V1_SIZE 80
/* The k_decode kernels of the last completed run. Every frame group (the frames one decode wave
 * takes: 64 / channels consecutive frames of the batch's streams of one container and channel
 * count) is decoded by the kernel of its history bucket: the smallest of 4, 8, 12, 16, 32 that
 * holds the highest predictor order among the group's subframes, or, when one of them is
 * CONSTANT or VERBATIM, the MIX kernel of 8 or 32. *used: the OR, over the batch's classes, of
 * the ZFLAC_BUCKET_* of every frame group as that run classified them. *planned: the buckets
 * that had a launch of their own when the run was enqueued (predicted at creation from each
 * stream's first subframe, plus what earlier runs found); groups of a bucket in used & ~planned
 * were decoded by the run's `rest` launch (zflac_timings.rest_launches), and the bucket is
 * planned from the next run on. ZFLAC_E_INVALID_ARGUMENT: a NULL batch or pointer, before the
 * first completed run, between _submit and _wait. */
#define ZFLAC_BUCKET_8 1u
#define ZFLAC_BUCKET_4 2u
#define ZFLAC_BUCKET_16 4u
#define ZFLAC_BUCKET_32 8u
#define ZFLAC_BUCKET_MIX_8 16u
#define ZFLAC_BUCKET_MIX_32 32u
#define ZFLAC_BUCKET_12 64u
#define ZFLAC_BUCKET_ALL 127u
int zflac_hip_batch_decode_buckets(zflac_batch *b, uint32_t *used, uint32_t *planned);
/* What built the frame table of the last completed run. The streams of one container and channel
 * count (a class) share a table, found either by k_scan (every input byte searched for frame sync
 * codes) or by k_hop (from each frame header to the next, by the frame number: classes of many
 * short streams with fixed blocking and a STREAMINFO total, see ZFLAC_FLAG_FRONT_*). *planned: the
 * OR, over the batch's classes, of the ZFLAC_FRONT_* each class's run was enqueued with. *used: the
 * same for the table the results came from; a class whose hop lost a stream is redone with the
 * scan front by _wait (planned HOP, used SCAN) and keeps the scan front in later runs. Results
 * never depend on the front. ZFLAC_E_INVALID_ARGUMENT as for _decode_buckets. */
#define ZFLAC_FRONT_SCAN 1
#define ZFLAC_FRONT_HOP 2
int zflac_hip_batch_front(zflac_batch *b, int *planned, int *used);
/* Where stream i's digest (zflac_hip_batch_md5) came from in the last completed run of a
 * ZFLAC_FLAG_DEVICE_MD5 batch:
 *   _NONE          no digest: the stream ended in an error (InvalidChecksum included), or the batch
 *                  has no device MD5;
 *   _PIPELINED     the hash _submit enqueued behind the decode, in the device's md5 hub or (with
 *                  ZFLAC_MD5_NOHUB) on the run stream: the streams the parallel pass certified;
 *   _SYNC          the synchronous hash launch of _wait: streams the sequential planner finished,
 *                  or a class that was run again;
 *   _HOST_RECHECK  the device digest of a left-justified stream (9..15, 17..31 bits) was not
 *                  STREAMINFO's; the stream was decoded again alone, without the shift, hashed on
 *                  the host, and that digest matched (zflac hashes before it left-justifies and keeps
 *                  samples beyond the stream's depth). _md5 then returns STREAMINFO's digest.
 * ZFLAC_E_INVALID_ARGUMENT: a NULL batch or pointer, before the first completed run, i out of range. */
#define ZFLAC_MD5_SRC_NONE 0
#define ZFLAC_MD5_SRC_PIPELINED 1
#define ZFLAC_MD5_SRC_SYNC 2
#define ZFLAC_MD5_SRC_HOST_RECHECK 3
int zflac_hip_batch_md5_source(zflac_batch *b, size_t i, int *source);
/* *kernels: the OR of the ZFLAC_MD5_K_* of the hash launches the last completed run's device
 * digests came from (_PIPELINED and _SYNC streams; a hub launch counts for every run it hashed):
 * k_md5_coop (every job of the launch in one form, cooperative loads through LDS), k_md5_multi
 * (jobs of several forms in one hub launch; also what a k_md5_coop launch falls back to where the
 * device refuses its LDS), k_md5 (a single run's jobs, each lane its own loads). 0 without
 * ZFLAC_FLAG_DEVICE_MD5. *rechecks: over the batch's lifetime, how often a left-justified stream
 * was decoded again to take its digest before the shift, after a mismatch in _wait (see
 * _HOST_RECHECK) or in _batch_read's host hash; a stream inside its depth whose STREAMINFO MD5 is
 * right never counts. ZFLAC_E_INVALID_ARGUMENT as for _decode_buckets. */
#define ZFLAC_MD5_K_COOP 1u
#define ZFLAC_MD5_K_MULTI 2u
#define ZFLAC_MD5_K_LANE 4u
int zflac_hip_batch_md5_stats(zflac_batch *b, uint32_t *kernels, uint64_t *rechecks);
size_t zflac_hip_batch_size(zflac_batch *b);
void zflac_hip_batch_destroy(zflac_batch *b);

/* ---- dense device export --------------------------------------------------------- */
/* The batch's decoded samples as one dense tensor in caller-owned device memory, written by
 * one HIP kernel (k_export): B rows (one per stream, in batch order) of `channels` x `frames`
 * elements. Row i holds frames [starts[i], starts[i] + frames) of stream i. Frames at or
 * past the stream's end and channels the stream does not have are zero; a stream with more
 * than `channels` channels exports its first `channels`; a stream whose result is an error
 * exports an all-zero row. Every element of the destination is written. */
#define ZFLAC_EXPORT_F32 0  /* (float)sample * 2^-(container bits - 1): 2^-7, 2^-15 or 2^-31 (exact;
                               the int->float conversion rounds 25..32-bit samples to nearest-even) */
#define ZFLAC_EXPORT_F16 1  /* that f32 value rounded to nearest-even to IEEE half, subnormals kept */
#define ZFLAC_EXPORT_BF16 2 /* that f32 value rounded to nearest-even to bfloat16 */
#define ZFLAC_EXPORT_I32 3  /* the container value sign-extended (the number zflac_hip_batch_read returns) */
#define ZFLAC_LAYOUT_PLANAR 0      /* [row][channel][frame] */
#define ZFLAC_LAYOUT_INTERLEAVED 1 /* [row][frame][channel] */
typedef struct zflac_export_desc {
    uint32_t size;          /* sizeof(zflac_export_desc) */
    uint8_t dtype, layout;  /* ZFLAC_EXPORT_*, ZFLAC_LAYOUT_* */
    uint16_t channels;      /* C >= 1 */
    uint64_t frames;        /* T >= 1 */
    const uint64_t *starts; /* host array, one per stream, or NULL = all 0 */
} zflac_export_desc;
/* Export the last completed run. dst_device: B * C * T elements of the dtype on the batch's
 * device (any alignment; 16-byte aligned rows take the fast paths). valid_frames (host, B
 * entries, may be NULL) receives clamp(frames of stream i - starts[i], 0, T), 0 for an error
 * stream. stream == NULL: runs on the batch's own stream and returns when the tensor is
 * complete. Otherwise `stream` is a hipStream_t of the batch's device: the export is enqueued
 * there and the call returns without synchronising, so later work on that stream sees the
 * tensor; the batch's next run waits for it on the device, and _destroy on the host.
 * ZFLAC_E_INVALID_ARGUMENT (nothing written): NULL batch / desc / dst, desc->size, an unknown
 * dtype or layout, channels or frames of 0, dst_bytes < B*C*T*element size, before the first
 * completed run, between _submit and _wait. ZFLAC_E_DEVICE on a HIP failure. */
int zflac_hip_batch_export(zflac_batch *b, const zflac_export_desc *d, void *dst_device, size_t dst_bytes,
                           uint64_t *valid_frames, void *stream);
/* Device time of the last synchronous (stream == NULL) export of a batch created with
 * ZFLAC_FLAG_TIMING (table copy + k_export); ZFLAC_E_INVALID_ARGUMENT when there is none. */
int zflac_hip_batch_export_ms(zflac_batch *b, double *ms);

/* ---- dense device export at one sample rate -------------------------------------- */
/* zflac_hip_batch_export with every row resampled to `sample_rate` by one HIP kernel
 * (k_resample), so a batch of mixed-rate streams becomes one tensor with one time base.
 * A stream of rate fin (zflac_info.sample_rate) goes to fout = sample_rate through a polyphase
 * Kaiser-windowed sinc: g = gcd(fin, fout), M = fin / g, L = fout / g,
 * s = min(1, L / M) * rolloff, W = ceil(zeros / s), K = 2 W + 1. Output frame m is
 *   y[m] = sum_{k < K} h[r][k] * x[q - W + k],  q = floor(m M / L), r = (m M) mod L,
 * x the sample as ZFLAC_EXPORT_F32 has it, zero outside the stream, and
 *   h[r][k] = u[r][k] / sum_k u[r][k],  u[r][k] = s sinc(t) kaiser(t),  t = s ((k - W) - r / L),
 *   kaiser(t) = I0(beta sqrt(1 - (t / zeros)^2)) / I0(beta) for |t| < zeros, 0 otherwise
 * (tables in double, rounded once to float; sums in f32 with fused multiply-adds in ascending
 * k, so a frame's value does not depend on the window it is exported in; no renormalisation at
 * the stream's edges). The resampled stream has ceil(frames * L / M) frames. A stream already at
 * `sample_rate` is not filtered: its row is bit-identical to zflac_hip_batch_export's. A stream
 * whose rate is 0 exports a zero row of valid length 0. */
typedef struct zflac_resample_desc {
    uint32_t size;          /* sizeof(zflac_resample_desc) */
    uint8_t dtype, layout;  /* ZFLAC_EXPORT_F32 / _F16 / _BF16 (rounded from the f32 sum as the plain
                               export rounds), ZFLAC_LAYOUT_* */
    uint16_t channels;      /* C >= 1 */
    uint64_t frames;        /* T >= 1, frames of the resampled streams */
    const uint64_t *starts; /* host array, one per stream, in frames of the resampled stream, or NULL */
    uint32_t sample_rate;   /* the target rate, 1 .. 1048575 */
    uint16_t zeros;         /* zero crossings of the sinc on each side, >= 1 (16 is a good default) */
    uint16_t reserved;      /* must be 0 */
    double rolloff;         /* 0 < rolloff <= 1: the cutoff as a fraction of the lower Nyquist rate (0.85) */
    double beta;            /* Kaiser window shape, >= 0 (8.555504641634386) */
} zflac_resample_desc;
/* The contract of zflac_hip_batch_export (destination, stream semantics, channel fitting, zero
 * fill, error rows, every element written), with frames, starts and valid_frames counted in
 * frames of the resampled streams: valid_frames[i] = clamp(ceil(n_i L_i / M_i) - starts[i], 0, T).
 * ZFLAC_E_INVALID_ARGUMENT (nothing written): whatever the plain export rejects,
 * ZFLAC_EXPORT_I32, a sample_rate of 0 or above 1048575, zeros of 0, rolloff or beta out of
 * range, reserved != 0, and two limits of the call: a stream whose K exceeds 4096 taps, and
 * tables (L * K floats per distinct source rate among the streams that are filtered) that
 * together exceed 4 Mi floats. A caller with such streams exports them apart or with a
 * narrower filter. The batch keeps each table it builds in device memory (one per distinct
 * source rate, target rate, zeros, rolloff, beta) until it is destroyed, or until a later
 * call's tables would take it past 4 Mi floats; an export with parameters it has met builds
 * nothing. zflac_hip_batch_export_ms reports the last synchronous export of either kind. */
int zflac_hip_batch_export_resampled(zflac_batch *b, const zflac_resample_desc *d, void *dst_device,
                                     size_t dst_bytes, uint64_t *valid_frames, void *stream);
/* Frames of a stream of n_frames at rate_in once resampled to rate_out: ceil(n_frames * L / M);
 * 0 when either rate is 0. Host arithmetic, no GPU needed. */
uint64_t zflac_hip_resampled_frames(uint64_t n_frames, uint32_t rate_in, uint32_t rate_out);
/* The batch's resampling tables: how many it has built since it was created and how many
 * floats it holds now (either pointer may be NULL). */
int zflac_hip_batch_resample_tables(zflac_batch *b, uint64_t *built, uint64_t *held_floats);

/* ---- channel mixing in the dense exports -------------------------------------------- */
/* zflac_hip_batch_export and zflac_hip_batch_export_resampled with the channels of each stream
 * mixed on the device by a matrix chosen by the stream's channel count, so that a batch of mono,
 * stereo and multichannel streams becomes one tensor of C channels (a mono downmix, a stereo
 * fold-down) in the same one launch (k_export_mixed, k_resample_mixed). */
#define ZFLAC_MIX_MAX_CHANNELS 8
typedef struct zflac_mix_desc {
    uint32_t size;      /* sizeof(zflac_mix_desc): 72 on LP64 */
    uint32_t reserved;  /* must be 0 */
    /* matrix[n - 1]: how streams of n channels are mixed: a host array of C x n floats,
     * row-major (m[c * n + j] = weight of source channel j in output channel c), or NULL:
     * such streams take the plain export's fit rule */
    const float *matrix[8];
} zflac_mix_desc;
/* What stays as in the unmixed call of the same kind (zflac_hip_batch_export for _export_mixed,
 * zflac_hip_batch_export_resampled for _export_resampled_mixed): the destination, the stream
 * semantics, starts, the zero fill, error rows, "every element written" and valid_frames.
 * mix == NULL, or a mix whose eight pointers are all NULL, is that unmixed call in every respect:
 * the same bits, ZFLAC_EXPORT_I32 allowed (plain export), the same errors, the same kernel. A row
 * whose stream has n channels with matrix[n - 1] == NULL has the unmixed call's bits, also when
 * other rows of the same call are mixed.
 *
 * Plain export of a mixed row (a stream whose result is OK, of n channels, matrix[n - 1] == m):
 * output channel c of frame t is v_c[t], computed in f32 as
 *   acc = +0; for j = 0 .. n - 1: acc = fmaf(m[c * n + j], x_j[t], acc)
 * with x_j[t] the sample as ZFLAC_EXPORT_F32 has it; v_c[t] is then rounded to f16 or bf16
 * exactly as the plain export rounds its f32 value. Frames past the stream's end are +0.
 *
 * Resampled export of a mixed row: mix, then filter. The filter of
 * zflac_hip_batch_export_resampled runs with v_c in place of x,
 *   y_c[m] = sum_{k < K} h[r][k] * v_c[q - W + k],
 * v_c zero outside the stream, the sum with fused multiply-adds in ascending k as there, so a
 * frame's value still does not depend on the window or tile it falls in. (Mixing and filtering
 * are both linear: a mono consumer pays for one filtered channel, not two.) A stream already at
 * the target rate is not filtered: its row has zflac_hip_batch_export_mixed's bits.
 *
 * Coefficients: every coefficient is 0, or finite with 2^-64 <= |m| <= 2^64. With |x| a multiple
 * of 2^-31 and at most 1, no product or partial sum is then subnormal or -0, so leaving out a zero
 * coefficient, or taking a coefficient of 1 as a copy, gives the same bits as the fmaf chain: a
 * kernel may do either. An output channel whose row of m is all zeros is +0 (0x00000000) in every
 * frame, as if it were never filtered. All non-NULL matrices are read and checked before the call
 * returns: the caller may free or overwrite them as soon as it returns, also when `stream` is the
 * caller's own.
 *
 * ZFLAC_E_INVALID_ARGUMENT (nothing written or enqueued): whatever the unmixed call rejects;
 * mix->size != sizeof(zflac_mix_desc); reserved != 0; a non-NULL matrix together with
 * ZFLAC_EXPORT_I32 (float dtypes only); a non-NULL matrix with channels > 8; a coefficient outside
 * the rule above in any non-NULL matrix, whether or not a stream of that channel count is in the
 * batch. zflac_hip_batch_export_ms reports the last synchronous export of any of the four kinds. */
int zflac_hip_batch_export_mixed(zflac_batch *b, const zflac_export_desc *d, const zflac_mix_desc *mix,
                                 void *dst_device, size_t dst_bytes, uint64_t *valid_frames, void *stream);
int zflac_hip_batch_export_resampled_mixed(zflac_batch *b, const zflac_resample_desc *d, const zflac_mix_desc *mix,
                                           void *dst_device, size_t dst_bytes, uint64_t *valid_frames, void *stream);

/* ---- log-mel features of a dense f32 waveform ---------------------------------------- */
/* From the planar f32 tensor the exports write (or any dense f32 rows in device memory) to
 * [row][bin][frame] features in one launch of one HIP kernel (k_mel): a windowed DFT as an f32
 * matrix product on the matrix cores, the power spectrum, a filterbank as a second f32 matrix
 * product, an optional log. A plan (zflac_mel) holds the tables; a run turns a waveform into
 * features.
 *
 * Row i of the waveform is x_i[s] = wave_device[i * row_stride + s] for 0 <= s < wave_frames and
 * zero outside that range (a [B, C, T] planar export is B * C rows of stride T). With N = n_fft,
 * K = N / 2 + 1 and off = center ? N / 2 : 0, feature frame t = first_frame + j (j < frames) is
 *   re[k] = sum_n c[n][k] * x_i[t * hop - off + n]     im[k] = sum_n s[n][k] * x_i[...]   k < K
 *   c[n][k] = (float)( window[n] * cos(2 pi ((n k) mod N) / N) )
 *   s[n][k] = (float)(-window[n] * sin(2 pi ((n k) mod N) / N) )
 *   P[k] = re[k]^2 + im[k]^2
 *   v[m] = sum_k filters[m][k] * P[k]                  m < n_bins
 * The tables are built in double from the caller's floats and rounded once; s[.][0] and
 * s[.][N / 2] are exactly 0. out[i][m][j] is v[m] (ZFLAC_MEL_POWER), log10f(max(v[m], floor)) or
 * logf(max(v[m], floor)), then rounded to f16 or bf16 exactly as the plain export rounds its f32
 * value. All sums are f32; the order of summation is the kernel's, the same for every frame: the
 * bits of a frame do not depend on rows, frames, first_frame, where the frame falls in a tile or
 * the alignment of wave_device. A frame with no non-zero sample under it has P = +0 everywhere,
 * so v = +0 and a log output of exactly log(floor). Every element of the destination is written.
 *
 * Padding is zeros only. There is no reflect mode: with center = 1 the first and the last
 * N / (2 hop) frames differ from those of a reflect-padded STFT (torch.stft's default). That
 * holds for zflac_hip_mel_run; zflac_hip_mel_run_ex below has ZFLAC_PAD_REFLECT. */
#define ZFLAC_MEL_POWER 0   /* the filterbank sums as they are */
#define ZFLAC_MEL_LOG10 1   /* log10f(max(v, floor)) */
#define ZFLAC_MEL_LN    2   /* logf(max(v, floor)) */
#define ZFLAC_MEL_BINS_FIRST   0  /* [row][bin][frame] */
#define ZFLAC_MEL_FRAMES_FIRST 1  /* [row][frame][bin] */
typedef struct zflac_mel_desc {
    uint32_t size;                        /* sizeof(zflac_mel_desc): 40 on LP64 */
    uint8_t dtype, layout, scale, center; /* ZFLAC_EXPORT_F32/_F16/_BF16; ZFLAC_MEL_*; center 0 or 1 */
    uint16_t n_fft;                       /* N: even, 2..2048 */
    uint16_t hop;                         /* 1..N */
    uint16_t n_bins;                      /* rows of `filters`: 1..256 */
    uint16_t reserved;                    /* must be 0 */
    float floor;                          /* log scales: finite and > 0; ZFLAC_MEL_POWER: must be 0 */
    const float *window;                  /* host, N floats */
    const float *filters;                 /* host, n_bins x (N/2 + 1) floats, row-major */
} zflac_mel_desc;
typedef struct zflac_mel zflac_mel;
/* A plan on `device`. The arguments are checked first and the device is touched afterwards (on a
 * machine without a GPU a good descriptor returns ZFLAC_E_DEVICE, a bad one
 * ZFLAC_E_INVALID_ARGUMENT); the host arrays are read before the call returns.
 * ZFLAC_E_INVALID_ARGUMENT: NULL d, out, window or filters; a wrong size; an unknown dtype
 * (ZFLAC_EXPORT_I32 included), layout or scale; center > 1; n_fft odd or outside 2..2048; hop of 0
 * or above n_fft; n_bins outside 1..256; reserved != 0; a floor outside its rule; a non-finite
 * window or filter value. */
int zflac_hip_mel_create(const zflac_mel_desc *d, int device, zflac_mel **out);
/* dst_device: rows * n_bins * frames elements of the plan's dtype, [row][bin][frame] or
 * [row][frame][bin]. Frames at or past zflac_hip_mel_frames() are still computed, from the
 * zero-extended row. stream == NULL: runs on the plan's own stream and returns when the tensor is
 * complete; otherwise the launch is enqueued on that hipStream_t of the plan's device without
 * synchronising. A run stages nothing (the tables are immutable, the arguments go by value), so
 * runs of one plan on different streams may overlap. rows == 0: ZFLAC_OK, nothing done.
 * ZFLAC_E_INVALID_ARGUMENT (nothing enqueued): NULL m, wave_device or dst_device; a wave_device
 * that is not 4-byte aligned; row_stride < wave_frames; frames == 0; dst_bytes < rows * n_bins *
 * frames * element size; (first_frame + frames) * hop not fitting 63 bits (nor rows * row_stride
 * 61); more than 2^31 - 1 workgroups (rows * ceil(frames / 128)). */
int zflac_hip_mel_run(zflac_mel *m, const float *wave_device, uint64_t rows, uint64_t wave_frames,
                      uint64_t row_stride, uint64_t first_frame, uint64_t frames,
                      void *dst_device, size_t dst_bytes, void *stream);
/* zflac_hip_mel_run with three more things a front end like Whisper's needs: a length per row,
 * reflect padding (torch.stft's default) and the clamp to the row maximum with an affine map
 * behind it. The plan, the tables and the sums are zflac_hip_mel_run's.
 *
 * Row length. n_i = min(lengths_device[i], wave_frames), or wave_frames for every row when
 * lengths_device is NULL. Nothing at or past x_i[n_i] is ever read as signal.
 *
 * ZFLAC_PAD_ZEROS: the definition above with n_i in place of wave_frames.
 * ZFLAC_PAD_REFLECT (a plan with center = 1 only): the frame sums read xr_i[s] in place of x_i[s],
 *   xr_i[s] = x_i[rho(s)]  for -N/2 <= s < n_i + N/2 and 0 <= rho(s) < n_i, and 0 otherwise,
 *   rho(s) = -s for s < 0,  2 (n_i - 1) - s for s >= n_i,  s otherwise.
 * One reflection, a total function: for n_i > N/2 it is numpy.pad(mode="reflect") and torch.stft's
 * padding by N/2; for n_i <= N/2 (0 and 1 included) it is still defined, so no length is checked
 * on the host. A row with n_i = 0 is all zeros. Frames at or past zflac_hip_mel_frames(n_i, ...)
 * are still computed, from xr_i.
 * The order of every sum is that of zflac_hip_mel_run and a frame's bits depend only on the N
 * values under it: a frame whose span lies inside [0, n_i) has the same bits in both pad modes,
 * and a reflect run of a row equals a zeros run of an uncentred plan with the same tables over
 * that row padded by reflection on the host.
 *
 * row_max_device != NULL: element i receives M_i, the maximum over the n_bins x frames elements
 * of row i that this call writes of the f32 value before it is rounded to the destination dtype
 * (v, or its log); the same bits for every dtype and layout. A maximum does not depend on the
 * order it is taken in, so M_i is deterministic. A NaN among the values is skipped (fmaxf).
 *
 * ZFLAC_NORM_ROW_MAX (needs row_max_device, a log scale, finite range >= 0, finite add, finite
 * mul != 0): with l the value ZFLAC_NORM_NONE would have stored (rounded to the destination
 * dtype, then widened to f32 again) the element stored is
 *   conv( (fmaxf(l, M_i - range) + add) * mul )
 * where the subtraction, the addition and the product are one f32 rounding each and nothing is
 * fused. For an f32 destination that is the single-rounding formula; for f16 / bf16 the value is
 * rounded to the dtype twice, once before the clamp and once after the product: a defined double
 * rounding, the one a caller who normalises a stored f16 / bf16 tensor gets. Whisper's input is
 * range = 8, add = 4, mul = 0.25 ((x + 4) / 4 in the same bits). M_i is taken over the window
 * [first_frame, first_frame + frames) this call asks for, so normalised outputs, unlike all
 * others, depend on the window. With ZFLAC_NORM_NONE range, add and mul must be 0.
 *
 * pad = ZFLAC_PAD_ZEROS, norm = ZFLAC_NORM_NONE, lengths_device = row_max_device = NULL is
 * zflac_hip_mel_run in every respect: the same kernel, the same bits, the same errors.
 *
 * Stream semantics are zflac_hip_mel_run's. The call enqueues up to three things on the one
 * stream (a fill of row_max_device with -inf, k_mel, the normalising pass k_mel_norm) and stages
 * nothing from the host; row_max_device belongs to the caller, so runs of one plan on different
 * streams with different row_max_device may overlap. rows == 0: ZFLAC_OK, nothing done.
 * ZFLAC_E_INVALID_ARGUMENT (nothing enqueued): NULL m or r; a wrong size; an unknown pad or norm;
 * reserved or reserved2 != 0; everything zflac_hip_mel_run refuses; lengths_device not 8-byte or
 * row_max_device not 4-byte aligned; ZFLAC_PAD_REFLECT with an uncentred plan; ZFLAC_NORM_ROW_MAX
 * outside its rule above; non-zero range, add or mul with ZFLAC_NORM_NONE. */
#define ZFLAC_PAD_ZEROS   0
#define ZFLAC_PAD_REFLECT 1
#define ZFLAC_NORM_NONE    0
#define ZFLAC_NORM_ROW_MAX 1
typedef struct zflac_mel_run_desc {
    uint32_t size;                  /* sizeof(zflac_mel_run_desc): 104 on LP64 */
    uint8_t pad, norm;              /* ZFLAC_PAD_*, ZFLAC_NORM_* */
    uint16_t reserved;              /* must be 0 */
    const float *wave_device;
    uint64_t rows, wave_frames, row_stride;  /* as zflac_hip_mel_run */
    const uint64_t *lengths_device; /* device, one per row, or NULL: wave_frames for every row */
    uint64_t first_frame, frames;
    void *dst_device;
    size_t dst_bytes;
    float *row_max_device;          /* device, `rows` floats, written; or NULL */
    float range, add, mul;          /* ZFLAC_NORM_ROW_MAX; else 0 */
    uint32_t reserved2;             /* must be 0 */
} zflac_mel_run_desc;
int zflac_hip_mel_run_ex(zflac_mel *m, const zflac_mel_run_desc *r, void *stream);
/* Frames of a centred (n ? n / hop + 1 : 0) or uncentred (n >= n_fft ? (n - n_fft) / hop + 1 : 0)
 * STFT of n_samples: what callers use as the valid length. 0 when hop is 0. Host arithmetic. */
uint64_t zflac_hip_mel_frames(uint64_t n_samples, uint32_t n_fft, uint32_t hop, int center);
/* Waits for the device, then frees the plan. NULL is ignored. */
void zflac_hip_mel_destroy(zflac_mel *m);

/* The arithmetic of a plan's first product (the DFT), chosen when the plan is made.
 *
 * ZFLAC_MEL_MATH_F32 is zflac_hip_mel_create's plan in every respect: the same tables, kernels,
 * bits and errors. The f32 matrix instruction runs at 1/16 of the bf16 matrix rate on gfx950; the
 * two split modes buy that rate back by cutting both operands into bfloat16 pieces and keeping
 * only the products that matter (kernel k_mel_split).
 *
 * b(v) is v rounded to the nearest bfloat16, ties to even, as ZFLAC_EXPORT_BF16 rounds. An f32 v
 * has the pieces v0 = b(v), v1 = b(v - v0), v2 = b(v - v0 - v1); the subtractions are exact in
 * f32 and v0 + v1 + v2 = v exactly. c_i[n][k] and s_i[n][k] are the pieces of the f32 tables c and
 * s of zflac_hip_mel_run's definition, built on the host; x_j are the pieces of the f32 sample (or
 * the reflected or zero value) a frame reads, taken on the device. Then
 *   re[k] = sum_n sum_{(i,j) in T} c_i[n][k] * x_j[t * hop - off + n]      im[k] likewise with s_i
 *   T = { i + j <= 2 }  six terms,   ZFLAC_MEL_MATH_BF16X6
 *   T = { i + j <= 1 }  three terms, ZFLAC_MEL_MATH_BF16X3
 * Every product is exact in f32 (8 x 8 significant bits); the sums are f32 accumulations inside
 * the matrix cores, in the kernel's order, which is the same for every frame. Everything behind
 * re and im is the f32 plan's: P = fmaf(im, im, re * re), the filterbank as an f32 fmaf chain over
 * the f32 filter table, the floor, the log and the rounding to the dtype.
 *
 * What the dropped products cost: a sum differs from the full product c * x by at most
 * 3 * 2^-24 * sum_n |c| |x| (BF16X6) or 2^-14 * sum_n |c| |x| (BF16X3), which is about 130 dB and
 * 84 dB below sum_n |c| |x| in the worst case. BF16X6 is below the rounding an f32 sum of N terms
 * has anyway and is f32-grade. The error is relative to the whole frame, not to the bin: under
 * BF16X3 a bin more than about 80 dB below the loudest content of its frame carries no correct
 * digit (a log-mel front end that clamps 80 dB below the maximum loses nothing it keeps; an
 * analysis of a quiet partial beside a loud one wants BF16X6 or F32).
 *
 * Domain: finite samples with |x| <= 2^64; a piece below 2^-126 may be flushed to zero. Frames
 * over a non-finite sample are unspecified; no other frame is affected. The guarantees of the f32
 * plan hold for a split plan against itself: a frame's bits depend on the N values under it alone
 * (not on rows, frames, first_frame, the position in a tile or the alignment of wave_device); a
 * frame with no non-zero value under it gives exactly log(floor), or +0 on the POWER scale; a
 * frame inside [0, n_i) has the same bits in both pad modes; a reflect run equals a zeros run of
 * an uncentred plan of the same math over the host-reflected row, bit for bit.
 *
 * zflac_hip_mel_run, zflac_hip_mel_run_ex, zflac_hip_mel_frames and zflac_hip_mel_destroy take
 * such a plan unchanged, with every rule they state (ZFLAC_NORM_ROW_MAX runs k_mel_norm as it is).
 * An unknown math is ZFLAC_E_INVALID_ARGUMENT, checked after everything zflac_hip_mel_create
 * checks and before the device is touched. */
#define ZFLAC_MEL_MATH_F32    UINT32_C(0)  /* zflac_hip_mel_create's plan: the same tables, kernels, bits */
#define ZFLAC_MEL_MATH_BF16X6 UINT32_C(1)  /* split operands, product terms of level i + j <= 2 */
#define ZFLAC_MEL_MATH_BF16X3 UINT32_C(2)  /* split operands, product terms of level i + j <= 1 */
int zflac_hip_mel_create_ex(const zflac_mel_desc *d, uint32_t math, int device, zflac_mel **out);
/* The plan's ZFLAC_MEL_MATH_*; -ZFLAC_E_INVALID_ARGUMENT for NULL. */
int zflac_hip_mel_math(const zflac_mel *m);

/* Framed plans: a frame shorter than the DFT, Kaldi's framings, and the per-frame operations of
 * a Kaldi filterbank front end folded into the tables. N = d->n_fft is the DFT size, K = N / 2 + 1,
 * Nw = f->win_length the frame length, and d->window holds Nw floats.
 *
 * Frame start. Frame t reads x_i[s0(t) + n], n < Nw:
 *   ZFLAC_FRAMING_STFT          s0(t) = t hop - (center ? N / 2 : 0) + (N - Nw) / 2: torch.stft with
 *                               the window centred in the DFT; frames: zflac_hip_mel_frames's.
 *   ZFLAC_FRAMING_SNIP          s0(t) = t hop; frames: n >= Nw ? (n - Nw) / hop + 1 : 0 (Kaldi,
 *                               snip_edges = true). center must be 0.
 *   ZFLAC_FRAMING_KALDI_CENTER  s0(t) = t hop + hop / 2 - Nw / 2 (integer divisions); frames:
 *                               (n + hop / 2) / hop (Kaldi, snip_edges = false). center must be 0.
 * hop <= Nw for every framed plan. s0(0) may be positive (_STFT, center = 0, Nw < N).
 *
 * Frame operator, in Kaldi's order, on f[n] = g x_i[s0 + n] (g = sample_scale):
 *   1. remove_dc:    f[n] -= mean(f)
 *   2. preemphasis:  y[0] = (1 - a) f[0],  y[n] = f[n] - a f[n - 1]
 *   3. window:       z[n] = window[n] y[n]
 *   4. z zero-extended to N, its DFT, the power P[k] = |Z[k]|^2, then as zflac_hip_mel_run.
 * z = A x is linear in the frame, so the library folds A into the tables and the kernels run the
 * sums of zflac_hip_mel_run unchanged over Nw terms:
 *   re[k] = sum_{n < Nw} c'[n][k] x_i[s0 + n]
 *   c'[n][k] = (float)( sum_m window[m] cos(2 pi ((m k) mod N) / N) A[m][n] ),  s' with -sin,
 * built in double and rounded once (the sine entries of k = 0 and k = N / 2 are exactly 0 before
 * the folding, as ever). The window sits at n = 0..Nw-1 of the DFT, not centred in it: the power
 * spectrum does not see that shift, so a framed plan agrees with the plan of the same window
 * zero-padded to N within the error bound of the sums, not bit for bit.
 * The table is padded with zero rows to an even Nw (F32) or a multiple of 16 (split plans); a
 * padded position may read a real sample against a zero coefficient, which adds nothing for a
 * finite sample (non-finite samples: the split plans' "unspecified" clause holds for both).
 *
 * A framed plan with Nw = N, ZFLAC_FRAMING_STFT, remove_dc = 0, preemphasis = 0 and
 * sample_scale = 1 is zflac_hip_mel_create_ex's plan: the same tables byte for byte, the same
 * kernels, the same bits. zflac_hip_mel_run, _run_ex, _math and _destroy take a framed plan.
 * ZFLAC_PAD_REFLECT needs ZFLAC_FRAMING_STFT with center = 1 and pads by N / 2, half the DFT
 * size, as torch.stft does. ZFLAC_PAD_MIRROR (zflac_mel_run_desc.pad; ZFLAC_FRAMING_KALDI_CENTER
 * only) reads xm_i[s] in place of x_i[s]:
 *   xm_i[s] = x_i[rho(s)] if 0 <= rho(s) < n_i, else 0
 *   rho(s) = -1 - s for s < 0,  2 n_i - 1 - s for s >= n_i,  s otherwise
 * (the edge sample is repeated). One mirror, a total function: Kaldi's ExtractWindow wherever one
 * reflection suffices, zeros where Kaldi would reflect again. ZFLAC_PAD_ZEROS works with every
 * framing. A frame inside [0, n_i) has the same bits in every pad mode.
 *
 * Checked, in this order, before the device is touched (ZFLAC_E_INVALID_ARGUMENT): everything
 * zflac_hip_mel_create checks up to and including floor, then f (NULL), f->size, win_length
 * (1..n_fft), framing, remove_dc (0 or 1), preemphasis (finite, 0 <= a <= 1), sample_scale
 * (finite, 2^-64 <= |g| <= 2^64), reserved; window and filters (NULL, then every value finite,
 * window read as Nw floats); framing against center; hop <= Nw; math.
 *
 * Not provided: dither (0 only), use_energy / raw_energy, VTLN warping, and pre-emphasis over the
 * whole waveform (NeMo's); the pre-emphasis here is Kaldi's, per frame. */
#define ZFLAC_FRAMING_STFT         0
#define ZFLAC_FRAMING_SNIP         1
#define ZFLAC_FRAMING_KALDI_CENTER 2
#define ZFLAC_PAD_MIRROR 2
typedef struct zflac_mel_frame_desc {
    uint32_t size;          /* sizeof(zflac_mel_frame_desc): 20 */
    uint16_t win_length;    /* Nw: 1..n_fft; desc->window then has Nw floats */
    uint8_t  framing;       /* ZFLAC_FRAMING_* */
    uint8_t  remove_dc;     /* 0 or 1 */
    float    preemphasis;   /* a: finite, 0 <= a <= 1 */
    float    sample_scale;  /* g: finite, 2^-64 <= |g| <= 2^64 (1 = none, 32768 = Kaldi's 16-bit scale) */
    uint32_t reserved;      /* must be 0 */
} zflac_mel_frame_desc;
int zflac_hip_mel_create_framed(const zflac_mel_desc *d, const zflac_mel_frame_desc *f,
                                uint32_t math, int device, zflac_mel **out);
/* Frames of a row of n_samples under the plan's framing (the table above). 0 for NULL. Host
 * arithmetic. */
uint64_t zflac_hip_mel_plan_frames(const zflac_mel *m, uint64_t n_samples);

/* Mean / variance normalisation of each (row, bin) over the row's valid frames, in place, behind
 * zflac_hip_mel_run / _run_ex (utterance CMVN; kernel k_mel_cmvn). feat_device is rows x n_bins x
 * frames elements of the plan's dtype in the plan's layout. F_i = min(valid_device[i], frames), or
 * frames for every row when valid_device is NULL. With l[j] the stored element of (row i, bin b)
 * at frame j widened to f32:
 *   mu = sum_{j < F_i} l[j] / F_i
 *   var = sum_{j < F_i} (l[j] - mu)^2 / max(F_i - ddof, 0),  sigma = sqrt(var), 0 when the divisor is 0
 * Both sums are f64, in an order that is a function of F_i alone (and of the plan): no floating
 * atomics, so a run repeats bit for bit and a row's bits do not depend on the row count or on the
 * row's position. mu32 = (float)mu; r = (float)(1 / (sigma + eps)), 0 when sigma + eps = 0, and 1
 * for ZFLAC_CMVN_MEAN. Stored at j < F_i: conv((l[j] - mu32) * r), two f32 roundings, nothing
 * fused; at j >= F_i: conv(pad_value). mean_device / std_device (rows x n_bins f32, optional)
 * receive mu32 and (float)sigma (std: 0 for ZFLAC_CMVN_MEAN); both are 0 where F_i = 0. The
 * statistics depend on the frame window the caller hands over, as the row maximum does.
 * Stream semantics are zflac_hip_mel_run_ex's; nothing is staged from the host. rows == 0:
 * ZFLAC_OK, nothing done.
 * ZFLAC_E_INVALID_ARGUMENT (nothing enqueued), in this order: NULL m or c; size; mode; ddof > 1;
 * reserved; NULL feat_device; frames == 0; rows * n_bins * frames * element size not fitting 63
 * bits; valid_device not 8-byte, mean_device or std_device not 4-byte aligned; eps not finite or
 * negative; pad_value not finite. */
#define ZFLAC_CMVN_MEAN 0
#define ZFLAC_CMVN_MEAN_VAR 1
typedef struct zflac_mel_cmvn_desc {
    uint32_t size;                  /* sizeof(zflac_mel_cmvn_desc): 64 on LP64 */
    uint8_t mode, ddof;             /* ZFLAC_CMVN_*; 0 or 1 */
    uint16_t reserved;              /* must be 0 */
    void *feat_device;              /* rows x n_bins x frames of the plan's dtype and layout, in place */
    uint64_t rows, frames;
    const uint64_t *valid_device;   /* per row, valid frames; or NULL: frames */
    float *mean_device, *std_device;/* optional outputs, rows x n_bins f32; may be NULL */
    float eps;                      /* finite, >= 0 */
    float pad_value;                /* finite; stored in frames >= F_i */
} zflac_mel_cmvn_desc;
int zflac_hip_mel_cmvn(zflac_mel *m, const zflac_mel_cmvn_desc *c, void *stream);

/* Cepstra and dynamic features behind the log-mel features: a projection of every frame's bins by
 * a matrix (MFCC: a DCT with the lifter folded in; kernel k_mel_dct), the normalisation of
 * zflac_hip_mel_cmvn over the projected features, and Kaldi's add-deltas (kernel k_mel_delta). A
 * cepstra plan holds what the kernels read on the device: the matrix T (n_out x n_in f32,
 * row-major) and the delta scales. The tensors are those of the mel plans: rows x C x frames
 * (ZFLAC_MEL_BINS_FIRST) or rows x frames x C (ZFLAC_MEL_FRAMES_FIRST) elements, contiguous.
 *
 * matrix == NULL: no projection, the plan computes deltas only; n_out must equal n_in and in_dtype
 * out_dtype. delta_order == 0: the plan only projects. A plan with neither is refused.
 *
 * Delta scales (Kaldi's DeltaFeatures): s_0 = [1], s_o = s_{o-1} convolved with
 * [j / sum_{|i| <= W} i^2, j = -W..W], W = delta_window; s_o has 2 o W + 1 taps, j = -oW..oW. They
 * are built in double and rounded to f32 once. Order 1, W = 2: [-2, -1, 0, 1, 2] / 10. Order 2,
 * W = 2: [4, 4, 1, -4, -10, -4, 1, 4, 4] / 100. zflac_hip_cepstra_delta_scales copies the taps of
 * one order (0..delta_order) to out and returns their count, or -ZFLAC_E_INVALID_ARGUMENT for a
 * NULL plan or out, an order above the plan's, or cap below the count.
 *
 * zflac_hip_cepstra_create checks, in this order, before the device is touched
 * (ZFLAC_E_INVALID_ARGUMENT): NULL d or out; size; in_dtype, out_dtype (ZFLAC_EXPORT_F32 / _F16 /
 * _BF16); layout; delta_order > 3; n_in, then n_out (1..256 each); delta_window (1..5 when
 * delta_order > 0, else 0); reserved; with matrix == NULL: n_out != n_in, in_dtype != out_dtype,
 * delta_order == 0; with a matrix: every value finite. Then the device (ZFLAC_E_DEVICE).
 *
 * The three run calls take the caller's stream with the semantics of zflac_hip_mel_cmvn: nothing is
 * staged from the host, rows == 0 is ZFLAC_OK with nothing done, and a refused call enqueues
 * nothing. No kernel uses atomics: a run repeats bit for bit, and a frame's bits do not depend on
 * the row count, on the row's position, on where the frame sits in the call's window (but see the
 * deltas' edges) or on the alignment of the tensors.
 *
 * zflac_hip_cepstra_project: src_device is rows x n_in x frames of in_dtype, dst_device rows x
 * n_out x frames of out_dtype, both in the plan's layout. With l[m] the stored bin m of a frame,
 *   out[k] = conv_out( sum_{m < n_in} T[k][m] * widen(l[m]) )
 * in f32: acc = 0, then acc = fma(T[k][m], l[m], acc) for m = 0, 1, .. n_in - 1, the same in both
 * layouts. Every frame handed over is computed; the call takes no lengths. A non-finite value
 * stays in its frame.
 * Refused (ZFLAC_E_INVALID_ARGUMENT), in this order: NULL p or r; size; reserved; a plan without a
 * matrix; NULL src_device, then dst_device; src_device == dst_device; src_device not aligned to
 * in_dtype's size, dst_device to out_dtype's; frames == 0; rows * n_in * frames * in_dtype's size,
 * then rows * n_out * frames * out_dtype's size, not fitting 63 bits.
 *
 * zflac_hip_cepstra_cmvn is zflac_hip_mel_cmvn with n_out for the bin count and the plan's
 * out_dtype and layout: the same descriptor, the same kernel launch, the same bits and the same
 * refusals in the same order. Kaldi normalises cepstra before it appends deltas.
 *
 * zflac_hip_cepstra_deltas: src_device is rows x C x frames, dst_device rows x (delta_order + 1) C
 * x frames, C = n_out, both of out_dtype in the plan's layout. Feature block o (features o C ..
 * o C + C - 1) is the o-th derivative, block 0 the input; frames first, a frame's (delta_order + 1) C
 * values are contiguous in Kaldi's order: base, delta, delta-delta. F_i = min(valid_device[i],
 * frames), or frames when valid_device is NULL. For t < F_i
 *   out_o[c][t] = conv( sum_{j = -oW..oW} s_o[j] * widen(x[c][clamp(t + j, 0, F_i - 1)]) )
 * in f32: acc = 0, then acc = fma(s_o[j], x, acc) for j = -oW, .. oW, an order fixed by (o, W)
 * alone. Block 0 is the exact copy. For t >= F_i every block holds conv(pad_value); nothing at or
 * past F_i is read. This is Kaldi's ComputeDeltas: one pass over the base features with the index
 * clamped, not the delta operator applied o times. It differs from
 * torchaudio.functional.compute_deltas applied twice only within 2 W frames of a row's ends. As
 * with CMVN, the edge frames depend on the frame window the caller hands over: the clamp is at the
 * first frame of the call and at F_i.
 * Refused (ZFLAC_E_INVALID_ARGUMENT), in this order: NULL p or r; size; reserved, then reserved2; a
 * plan with delta_order == 0; NULL src_device, then dst_device; src_device == dst_device; either not aligned
 * to out_dtype's size; frames == 0; rows * (delta_order + 1) * n_out * frames * out_dtype's size
 * not fitting 63 bits; valid_device not 8-byte aligned; pad_value not finite.
 *
 * Not provided: Kaldi's use_energy / raw_energy (C0 is the DCT's row 0), dither, frame splicing
 * and low-frame-rate stacking. */
typedef struct zflac_cepstra zflac_cepstra;
typedef struct zflac_cepstra_desc {
    uint32_t size;                 /* sizeof(zflac_cepstra_desc): 24 on LP64 */
    uint8_t  in_dtype, out_dtype, layout, delta_order;  /* ZFLAC_EXPORT_F32/_F16/_BF16 twice; ZFLAC_MEL_BINS_FIRST/_FRAMES_FIRST; 0..3 */
    uint16_t n_in, n_out;          /* 1..256 each; matrix == NULL: n_out must equal n_in */
    uint8_t  delta_window;         /* 1..5 when delta_order > 0, else 0 */
    uint8_t  reserved[3];          /* 0 */
    const float *matrix;           /* host, n_out x n_in row-major, every value finite; or NULL: no projection */
} zflac_cepstra_desc;
int zflac_hip_cepstra_create(const zflac_cepstra_desc *d, int device, zflac_cepstra **out);
void zflac_hip_cepstra_destroy(zflac_cepstra *p);
/* n_out * (delta_order + 1); 0 for NULL */
uint32_t zflac_hip_cepstra_features(const zflac_cepstra *p);
int zflac_hip_cepstra_delta_scales(const zflac_cepstra *p, uint32_t order, float *out, uint32_t cap);

typedef struct zflac_cepstra_project_desc {
    uint32_t size;             /* sizeof(zflac_cepstra_project_desc): 40 on LP64 */
    uint32_t reserved;         /* must be 0 */
    const void *src_device;    /* rows x n_in x frames of in_dtype, the plan's layout */
    void *dst_device;          /* rows x n_out x frames of out_dtype, the plan's layout */
    uint64_t rows, frames;
} zflac_cepstra_project_desc;
int zflac_hip_cepstra_project(zflac_cepstra *p, const zflac_cepstra_project_desc *r, void *stream);

int zflac_hip_cepstra_cmvn(zflac_cepstra *p, const zflac_mel_cmvn_desc *c, void *stream);

typedef struct zflac_cepstra_delta_desc {
    uint32_t size;                 /* sizeof(zflac_cepstra_delta_desc): 56 on LP64 */
    uint32_t reserved;             /* must be 0 */
    const void *src_device;        /* rows x n_out x frames of out_dtype, the plan's layout */
    void *dst_device;              /* rows x (delta_order + 1) n_out x frames of out_dtype */
    uint64_t rows, frames;
    const uint64_t *valid_device;  /* per row, valid frames; or NULL: frames */
    float pad_value;               /* finite; stored in every block at frames >= F_i */
    uint32_t reserved2;            /* must be 0 */
} zflac_cepstra_delta_desc;
int zflac_hip_cepstra_deltas(zflac_cepstra *p, const zflac_cepstra_delta_desc *r, void *stream);

/* Flags for zflac_hip_batch_create */
#define ZFLAC_FLAG_TIMING 1        /* record HIP events around each kernel */
#define ZFLAC_FLAG_FORCE_SLOW 2    /* skip the parallel fast path (testing the sequential path) */
/* Verify every stream's STREAMINFO MD5 on the device after each run (one lane per
 * stream: pays off for batches of many streams; a single long stream hashes faster on
 * the host, which zflac_hip_read / zflac_hip_batch_read do without this flag). A
 * mismatch makes the stream's result ZFLAC_E_INVALID_CHECKSUM (src/zflac.zig:279-280).
 * The hash of the streams a run certifies is enqueued by zflac_hip_batch_submit right
 * behind that run's kernels (so it overlaps other batches' runs in flight); streams the
 * sequential planner finishes are hashed by zflac_hip_batch_wait. */
#define ZFLAC_FLAG_DEVICE_MD5 4
/* Check every decoded frame's CRC-16 trailer on the device (k_crc16). zflac reads the
 * trailer and ignores it (src/zflac.zig:548-551), so this is off by default; with it, the
 * first frame in stream order whose trailer differs makes the stream ZFLAC_E_FRAME_CRC
 * (ahead of a later frame's error and of the MD5 check, which come after it in zflac's
 * read order). */
#define ZFLAC_FLAG_CHECK_CRC16 8
/* Subframe-start walk of 2+ channel streams: by default the library picks k_walk (a lane per
 * frame) for launches of many frames and k_walk_wave (a wave per frame, wave-wide bit scan)
 * otherwise. These force one (testing, timing); results are identical. */
#define ZFLAC_FLAG_WALK_LANE 16
#define ZFLAC_FLAG_WALK_WAVE 32
/* The frame-table front (zflac_hip_batch_front). By default (and with both flags) each class
 * takes k_hop when every stream has a STREAMINFO total and fixed blocking (first frame 0xF8,
 * STREAMINFO min block == max block), no stream has more than 64 frames and the class has at
 * least 768 streams; k_scan otherwise. _FRONT_SCAN forces k_scan; _FRONT_HOP forces k_hop for
 * every class whose streams allow it (totals, fixed blocking, frames per stream), whatever the
 * stream count. The environment variable ZFLAC_FRONT=scan|hop|auto does the same for batches
 * created without either flag. ZFLAC_HOP_MAX_FRAMES and ZFLAC_HOP_MIN_STREAMS, read when a batch
 * is created, replace the two limits: overrides for tests and for the sweeps the limits were
 * measured with (tools/sweep_front.py), not tuning knobs. k_hop also requires every frame but a
 * stream's last to code the STREAMINFO block size; a stream that does not sends its class back to
 * k_scan like any stream the hop cannot follow. Results are identical. */
#define ZFLAC_FLAG_FRONT_SCAN 64
#define ZFLAC_FLAG_FRONT_HOP 128

const char *zflac_hip_error_name(int code);
/* Number of HIP devices visible; 0 means every decode will fail with ZFLAC_E_DEVICE. */
int zflac_hip_device_count(void);
/* Library build tag, e.g. "zflac_hip gfx950 r3". */
const char *zflac_hip_version(void);
/* Identity of the compiled library: "src=<sha256 of its sources, headers, target, flags and
 * -D defines>" (zflac_amd/build.py source_fingerprint). hipcc output is not bit-reproducible,
 * so this, not a hash of the .so, says which kernels a measurement ran. */
const char *zflac_hip_build_id(void);
/* ABI revision of this header; bumped whenever a struct or a signature changes.
 * 3: zflac_hip_batch_timings_ex, zflac_hip_abi_version; device MD5 pipelined into submit.
 * 4: zflac_timings.rest_launches; zflac_hip_build_id; zflac_hip_batch_ready.
 * 5: zflac_timings.sequential_streams (was reserved0); total-unknown streams certified by the
 *    parallel pass.
 *    Added without a bump (no existing struct or signature changed): zflac_export_desc,
 *    zflac_hip_batch_export, zflac_hip_batch_export_ms, ZFLAC_EXPORT_*, ZFLAC_LAYOUT_*;
 *    zflac_resample_desc, zflac_hip_batch_export_resampled, zflac_hip_resampled_frames,
 *    zflac_hip_batch_resample_tables; zflac_hip_batch_decode_buckets, ZFLAC_BUCKET_*;
 *    zflac_hip_batch_front, ZFLAC_FRONT_*, ZFLAC_FLAG_FRONT_*; zflac_mix_desc,
 *    ZFLAC_MIX_MAX_CHANNELS, zflac_hip_batch_export_mixed, zflac_hip_batch_export_resampled_mixed;
 *    zflac_mel_desc, zflac_mel, ZFLAC_MEL_*, zflac_hip_mel_create, zflac_hip_mel_run,
 *    zflac_hip_mel_frames, zflac_hip_mel_destroy; zflac_mel_run_desc, zflac_hip_mel_run_ex,
 *    ZFLAC_PAD_*, ZFLAC_NORM_*; zflac_hip_batch_md5_source, ZFLAC_MD5_SRC_*,
 *    zflac_hip_batch_md5_stats, ZFLAC_MD5_K_*; ZFLAC_MEL_MATH_*, zflac_hip_mel_create_ex,
 *    zflac_hip_mel_math; zflac_mel_frame_desc, ZFLAC_FRAMING_*, ZFLAC_PAD_MIRROR,
 *    zflac_hip_mel_create_framed, zflac_hip_mel_plan_frames; zflac_mel_cmvn_desc, ZFLAC_CMVN_*,
 *    zflac_hip_mel_cmvn; zflac_cepstra, zflac_cepstra_desc, zflac_hip_cepstra_create,
 *    zflac_hip_cepstra_destroy, zflac_hip_cepstra_features, zflac_hip_cepstra_delta_scales,
 *    zflac_cepstra_project_desc, zflac_hip_cepstra_project, zflac_hip_cepstra_cmvn,
 *    zflac_cepstra_delta_desc, zflac_hip_cepstra_deltas. */
#define ZFLAC_HIP_ABI_VERSION 5
int zflac_hip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
