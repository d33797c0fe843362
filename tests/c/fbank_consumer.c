/* fbank_consumer.c -- a strict C11 consumer of the framed-plan and CMVN part of
 * include/zflac_hip.h (tests/test_fbank_abi.py builds it with -std=c11 -Wall -Wextra -Werror
 * -pedantic against the header alone and links it to the in-tree library): the struct layouts a
 * foreign binding relies on as static asserts, the constants, and the calls' answers that need no
 * GPU (a bad descriptor before the device, a good one ZFLAC_E_DEVICE on device -1). */
#include <assert.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "zflac_hip.h"

static_assert(sizeof(zflac_mel_frame_desc) == 20, "zflac_mel_frame_desc");
static_assert(offsetof(zflac_mel_frame_desc, size) == 0, "size");
static_assert(offsetof(zflac_mel_frame_desc, win_length) == 4, "win_length");
static_assert(offsetof(zflac_mel_frame_desc, framing) == 6, "framing");
static_assert(offsetof(zflac_mel_frame_desc, remove_dc) == 7, "remove_dc");
static_assert(offsetof(zflac_mel_frame_desc, preemphasis) == 8, "preemphasis");
static_assert(offsetof(zflac_mel_frame_desc, sample_scale) == 12, "sample_scale");
static_assert(offsetof(zflac_mel_frame_desc, reserved) == 16, "reserved");

static_assert(sizeof(zflac_mel_cmvn_desc) == 64, "zflac_mel_cmvn_desc");
static_assert(offsetof(zflac_mel_cmvn_desc, mode) == 4, "mode");
static_assert(offsetof(zflac_mel_cmvn_desc, ddof) == 5, "ddof");
static_assert(offsetof(zflac_mel_cmvn_desc, reserved) == 6, "reserved");
static_assert(offsetof(zflac_mel_cmvn_desc, feat_device) == 8, "feat_device");
static_assert(offsetof(zflac_mel_cmvn_desc, rows) == 16, "rows");
static_assert(offsetof(zflac_mel_cmvn_desc, frames) == 24, "frames");
static_assert(offsetof(zflac_mel_cmvn_desc, valid_device) == 32, "valid_device");
static_assert(offsetof(zflac_mel_cmvn_desc, mean_device) == 40, "mean_device");
static_assert(offsetof(zflac_mel_cmvn_desc, std_device) == 48, "std_device");
static_assert(offsetof(zflac_mel_cmvn_desc, eps) == 56, "eps");
static_assert(offsetof(zflac_mel_cmvn_desc, pad_value) == 60, "pad_value");
static_assert(sizeof(zflac_mel_desc) == 40 && sizeof(zflac_mel_run_desc) == 104, "the older descriptors did not grow");

static_assert(ZFLAC_FRAMING_STFT == 0 && ZFLAC_FRAMING_SNIP == 1 && ZFLAC_FRAMING_KALDI_CENTER == 2, "framings");
static_assert(ZFLAC_PAD_ZEROS == 0 && ZFLAC_PAD_REFLECT == 1 && ZFLAC_PAD_MIRROR == 2, "pads");
static_assert(ZFLAC_CMVN_MEAN == 0 && ZFLAC_CMVN_MEAN_VAR == 1, "cmvn modes");
static_assert(ZFLAC_HIP_ABI_VERSION == 5, "no bump");

#define NW 400
#define NFFT 512
#define BINS 80

static float window[NW];
static float filters[BINS * (NFFT / 2 + 1)];

int main(void) {
    zflac_mel_desc d;
    zflac_mel_frame_desc f;
    zflac_mel_cmvn_desc c;
    zflac_mel *m = NULL;
    int good, bad_frame, bad_order, cmvn_null;
    size_t i;
    for (i = 0; i < NW; i++) window[i] = 1.0f;
    for (i = 0; i < sizeof filters / sizeof filters[0]; i++) filters[i] = 0.5f;
    memset(&d, 0, sizeof d);
    d.size = (uint32_t)sizeof d;
    d.dtype = ZFLAC_EXPORT_F32;
    d.layout = ZFLAC_MEL_FRAMES_FIRST;
    d.scale = ZFLAC_MEL_LN;
    d.n_fft = NFFT;
    d.hop = 160;
    d.n_bins = BINS;
    d.floor = 1.1920929e-07f;
    d.window = window;
    d.filters = filters;
    memset(&f, 0, sizeof f);
    f.size = (uint32_t)sizeof f;
    f.win_length = NW;
    f.framing = ZFLAC_FRAMING_SNIP;
    f.remove_dc = 1;
    f.preemphasis = 0.97f;
    f.sample_scale = 32768.0f;
    good = zflac_hip_mel_create_framed(&d, &f, ZFLAC_MEL_MATH_F32, -1, &m); /* no such device: the arguments passed */
    f.win_length = NFFT + 1;
    bad_frame = zflac_hip_mel_create_framed(&d, &f, ZFLAC_MEL_MATH_F32, -1, &m);
    f.win_length = NW;
    d.center = 1; /* a Kaldi framing with a centred plan */
    bad_order = zflac_hip_mel_create_framed(&d, &f, ZFLAC_MEL_MATH_BF16X3, -1, &m);
    memset(&c, 0, sizeof c);
    c.size = (uint32_t)sizeof c;
    cmvn_null = zflac_hip_mel_cmvn(NULL, &c, NULL);
    printf("{\"good\": %d, \"bad_frame\": %d, \"bad_order\": %d, \"cmvn_null\": %d, \"frames_null\": %llu, \"abi\": %d}\n", good,
           bad_frame, bad_order, cmvn_null, (unsigned long long)zflac_hip_mel_plan_frames(NULL, 16000), zflac_hip_abi_version());
    return 0;
}
