/* cepstra_consumer.c -- a strict C11 consumer of the cepstra part of include/zflac_hip.h
 * (tests/test_cepstra_abi.py builds it with -std=c11 -Wall -Wextra -Werror -pedantic against the
 * header alone and links it to the in-tree library): the struct layouts a foreign binding relies
 * on as static asserts, and the calls' answers that need no GPU (a bad descriptor before the
 * device, a good one ZFLAC_E_DEVICE on device -1, every run call refused on no plan). */
#include <assert.h>
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "zflac_hip.h"

static_assert(sizeof(zflac_cepstra_desc) == 24, "zflac_cepstra_desc");
static_assert(offsetof(zflac_cepstra_desc, size) == 0, "size");
static_assert(offsetof(zflac_cepstra_desc, in_dtype) == 4, "in_dtype");
static_assert(offsetof(zflac_cepstra_desc, out_dtype) == 5, "out_dtype");
static_assert(offsetof(zflac_cepstra_desc, layout) == 6, "layout");
static_assert(offsetof(zflac_cepstra_desc, delta_order) == 7, "delta_order");
static_assert(offsetof(zflac_cepstra_desc, n_in) == 8, "n_in");
static_assert(offsetof(zflac_cepstra_desc, n_out) == 10, "n_out");
static_assert(offsetof(zflac_cepstra_desc, delta_window) == 12, "delta_window");
static_assert(offsetof(zflac_cepstra_desc, reserved) == 13, "reserved");
static_assert(offsetof(zflac_cepstra_desc, matrix) == 16, "matrix");

static_assert(sizeof(zflac_cepstra_project_desc) == 40, "zflac_cepstra_project_desc");
static_assert(offsetof(zflac_cepstra_project_desc, reserved) == 4, "reserved");
static_assert(offsetof(zflac_cepstra_project_desc, src_device) == 8, "src_device");
static_assert(offsetof(zflac_cepstra_project_desc, dst_device) == 16, "dst_device");
static_assert(offsetof(zflac_cepstra_project_desc, rows) == 24, "rows");
static_assert(offsetof(zflac_cepstra_project_desc, frames) == 32, "frames");

static_assert(sizeof(zflac_cepstra_delta_desc) == 56, "zflac_cepstra_delta_desc");
static_assert(offsetof(zflac_cepstra_delta_desc, reserved) == 4, "reserved");
static_assert(offsetof(zflac_cepstra_delta_desc, src_device) == 8, "src_device");
static_assert(offsetof(zflac_cepstra_delta_desc, dst_device) == 16, "dst_device");
static_assert(offsetof(zflac_cepstra_delta_desc, rows) == 24, "rows");
static_assert(offsetof(zflac_cepstra_delta_desc, frames) == 32, "frames");
static_assert(offsetof(zflac_cepstra_delta_desc, valid_device) == 40, "valid_device");
static_assert(offsetof(zflac_cepstra_delta_desc, pad_value) == 48, "pad_value");
static_assert(offsetof(zflac_cepstra_delta_desc, reserved2) == 52, "reserved2");
static_assert(sizeof(zflac_mel_cmvn_desc) == 64 && sizeof(zflac_mel_desc) == 40, "the older descriptors did not grow");
static_assert(ZFLAC_HIP_ABI_VERSION == 5, "no bump");

#define NIN 23
#define NOUT 13

static float matrix[NOUT * NIN];

int main(void) {
    zflac_cepstra_desc d;
    zflac_cepstra_project_desc r;
    zflac_cepstra_delta_desc q;
    zflac_mel_cmvn_desc c;
    zflac_cepstra *p = NULL;
    float taps[8];
    int good, deltas_only, bad_window, neither, nan_matrix;
    size_t i;
    for (i = 0; i < sizeof matrix / sizeof matrix[0]; i++) matrix[i] = 0.25f;
    memset(&d, 0, sizeof d);
    d.size = (uint32_t)sizeof d;
    d.in_dtype = ZFLAC_EXPORT_F32;
    d.out_dtype = ZFLAC_EXPORT_BF16;
    d.layout = ZFLAC_MEL_FRAMES_FIRST;
    d.delta_order = 2;
    d.n_in = NIN;
    d.n_out = NOUT;
    d.delta_window = 2;
    d.matrix = matrix;
    good = zflac_hip_cepstra_create(&d, -1, &p); /* no such device: the arguments passed */
    d.delta_window = 6;
    bad_window = zflac_hip_cepstra_create(&d, -1, &p);
    d.delta_window = 2;
    matrix[NOUT * NIN - 1] = NAN;
    nan_matrix = zflac_hip_cepstra_create(&d, -1, &p);
    d.matrix = NULL;
    d.n_out = NIN;
    d.out_dtype = ZFLAC_EXPORT_F32;
    deltas_only = zflac_hip_cepstra_create(&d, -1, &p);
    d.delta_order = 0;
    d.delta_window = 0;
    neither = zflac_hip_cepstra_create(&d, -1, &p);
    memset(&r, 0, sizeof r);
    r.size = (uint32_t)sizeof r;
    memset(&q, 0, sizeof q);
    q.size = (uint32_t)sizeof q;
    memset(&c, 0, sizeof c);
    c.size = (uint32_t)sizeof c;
    zflac_hip_cepstra_destroy(NULL);
    printf("{\"good\": %d, \"bad_window\": %d, \"nan_matrix\": %d, \"deltas_only\": %d, \"neither\": %d, \"project_null\": %d, "
           "\"cmvn_null\": %d, \"deltas_null\": %d, \"features_null\": %u, \"scales_null\": %d, \"abi\": %d}\n",
           good, bad_window, nan_matrix, deltas_only, neither, zflac_hip_cepstra_project(NULL, &r, NULL),
           zflac_hip_cepstra_cmvn(NULL, &c, NULL), zflac_hip_cepstra_deltas(NULL, &q, NULL), zflac_hip_cepstra_features(NULL),
           zflac_hip_cepstra_delta_scales(NULL, 1, taps, 8), zflac_hip_abi_version());
    return 0;
}
