// cepstra_host.cpp -- the cepstra plan (zflac_cepstra): the matrix and the delta scales in device
// memory, the device, the dtypes and the plan's own stream, and the launches of k_mel_dct,
// k_mel_cmvn and k_mel_delta. A run stages nothing: the tables never change and the arguments go
// by value, so runs of one plan on different streams may overlap. The checks are cepstra_plan.h's.
#include "batch.h"
#include "cepstra_plan.h"
#include "launch.h"

struct zflac_cepstra {
    int device = 0;
    zflac::CepstraPlan plan;
    hipStream_t stream = nullptr;
    zflac::DevBuf<float> matrix, scales;
    ~zflac_cepstra() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace zflac {

int cepstra_create(const zflac_cepstra_desc* d, int device, zflac_cepstra** out) {
    CepstraPlan p;
    const int rc = cepstra_plan_create(d, out, p);  // the arguments first, the device afterwards
    if (rc) return rc;
    *out = nullptr;
    return guarded([&]() -> int {
        const std::vector<float> scales = cepstra_scale_table(p.delta_order, p.delta_window);
        int count = 0;
        if (device < 0 || hipGetDeviceCount(&count) != hipSuccess || device >= count) return E_DEVICE;
        DeviceScope scope(device);
        auto c = std::make_unique<zflac_cepstra>();
        c->device = device;
        c->plan = p;
        ck(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        if (p.has_matrix) {
            const size_t n = (size_t)p.n_out * p.n_in;
            c->matrix.alloc(n);
            ck(hipMemcpy(c->matrix.p, d->matrix, n * sizeof(float), hipMemcpyHostToDevice));
        }
        if (!scales.empty()) {
            c->scales.alloc(scales.size());
            ck(hipMemcpy(c->scales.p, scales.data(), scales.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        *out = c.release();
        return E_OK;
    });
}

uint32_t cepstra_features(const zflac_cepstra* c) { return c ? c->plan.features() : 0; }

int cepstra_delta_scales_of(const zflac_cepstra* c, uint32_t order, float* out, uint32_t cap) {
    if (!c || !out || order > c->plan.delta_order) return -E_INVALID_ARGUMENT;
    const std::vector<double> s = cepstra_delta_scales(order, order ? c->plan.delta_window : 1);
    if (cap < s.size()) return -E_INVALID_ARGUMENT;
    for (size_t i = 0; i < s.size(); i++) out[i] = (float)s[i];
    return (int)s.size();
}

// launches(st) on the plan's device: on the caller's stream, or on the plan's own, and then the
// call returns when the work is done
template <typename F>
static int cepstra_on_stream(zflac_cepstra* c, void* stream, F&& launches) {
    return guarded([&]() -> int {
        DeviceScope scope(c->device);
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
        launches(st);
        if (!stream) ck(hipStreamSynchronize(st));
        return E_OK;
    });
}

int cepstra_project(zflac_cepstra* c, const zflac_cepstra_project_desc* r, void* stream) {
    CepstraGrid g;
    const int rc = cepstra_plan_project(c ? &c->plan : nullptr, r, g);
    if (rc || g.passes == 0) return rc;
    return cepstra_on_stream(c, stream, [&](hipStream_t st) {
        const CepstraPlan& p = c->plan;
        MelDctArgs a;
        a.src = r->src_device;
        a.dst = r->dst_device;
        a.T = c->matrix.p;
        a.frames = r->frames;
        a.tiles = g.tiles;
        a.total = g.passes;
        a.n_in = p.n_in;
        a.n_out = p.n_out;
        ck(launch_mel_dct(p.in_dtype, p.out_dtype, p.layout, a, st));
    });
}

// zflac_hip_mel_cmvn's launch over n_out bins
int cepstra_cmvn(zflac_cepstra* c, const zflac_mel_cmvn_desc* d, void* stream) {
    uint64_t passes = 0;
    const int rc = cepstra_plan_cmvn(c ? &c->plan : nullptr, d, passes);
    if (rc || passes == 0) return rc;
    return cepstra_on_stream(c, stream, [&](hipStream_t st) {
        const CepstraPlan& p = c->plan;
        MelCmvnArgs a;
        a.feat = d->feat_device;
        a.valid = d->valid_device;
        a.mean = d->mean_device;
        a.std = d->std_device;
        a.rows = d->rows;
        a.frames = d->frames;
        a.total = passes;
        a.n_bins = p.n_out;
        a.mode = d->mode;
        a.ddof = d->ddof;
        a.eps = d->eps;
        a.pad_value = d->pad_value;
        ck(launch_mel_cmvn(p.out_dtype, p.layout, a, st));
    });
}

int cepstra_deltas(zflac_cepstra* c, const zflac_cepstra_delta_desc* r, void* stream) {
    CepstraGrid g;
    const int rc = cepstra_plan_deltas(c ? &c->plan : nullptr, r, g);
    if (rc || g.passes == 0) return rc;
    return cepstra_on_stream(c, stream, [&](hipStream_t st) {
        const CepstraPlan& p = c->plan;
        MelDeltaArgs a;
        a.src = r->src_device;
        a.dst = r->dst_device;
        a.scales = c->scales.p;
        a.valid = r->valid_device;
        a.frames = r->frames;
        a.tiles = g.tiles;
        a.total = g.passes;
        a.C = p.n_out;
        a.order = p.delta_order;
        a.window = p.delta_window;
        a.pad_value = r->pad_value;
        ck(launch_mel_delta(p.out_dtype, p.layout, a, st));
    });
}

void cepstra_destroy(zflac_cepstra* c) {
    if (!c) return;
    try {
        DeviceScope scope(c->device);
        (void)hipDeviceSynchronize();  // a run on a caller's stream may still read the tables
        delete c;
    } catch (...) {
        delete c;
    }
}

}  // namespace zflac
