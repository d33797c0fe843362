// mel_host.cpp -- the feature plan (zflac_mel): its tables in device memory, its own stream, and
// the launch of k_mel. A run stages nothing: the tables never change and the arguments go by
// value, so runs of one plan on different streams may overlap.
#include "batch.h"
#include "launch.h"
#include "mel_plan.h"

struct zflac_mel {
    int device = 0;
    zflac::MelPlan plan;
    hipStream_t stream = nullptr;
    zflac::DevBuf<float> basis, filters;
    ~zflac_mel() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace zflac {

int mel_create(const zflac_mel_desc* d, int device, zflac_mel** out) {
    MelPlan p;
    const int rc = mel_plan_create(d, out, p);  // the arguments first, the device afterwards
    if (rc) return rc;
    *out = nullptr;
    return guarded([&]() -> int {
        std::vector<float> basis, filt;
        mel_tables(p, d->window, d->filters, basis, filt);
        int count = 0;
        if (device < 0 || hipGetDeviceCount(&count) != hipSuccess || device >= count) return E_DEVICE;
        DeviceScope scope(device);
        auto m = std::make_unique<zflac_mel>();
        m->device = device;
        m->plan = p;
        ck(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
        m->basis.alloc(basis.size());
        m->filters.alloc(filt.size());
        ck(hipMemcpy(m->basis.p, basis.data(), basis.size() * sizeof(float), hipMemcpyHostToDevice));
        ck(hipMemcpy(m->filters.p, filt.data(), filt.size() * sizeof(float), hipMemcpyHostToDevice));
        *out = m.release();
        return E_OK;
    });
}

int mel_run(zflac_mel* m, const float* wave, uint64_t rows, uint64_t wave_frames, uint64_t row_stride,
            uint64_t first_frame, uint64_t frames, void* dst, size_t dst_bytes, void* stream) {
    MelGrid g;
    const int rc = mel_plan_run(m ? &m->plan : nullptr, reinterpret_cast<uintptr_t>(wave), rows, wave_frames, row_stride,
                                first_frame, frames, reinterpret_cast<uintptr_t>(dst), dst_bytes, g);
    if (rc || g.blocks == 0) return rc;
    return guarded([&]() -> int {
        DeviceScope scope(m->device);
        const MelPlan& p = m->plan;
        MelArgs a;
        a.wave = wave;
        a.basis = m->basis.p;
        a.filters = m->filters.p;
        a.dst = dst;
        a.wave_frames = wave_frames;
        a.row_stride = row_stride;
        a.first_frame = first_frame;
        a.frames = frames;
        a.tiles = g.tiles;
        a.n_fft = p.n_fft;
        a.hop = p.hop;
        a.off = p.center ? p.n_fft / 2 : 0;
        a.n_bins = p.n_bins;
        a.bin_tiles = p.bin_tiles;
        a.scale = p.scale;
        a.floor = p.floor;
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : m->stream;
        ck(launch_mel(p.dtype, p.layout, p.m_tiles, a, rows, st));
        if (!stream) ck(hipStreamSynchronize(st));
        return E_OK;
    });
}

void mel_destroy(zflac_mel* m) {
    if (!m) return;
    try {
        DeviceScope scope(m->device);
        (void)hipDeviceSynchronize();  // a run on a caller's stream may still read the tables
        delete m;
    } catch (...) {
        delete m;
    }
}

}  // namespace zflac
