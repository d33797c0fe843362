// mel_host.cpp -- the feature plan (zflac_mel): its tables in device memory, its own stream, and
// the launches of k_mel, k_mel_ex and k_mel_norm, or of k_mel_split for a split-bf16 plan, and of
// k_mel_cmvn behind them. A run stages nothing: the tables never change
// and the arguments go by value, so runs of one plan on different streams may overlap.
#include "batch.h"
#include "launch.h"
#include "mel_plan.h"

struct zflac_mel {
    int device = 0;
    zflac::MelPlan plan;
    hipStream_t stream = nullptr;
    zflac::DevBuf<float> basis, filters;
    zflac::DevBuf<uint16_t> pieces;  // a split plan's basis (mel_plan.h), in place of `basis`
    ~zflac_mel() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace zflac {

// The tables of a checked plan, then the device
static int mel_build(const MelPlan& p, const zflac_mel_desc* d, int device, zflac_mel** out) {
    *out = nullptr;
    return guarded([&]() -> int {
        std::vector<float> basis, filt;
        std::vector<uint16_t> pieces;
        if (p.math == ZFLAC_MEL_MATH_F32) mel_tables(p, d->window, d->filters, basis, filt);
        else mel_bf16_tables(p, d->window, d->filters, pieces, filt);
        int count = 0;
        if (device < 0 || hipGetDeviceCount(&count) != hipSuccess || device >= count) return E_DEVICE;
        DeviceScope scope(device);
        auto m = std::make_unique<zflac_mel>();
        m->device = device;
        m->plan = p;
        ck(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
        m->filters.alloc(filt.size());
        if (p.math == ZFLAC_MEL_MATH_F32) {
            m->basis.alloc(basis.size());
            ck(hipMemcpy(m->basis.p, basis.data(), basis.size() * sizeof(float), hipMemcpyHostToDevice));
        } else {
            m->pieces.alloc(pieces.size());
            ck(hipMemcpy(m->pieces.p, pieces.data(), pieces.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        }
        ck(hipMemcpy(m->filters.p, filt.data(), filt.size() * sizeof(float), hipMemcpyHostToDevice));
        *out = m.release();
        return E_OK;
    });
}

int mel_create(const zflac_mel_desc* d, uint32_t math, int device, zflac_mel** out) {
    MelPlan p;
    const int rc = mel_plan_create_ex(d, math, out, p);  // the arguments first, the device afterwards
    if (rc) return rc;
    return mel_build(p, d, device, out);
}

int mel_create_framed(const zflac_mel_desc* d, const zflac_mel_frame_desc* f, uint32_t math, int device, zflac_mel** out) {
    MelPlan p;
    const int rc = mel_plan_create_framed(d, f, math, out, p);
    if (rc) return rc;
    return mel_build(p, d, device, out);
}

uint64_t mel_plan_frames_of(const zflac_mel* m, uint64_t n_samples) { return m ? mel_plan_frames(m->plan, n_samples) : 0; }

// The launch arguments of a run the planner has accepted; what only zflac_hip_mel_run_ex can ask
// for is off unless given
static MelExArgs mel_args(const zflac_mel* m, const float* wave, uint64_t wave_frames, uint64_t row_stride,
                          uint64_t first_frame, uint64_t frames, void* dst, const MelGrid& g,
                          const uint64_t* lengths = nullptr, float* row_max = nullptr, uint32_t pad = ZFLAC_PAD_ZEROS) {
    const MelPlan& p = m->plan;
    MelExArgs e;
    MelArgs& a = e.a;
    a.wave = wave;
    a.basis = m->basis.p;
    a.filters = m->filters.p;
    a.dst = dst;
    a.wave_frames = wave_frames;
    a.row_stride = row_stride;
    a.first_frame = first_frame;
    a.frames = frames;
    a.tiles = g.tiles;
    // the f32 table's sample rows; a split plan's frame length (its kernel reads zeros at and past it)
    a.span = p.math == ZFLAC_MEL_MATH_F32 ? p.span : p.win_length;
    a.hop = p.hop;
    a.off = p.off;
    a.n_bins = p.n_bins;
    a.bin_tiles = p.bin_tiles;
    a.scale = p.scale;
    a.floor = p.floor;
    e.lengths = lengths;
    e.row_max = row_max;
    e.pad = pad;
    e.pad_half = p.n_fft / 2;
    return e;
}

int mel_math(const zflac_mel* m) { return m ? (int)m->plan.math : -E_INVALID_ARGUMENT; }

// A split plan's launch: one kernel for both run calls
static hipError_t launch_split(const zflac_mel* m, const MelExArgs& e, uint64_t rows, hipStream_t st) {
    const MelPlan& p = m->plan;
    MelSplitArgs s;
    s.e = e;
    s.pieces = m->pieces.p;
    s.k_blocks = p.k_blocks;
    return launch_mel_split(p.dtype, p.layout, p.m_tiles, p.math == ZFLAC_MEL_MATH_BF16X6 ? 6 : 3, p.framed(), s, rows, st);
}

// launches(st) on the plan's device: on the caller's stream, or on the plan's own, and then the
// call returns when the work is done
template <typename F>
static int mel_on_stream(zflac_mel* m, void* stream, F&& launches) {
    return guarded([&]() -> int {
        DeviceScope scope(m->device);
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : m->stream;
        launches(st);
        if (!stream) ck(hipStreamSynchronize(st));
        return E_OK;
    });
}

int mel_run(zflac_mel* m, const float* wave, uint64_t rows, uint64_t wave_frames, uint64_t row_stride,
            uint64_t first_frame, uint64_t frames, void* dst, size_t dst_bytes, void* stream) {
    MelGrid g;
    const int rc = mel_plan_run(m ? &m->plan : nullptr, reinterpret_cast<uintptr_t>(wave), rows, wave_frames, row_stride,
                                first_frame, frames, reinterpret_cast<uintptr_t>(dst), dst_bytes, g);
    if (rc || g.blocks == 0) return rc;
    return mel_on_stream(m, stream, [&](hipStream_t st) {
        const MelPlan& p = m->plan;
        const MelExArgs e = mel_args(m, wave, wave_frames, row_stride, first_frame, frames, dst, g);
        if (p.math == ZFLAC_MEL_MATH_F32) ck(launch_mel(p.dtype, p.layout, p.m_tiles, e.a, rows, st));
        else ck(launch_split(m, e, rows, st));
    });
}

// Up to three things on the one stream: row_max = -inf, k_mel (k_mel_ex unless the descriptor is
// zflac_hip_mel_run's), k_mel_norm. Nothing is staged from the host.
int mel_run_ex(zflac_mel* m, const zflac_mel_run_desc* r, void* stream) {
    MelGrid g;
    const int rc = mel_plan_run_ex(m ? &m->plan : nullptr, r, g);
    if (rc || g.blocks == 0) return rc;
    return mel_on_stream(m, stream, [&](hipStream_t st) {
        const MelPlan& p = m->plan;
        const MelExArgs e = mel_args(m, r->wave_device, r->wave_frames, r->row_stride, r->first_frame, r->frames,
                                     r->dst_device, g, r->lengths_device, r->row_max_device, r->pad);
        if (e.row_max) ck(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(e.row_max), (int)0xFF800000u, r->rows, st));
        if (p.math != ZFLAC_MEL_MATH_F32) ck(launch_split(m, e, r->rows, st));
        else if (mel_run_is_plain(*r)) ck(launch_mel(p.dtype, p.layout, p.m_tiles, e.a, r->rows, st));
        else ck(launch_mel_ex(p.dtype, p.layout, p.m_tiles, p.framed(), e, r->rows, st));
        if (r->norm == ZFLAC_NORM_ROW_MAX) {
            MelNormArgs n;
            n.dst = r->dst_device;
            n.row_max = r->row_max_device;
            n.row_elems = (uint64_t)p.n_bins * r->frames;
            n.chunks = (n.row_elems - 1) / MEL_NORM_CHUNK + 1;
            n.total = r->rows * n.chunks;
            n.range = r->range;
            n.add = r->add;
            n.mul = r->mul;
            ck(launch_mel_norm(p.dtype, n, st));
        }
    });
}

// One launch of k_mel_cmvn; nothing is staged from the host
int mel_cmvn(zflac_mel* m, const zflac_mel_cmvn_desc* c, void* stream) {
    uint64_t passes = 0;
    const int rc = mel_plan_cmvn(m ? &m->plan : nullptr, c, passes);
    if (rc || passes == 0) return rc;
    return mel_on_stream(m, stream, [&](hipStream_t st) {
        const MelPlan& p = m->plan;
        MelCmvnArgs a;
        a.feat = c->feat_device;
        a.valid = c->valid_device;
        a.mean = c->mean_device;
        a.std = c->std_device;
        a.rows = c->rows;
        a.frames = c->frames;
        a.total = passes;
        a.n_bins = p.n_bins;
        a.mode = c->mode;
        a.ddof = c->ddof;
        a.eps = c->eps;
        a.pad_value = c->pad_value;
        ck(launch_mel_cmvn(p.dtype, p.layout, a, st));
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
