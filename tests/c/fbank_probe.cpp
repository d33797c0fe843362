// fbank_probe.cpp -- tests/test_fbank_plan.py's view of the framed half of
// zflac_amd/csrc/mel_plan.cpp (mel_plan_create_framed, the folded tables, mel_plan_frames, the
// ZFLAC_PAD_MIRROR rule of mel_plan_run_ex, mel_plan_cmvn): a program of its own (plain g++, no
// HIP; also built with -fsanitize=address,undefined) that takes one case on its command line and
// prints what the planner answers. Floats that a rule is about go by their bits.
//
//   create MATH SIZE DTYPE LAYOUT SCALE CENTER N HOP BINS RESERVED FLOOR FLAGS
//          FSIZE NW FRAMING DC PREEMPH_BITS GAIN_BITS FRESERVED
//       FLAGS: 1 d NULL, 2 out NULL, 4 window NULL, 8 filters NULL, 16 a NaN in window[NW - 1],
//       32 an infinity in the filters, 64 f NULL, 128 a NaN in window[NW] (behind the window: not
//       read). SIZE / FSIZE -1 = the struct's sizeof.
//       prints: rc win_length span off framing math k_blocks n_pieces
//   tables MATH N NW HOP BINS FRAMING CENTER DC PREEMPH_BITS GAIN_BITS FILE
//       the probe's window (NW values) and filters. FILE receives the f32 basis (MATH 0) or the
//       bf16 pieces, then the filters. prints: rc basis_floats piece_elems filter_floats span k_blocks
//   identity MATH N HOP BINS CENTER
//       prints: rc equal -- whether the framed plan with NW = N, _STFT, no operator holds the
//       tables of mel_plan_create_ex byte for byte (and the same plan fields)
//   frames FRAMING N NW HOP CENTER n...
//       prints mel_plan_frames of every n, one per line
//   runex PAD FRAMING CENTER NW
//       prints the rc of mel_plan_run_ex for an otherwise good descriptor on a plan N = 16, hop = 3
//   cmvn SIZE MODE DDOF RESERVED FEAT ROWS FRAMES VALID MEAN STD EPS_BITS PAD_BITS LAYOUT FLAGS
//       FEAT / VALID / MEAN / STD are addresses (never read). FLAGS: 1 plan NULL, 2 c NULL.
//       a plan of 80 bins, f32. prints: rc passes
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "mel_plan.h"

using namespace zflac;

static float probe_window(uint32_t n) { return 0.25f + (float)((n * 37u) % 101u) / 128.0f; }
static float probe_filter(uint32_t m, uint32_t k) { return (float)((m * 131u + k * 7u) % 97u) / 64.0f - 0.5f; }

static unsigned long long u64(const char* s) { return std::strtoull(s, nullptr, 0); }
static float bits(const char* s) {
    const uint32_t u = (uint32_t)u64(s);
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}

static zflac_mel_desc good_desc(uint32_t n, uint32_t nw, uint32_t hop, uint32_t bins, uint32_t center, std::vector<float>& w,
                                std::vector<float>& f) {
    w.resize(nw);
    f.resize((size_t)bins * (n / 2 + 1));
    for (uint32_t i = 0; i < nw; i++) w[i] = probe_window(i);
    for (uint32_t m = 0; m < bins; m++)
        for (uint32_t k = 0; k < n / 2 + 1; k++) f[(size_t)m * (n / 2 + 1) + k] = probe_filter(m, k);
    zflac_mel_desc d;
    std::memset(&d, 0, sizeof d);
    d.size = sizeof d;
    d.dtype = ZFLAC_EXPORT_F32;
    d.center = (uint8_t)center;
    d.n_fft = (uint16_t)n;
    d.hop = (uint16_t)hop;
    d.n_bins = (uint16_t)bins;
    d.window = w.data();
    d.filters = f.data();
    return d;
}

static zflac_mel_frame_desc frame_desc(uint32_t nw, uint32_t framing, uint32_t dc, float a, float g) {
    zflac_mel_frame_desc f;
    std::memset(&f, 0, sizeof f);
    f.size = sizeof f;
    f.win_length = (uint16_t)nw;
    f.framing = (uint8_t)framing;
    f.remove_dc = (uint8_t)dc;
    f.preemphasis = a;
    f.sample_scale = g;
    return f;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "create" && argc == 21) {
        const uint32_t math = (uint32_t)u64(argv[2]);
        const long size = std::strtol(argv[3], nullptr, 0), fsize = std::strtol(argv[14], nullptr, 0);
        const uint32_t n = (uint32_t)u64(argv[8]), bins = (uint32_t)u64(argv[10]), nw = (uint32_t)u64(argv[15]);
        const unsigned flags = (unsigned)u64(argv[13]);
        std::vector<float> w(4097, 0.5f), f((size_t)257 * 2049, 0.25f);
        if (flags & 16) w[nw > 0 && nw <= 2048 ? nw - 1 : 0] = std::numeric_limits<float>::quiet_NaN();
        if (flags & 128) w[nw <= 2048 ? nw : 4096] = std::numeric_limits<float>::quiet_NaN();
        if (flags & 32) f[bins > 0 && bins <= 256 && n <= 2048 ? (size_t)bins * (n / 2 + 1) - 1 : 0] = std::numeric_limits<float>::infinity();
        zflac_mel_desc d;
        std::memset(&d, 0, sizeof d);
        d.size = size < 0 ? (uint32_t)sizeof d : (uint32_t)size;
        d.dtype = (uint8_t)u64(argv[4]);
        d.layout = (uint8_t)u64(argv[5]);
        d.scale = (uint8_t)u64(argv[6]);
        d.center = (uint8_t)u64(argv[7]);
        d.n_fft = (uint16_t)n;
        d.hop = (uint16_t)u64(argv[9]);
        d.n_bins = (uint16_t)bins;
        d.reserved = (uint16_t)u64(argv[11]);
        d.floor = std::strtof(argv[12], nullptr);
        d.window = flags & 4 ? nullptr : w.data();
        d.filters = flags & 8 ? nullptr : f.data();
        zflac_mel_frame_desc fd = frame_desc(nw, (uint32_t)u64(argv[16]), (uint32_t)u64(argv[17]), bits(argv[18]), bits(argv[19]));
        fd.size = fsize < 0 ? (uint32_t)sizeof fd : (uint32_t)fsize;
        fd.reserved = (uint32_t)u64(argv[20]);
        MelPlan p;
        int out = 0;
        const int rc = mel_plan_create_framed(flags & 1 ? nullptr : &d, flags & 64 ? nullptr : &fd, math,
                                              flags & 2 ? nullptr : &out, p);
        std::printf("%d %u %u %d %u %u %u %u\n", rc, p.win_length, p.span, p.off, p.framing, p.math, p.k_blocks, p.n_pieces);
        return 0;
    }
    if (cmd == "tables" && argc == 13) {
        const uint32_t math = (uint32_t)u64(argv[2]), n = (uint32_t)u64(argv[3]), nw = (uint32_t)u64(argv[4]);
        std::vector<float> w, f, basis, filt;
        std::vector<uint16_t> pieces;
        const zflac_mel_desc d = good_desc(n, nw, (uint32_t)u64(argv[5]), (uint32_t)u64(argv[6]), (uint32_t)u64(argv[8]), w, f);
        const zflac_mel_frame_desc fd = frame_desc(nw, (uint32_t)u64(argv[7]), (uint32_t)u64(argv[9]), bits(argv[10]), bits(argv[11]));
        MelPlan p;
        int out = 0;
        const int rc = mel_plan_create_framed(&d, &fd, math, &out, p);
        if (rc == 0) {
            if (p.math == ZFLAC_MEL_MATH_F32) mel_tables(p, d.window, d.filters, basis, filt);
            else mel_bf16_tables(p, d.window, d.filters, pieces, filt);
            std::FILE* fh = std::fopen(argv[12], "wb");
            if (!fh) return 2;
            if (!basis.empty()) std::fwrite(basis.data(), sizeof(float), basis.size(), fh);
            if (!pieces.empty()) std::fwrite(pieces.data(), sizeof(uint16_t), pieces.size(), fh);
            std::fwrite(filt.data(), sizeof(float), filt.size(), fh);
            std::fclose(fh);
        }
        std::printf("%d %zu %zu %zu %u %u\n", rc, basis.size(), pieces.size(), filt.size(), p.span, p.k_blocks);
        return 0;
    }
    if (cmd == "identity" && argc == 7) {
        const uint32_t math = (uint32_t)u64(argv[2]), n = (uint32_t)u64(argv[3]);
        std::vector<float> w, f, b0, f0, b1, f1;
        std::vector<uint16_t> p0, p1;
        const zflac_mel_desc d = good_desc(n, n, (uint32_t)u64(argv[4]), (uint32_t)u64(argv[5]), (uint32_t)u64(argv[6]), w, f);
        const zflac_mel_frame_desc fd = frame_desc(n, ZFLAC_FRAMING_STFT, 0, 0.0f, 1.0f);
        MelPlan a, b;
        int out = 0;
        const int rc0 = mel_plan_create_ex(&d, math, &out, a), rc = mel_plan_create_framed(&d, &fd, math, &out, b);
        bool equal = rc0 == 0 && rc == 0;
        if (equal) {
            if (math == ZFLAC_MEL_MATH_F32) {
                mel_tables(a, d.window, d.filters, b0, f0);
                mel_tables(b, d.window, d.filters, b1, f1);
            } else {
                mel_bf16_tables(a, d.window, d.filters, p0, f0);
                mel_bf16_tables(b, d.window, d.filters, p1, f1);
            }
            equal = b0.size() == b1.size() && p0.size() == p1.size() && f0.size() == f1.size() &&
                    (b0.empty() || !std::memcmp(b0.data(), b1.data(), b0.size() * sizeof(float))) &&
                    (p0.empty() || !std::memcmp(p0.data(), p1.data(), p0.size() * sizeof(uint16_t))) &&
                    !std::memcmp(f0.data(), f1.data(), f0.size() * sizeof(float)) && b0.size() + p0.size() > 0 &&
                    a.span == b.span && a.off == b.off && a.win_length == b.win_length && a.k_blocks == b.k_blocks &&
                    a.n_pieces == b.n_pieces && a.bin_tiles == b.bin_tiles && a.m_tiles == b.m_tiles && a.framing == b.framing;
        }
        std::printf("%d %d\n", rc, equal ? 1 : 0);
        return 0;
    }
    if (cmd == "frames" && argc >= 8) {
        const uint32_t n = (uint32_t)u64(argv[3]), nw = (uint32_t)u64(argv[4]);
        std::vector<float> w, f;
        const zflac_mel_desc d = good_desc(n, nw, (uint32_t)u64(argv[5]), 2, (uint32_t)u64(argv[6]), w, f);
        const zflac_mel_frame_desc fd = frame_desc(nw, (uint32_t)u64(argv[2]), 0, 0.0f, 1.0f);
        MelPlan p;
        int out = 0;
        if (mel_plan_create_framed(&d, &fd, ZFLAC_MEL_MATH_F32, &out, p)) return 2;
        for (int i = 7; i < argc; i++) std::printf("%llu\n", (unsigned long long)mel_plan_frames(p, u64(argv[i])));
        return 0;
    }
    if (cmd == "runex" && argc == 6) {
        const uint32_t nw = (uint32_t)u64(argv[5]);
        std::vector<float> w, f;
        const zflac_mel_desc d = good_desc(16, nw, 3, 5, (uint32_t)u64(argv[4]), w, f);
        const zflac_mel_frame_desc fd = frame_desc(nw, (uint32_t)u64(argv[3]), 0, 0.0f, 1.0f);
        MelPlan p;
        int out = 0;
        if (mel_plan_create_framed(&d, &fd, ZFLAC_MEL_MATH_F32, &out, p)) return 2;
        zflac_mel_run_desc r;
        std::memset(&r, 0, sizeof r);
        r.size = sizeof r;
        r.pad = (uint8_t)u64(argv[2]);
        r.wave_device = reinterpret_cast<const float*>(uintptr_t(0x1000));
        r.rows = 2;
        r.wave_frames = r.row_stride = 100;
        r.frames = 7;
        r.dst_device = reinterpret_cast<void*>(uintptr_t(0x2000));
        r.dst_bytes = 2 * 5 * 7 * 4;
        MelGrid g;
        std::printf("%d\n", mel_plan_run_ex(&p, &r, g));
        return 0;
    }
    if (cmd == "cmvn" && argc == 16) {
        std::vector<float> w, f;
        zflac_mel_desc d = good_desc(512, 512, 160, 80, 0, w, f);
        d.layout = (uint8_t)u64(argv[14]);
        MelPlan p;
        int out = 0;
        if (mel_plan_create(&d, &out, p)) return 2;
        const long size = std::strtol(argv[2], nullptr, 0);
        const unsigned flags = (unsigned)u64(argv[15]);
        zflac_mel_cmvn_desc c;
        std::memset(&c, 0, sizeof c);
        c.size = size < 0 ? (uint32_t)sizeof c : (uint32_t)size;
        c.mode = (uint8_t)u64(argv[3]);
        c.ddof = (uint8_t)u64(argv[4]);
        c.reserved = (uint16_t)u64(argv[5]);
        c.feat_device = reinterpret_cast<void*>(uintptr_t(u64(argv[6])));
        c.rows = u64(argv[7]);
        c.frames = u64(argv[8]);
        c.valid_device = reinterpret_cast<const uint64_t*>(uintptr_t(u64(argv[9])));
        c.mean_device = reinterpret_cast<float*>(uintptr_t(u64(argv[10])));
        c.std_device = reinterpret_cast<float*>(uintptr_t(u64(argv[11])));
        c.eps = bits(argv[12]);
        c.pad_value = bits(argv[13]);
        uint64_t passes = 0;
        const int rc = mel_plan_cmvn(flags & 1 ? nullptr : &p, flags & 2 ? nullptr : &c, passes);
        std::printf("%d %llu\n", rc, (unsigned long long)passes);
        return 0;
    }
    std::fprintf(stderr, "fbank_probe: unknown case\n");
    return 64;
}
