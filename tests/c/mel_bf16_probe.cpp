// mel_bf16_probe.cpp -- tests/test_mel_bf16_plan.py's view of the split-bf16 half of
// zflac_amd/csrc/mel_plan.cpp (mel_plan_create_ex, the piece table): a program of its own (plain
// g++, no HIP; also built with -fsanitize=address,undefined) that takes one case on its command
// line and prints what the planner answers.
//
//   create MATH SIZE DTYPE LAYOUT SCALE CENTER N HOP BINS RESERVED FLOOR FLAGS
//       FLAGS: 1 d NULL, 2 out NULL, 4 window NULL, 8 filters NULL, 16 a NaN in the window,
//       32 an infinity in the filters. SIZE -1 = sizeof(zflac_mel_desc).
//       prints: rc math k_blocks n_pieces piece_elems
//   tables MATH N HOP BINS FILE
//       the probe's window and filters (mel_probe.cpp's). FILE receives the f32 basis and filters
//       of mel_plan_create + mel_tables, then what a plan of MATH holds: the same two tables again
//       (MATH 0, through mel_plan_create_ex) or the bf16 pieces (uint16) and the filters.
//       prints: rc basis_floats filter_floats piece_elems
//   index MATH N BINS
//       prints mel_bf16_basis_index of every (im, piece, n < 16 k_blocks, k < 32 bin_tiles), one per line
//   split BITS...
//       prints the three pieces (mel_bf16_split) of every f32 given by its bits, one value per line
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

static zflac_mel_desc good_desc(uint32_t n, uint32_t hop, uint32_t bins, std::vector<float>& w, std::vector<float>& f) {
    w.resize(n);
    f.resize((size_t)bins * (n / 2 + 1));
    for (uint32_t i = 0; i < n; i++) w[i] = probe_window(i);
    for (uint32_t m = 0; m < bins; m++)
        for (uint32_t k = 0; k < n / 2 + 1; k++) f[(size_t)m * (n / 2 + 1) + k] = probe_filter(m, k);
    zflac_mel_desc d;
    std::memset(&d, 0, sizeof d);
    d.size = sizeof d;
    d.dtype = ZFLAC_EXPORT_F32;
    d.n_fft = (uint16_t)n;
    d.hop = (uint16_t)hop;
    d.n_bins = (uint16_t)bins;
    d.window = w.data();
    d.filters = f.data();
    return d;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "create" && argc == 14) {
        const uint32_t math = (uint32_t)u64(argv[2]);
        const long size = std::strtol(argv[3], nullptr, 0);
        const uint32_t n = (uint32_t)u64(argv[8]), bins = (uint32_t)u64(argv[10]);
        const unsigned flags = (unsigned)u64(argv[13]);
        std::vector<float> w(4096, 0.5f), f((size_t)257 * 2049, 0.25f);
        if (flags & 16) w[n > 0 && n <= 2048 ? n - 1 : 0] = std::numeric_limits<float>::quiet_NaN();
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
        MelPlan p;
        int out = 0;
        const int rc = mel_plan_create_ex(flags & 1 ? nullptr : &d, math, flags & 2 ? nullptr : &out, p);
        std::printf("%d %u %u %u %zu\n", rc, p.math, p.k_blocks, p.n_pieces, p.piece_elems());
        return 0;
    }
    if (cmd == "tables" && argc == 7) {
        const uint32_t math = (uint32_t)u64(argv[2]);
        std::vector<float> w, f, basis0, filt0, basis, filt;
        std::vector<uint16_t> pieces;
        const zflac_mel_desc d = good_desc((uint32_t)u64(argv[3]), (uint32_t)u64(argv[4]), (uint32_t)u64(argv[5]), w, f);
        MelPlan p0, p;
        int out = 0;
        if (mel_plan_create(&d, &out, p0)) return 2;
        mel_tables(p0, d.window, d.filters, basis0, filt0);
        const int rc = mel_plan_create_ex(&d, math, &out, p);
        if (rc == 0) {
            if (p.math == ZFLAC_MEL_MATH_F32) mel_tables(p, d.window, d.filters, basis, filt);
            else mel_bf16_tables(p, d.window, d.filters, pieces, filt);
            std::FILE* fh = std::fopen(argv[6], "wb");
            if (!fh) return 2;
            std::fwrite(basis0.data(), sizeof(float), basis0.size(), fh);
            std::fwrite(filt0.data(), sizeof(float), filt0.size(), fh);
            if (!basis.empty()) std::fwrite(basis.data(), sizeof(float), basis.size(), fh);
            if (!pieces.empty()) std::fwrite(pieces.data(), sizeof(uint16_t), pieces.size(), fh);
            std::fwrite(filt.data(), sizeof(float), filt.size(), fh);
            std::fclose(fh);
        }
        std::printf("%d %zu %zu %zu\n", rc, basis0.size(), filt0.size(), pieces.size());
        return 0;
    }
    if (cmd == "index" && argc == 5) {
        std::vector<float> w, f;
        const zflac_mel_desc d = good_desc((uint32_t)u64(argv[3]), 1, (uint32_t)u64(argv[4]), w, f);
        MelPlan p;
        int out = 0;
        if (mel_plan_create_ex(&d, (uint32_t)u64(argv[2]), &out, p)) return 2;
        for (uint32_t im = 0; im < 2; im++)
            for (uint32_t piece = 0; piece < p.n_pieces; piece++)
                for (uint32_t n = 0; n < p.k_blocks * MEL_BF16_K; n++)
                    for (uint32_t k = 0; k < p.bin_tiles * MEL_TILE; k++)
                        std::printf("%zu\n", mel_bf16_basis_index(p, k, n, im, piece));
        return 0;
    }
    if (cmd == "split" && argc >= 3) {
        for (int i = 2; i < argc; i++) {
            const uint32_t u = (uint32_t)u64(argv[i]);
            float v;
            std::memcpy(&v, &u, 4);
            uint16_t h[3];
            mel_bf16_split(v, h);
            std::printf("%u %u %u\n", h[0], h[1], h[2]);
        }
        return 0;
    }
    std::fprintf(stderr, "mel_bf16_probe: unknown case\n");
    return 64;
}
