// mel_probe.cpp -- tests/test_mel_plan.py's view of zflac_amd/csrc/mel_plan.cpp: a program of its
// own (plain g++, no HIP; also built with -fsanitize=address,undefined) that takes one case on
// its command line and prints what the planner answers.
//
//   create SIZE DTYPE LAYOUT SCALE CENTER N HOP BINS RESERVED FLOOR FLAGS
//       FLAGS: 1 d NULL, 2 out NULL, 4 window NULL, 8 filters NULL, 16 a NaN in the window,
//       32 an infinity in the filters. SIZE -1 = sizeof(zflac_mel_desc).
//       prints: rc K bin_tiles m_tiles basis_floats filter_floats
//   tables N HOP BINS FILE
//       the tables of the probe's window and filters (below), written to FILE as float32:
//       basis, then filters. prints: rc basis_floats filter_floats
//   index N BINS
//       prints mel_basis_index of every (n, k, im) and mel_filter_index of every (m, k), one per line
//   run PLAN WAVE ROWS WAVE_FRAMES ROW_STRIDE FIRST FRAMES DST DST_BYTES N HOP BINS DTYPE
//       PLAN 0 = no plan. prints: rc tiles blocks
//   frames SAMPLES N HOP CENTER
//   layout
//       prints sizeof(zflac_mel_desc) and the offset of every field
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "mel_plan.h"

using namespace zflac;

// the window and the filters every case uses: tests/test_mel_plan.py has the same arithmetic
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
    if (cmd == "create" && argc == 13) {
        const long size = std::strtol(argv[2], nullptr, 0);
        const uint32_t n = (uint32_t)u64(argv[7]), bins = (uint32_t)u64(argv[9]);
        const unsigned flags = (unsigned)u64(argv[12]);
        // arrays long enough for whatever the planner may read of a descriptor it accepts
        std::vector<float> w(4096, 0.5f), f((size_t)257 * 2049, 0.25f);
        if (flags & 16) w[n > 0 && n <= 2048 ? n - 1 : 0] = std::numeric_limits<float>::quiet_NaN();
        if (flags & 32) f[bins > 0 && bins <= 256 && n <= 2048 ? (size_t)bins * (n / 2 + 1) - 1 : 0] = std::numeric_limits<float>::infinity();
        zflac_mel_desc d;
        std::memset(&d, 0, sizeof d);
        d.size = size < 0 ? (uint32_t)sizeof d : (uint32_t)size;
        d.dtype = (uint8_t)u64(argv[3]);
        d.layout = (uint8_t)u64(argv[4]);
        d.scale = (uint8_t)u64(argv[5]);
        d.center = (uint8_t)u64(argv[6]);
        d.n_fft = (uint16_t)n;
        d.hop = (uint16_t)u64(argv[8]);
        d.n_bins = (uint16_t)bins;
        d.reserved = (uint16_t)u64(argv[10]);
        d.floor = std::strtof(argv[11], nullptr);
        d.window = flags & 4 ? nullptr : w.data();
        d.filters = flags & 8 ? nullptr : f.data();
        MelPlan p;
        int out = 0;
        const int rc = mel_plan_create(flags & 1 ? nullptr : &d, flags & 2 ? nullptr : &out, p);
        std::printf("%d %u %u %u %zu %zu\n", rc, p.K, p.bin_tiles, p.m_tiles, p.basis_floats(), p.filter_floats());
        return 0;
    }
    if (cmd == "tables" && argc == 6) {
        std::vector<float> w, f, basis, filt;
        const zflac_mel_desc d = good_desc((uint32_t)u64(argv[2]), (uint32_t)u64(argv[3]), (uint32_t)u64(argv[4]), w, f);
        MelPlan p;
        int out = 0;
        const int rc = mel_plan_create(&d, &out, p);
        if (rc == 0) {
            mel_tables(p, d.window, d.filters, basis, filt);
            std::FILE* fh = std::fopen(argv[5], "wb");
            if (!fh) return 2;
            std::fwrite(basis.data(), sizeof(float), basis.size(), fh);
            std::fwrite(filt.data(), sizeof(float), filt.size(), fh);
            std::fclose(fh);
        }
        std::printf("%d %zu %zu\n", rc, basis.size(), filt.size());
        return 0;
    }
    if (cmd == "index" && argc == 4) {
        std::vector<float> w, f;
        const zflac_mel_desc d = good_desc((uint32_t)u64(argv[2]), 1, (uint32_t)u64(argv[3]), w, f);
        MelPlan p;
        int out = 0;
        if (mel_plan_create(&d, &out, p)) return 2;
        for (uint32_t im = 0; im < 2; im++)
            for (uint32_t n = 0; n < p.n_fft; n++)
                for (uint32_t k = 0; k < p.K; k++) std::printf("%zu\n", mel_basis_index(p, n, k, im));
        for (uint32_t m = 0; m < p.n_bins; m++)
            for (uint32_t k = 0; k < p.K; k++) std::printf("%zu\n", mel_filter_index(p, m, k));
        return 0;
    }
    if (cmd == "run" && argc == 15) {
        std::vector<float> w, f;
        zflac_mel_desc d = good_desc((uint32_t)u64(argv[11]), (uint32_t)u64(argv[12]), (uint32_t)u64(argv[13]), w, f);
        d.dtype = (uint8_t)u64(argv[14]);
        MelPlan p;
        int out = 0;
        if (mel_plan_create(&d, &out, p)) return 2;
        MelGrid g;
        const int rc = mel_plan_run(u64(argv[2]) ? &p : nullptr, (uintptr_t)u64(argv[3]), u64(argv[4]), u64(argv[5]),
                                    u64(argv[6]), u64(argv[7]), u64(argv[8]), (uintptr_t)u64(argv[9]), (size_t)u64(argv[10]), g);
        std::printf("%d %u %llu\n", rc, g.tiles, (unsigned long long)g.blocks);
        return 0;
    }
    if (cmd == "frames" && argc == 6) {
        std::printf("%llu\n", (unsigned long long)mel_frames(u64(argv[2]), (uint32_t)u64(argv[3]), (uint32_t)u64(argv[4]),
                                                             (int)u64(argv[5])));
        return 0;
    }
    if (cmd == "layout") {
        std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(zflac_mel_desc),
                    offsetof(zflac_mel_desc, size), offsetof(zflac_mel_desc, dtype), offsetof(zflac_mel_desc, layout),
                    offsetof(zflac_mel_desc, scale), offsetof(zflac_mel_desc, center), offsetof(zflac_mel_desc, n_fft),
                    offsetof(zflac_mel_desc, hop), offsetof(zflac_mel_desc, n_bins), offsetof(zflac_mel_desc, reserved),
                    offsetof(zflac_mel_desc, floor), offsetof(zflac_mel_desc, window), offsetof(zflac_mel_desc, filters));
        return 0;
    }
    std::fprintf(stderr, "mel_probe: unknown case\n");
    return 64;
}
