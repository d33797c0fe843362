// cepstra_probe.cpp -- tests/test_cepstra_plan.py's view of zflac_amd/csrc/cepstra_plan.cpp: a
// program of its own (plain g++, no HIP; also built with -fsanitize=address,undefined) that takes
// one case on its command line and prints what the planner answers. Floats that a rule is about
// go by their bits; device pointers are addresses that are never read.
//
//   create SIZE IN OUT LAYOUT ORDER NIN NOUT WINDOW R0 R1 R2 FLAGS
//       FLAGS: 1 d NULL, 2 out NULL, 4 matrix NULL, 8 a NaN in the matrix's last value,
//       16 an infinity just behind the matrix (not read). SIZE -1 = the struct's sizeof.
//       prints: rc in_dtype out_dtype layout has_matrix n_in n_out delta_order delta_window features
//   scales ORDER WINDOW
//       prints the taps of the order as f32 bits, one line; then the table offset of the order
//   project SIZE RESERVED SRC DST ROWS FRAMES FLAGS NIN NOUT IN OUT
//       FLAGS: 1 plan NULL, 2 r NULL, 4 a plan without a matrix. prints: rc tiles passes blocks
//   deltas SIZE RESERVED RESERVED2 SRC DST ROWS FRAMES VALID PAD_BITS FLAGS C DTYPE LAYOUT ORDER WINDOW
//       FLAGS: 1 plan NULL, 2 r NULL, 4 a plan without deltas. prints: rc tiles passes blocks
//   cmvn SIZE MODE DDOF RESERVED FEAT ROWS FRAMES VALID MEAN STD EPS_BITS PAD_BITS LAYOUT FLAGS NOUT DTYPE
//       FLAGS: 1 plan NULL, 2 c NULL. prints: rc passes
//   grid PASSES
//       prints cepstra_grid_blocks
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "cepstra_plan.h"

using namespace zflac;

static unsigned long long u64(const char* s) { return std::strtoull(s, nullptr, 0); }
static float bits(const char* s) {
    const uint32_t u = (uint32_t)u64(s);
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}
static uint32_t bits_of(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

// a checked plan for the run calls
static bool good_plan(CepstraPlan& p, uint32_t n_in, uint32_t n_out, uint32_t in_dt, uint32_t out_dt, uint32_t layout,
                      uint32_t order, uint32_t window, bool with_matrix, std::vector<float>& m) {
    m.assign((size_t)n_in * n_out, 0.5f);
    zflac_cepstra_desc d;
    std::memset(&d, 0, sizeof d);
    d.size = sizeof d;
    d.in_dtype = (uint8_t)in_dt;
    d.out_dtype = (uint8_t)out_dt;
    d.layout = (uint8_t)layout;
    d.delta_order = (uint8_t)order;
    d.n_in = (uint16_t)n_in;
    d.n_out = (uint16_t)n_out;
    d.delta_window = (uint8_t)window;
    d.matrix = with_matrix ? m.data() : nullptr;
    int out = 0;
    return cepstra_plan_create(&d, &out, p) == 0;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "create" && argc == 14) {
        const long size = std::strtol(argv[2], nullptr, 0);
        const uint32_t n_in = (uint32_t)u64(argv[7]), n_out = (uint32_t)u64(argv[8]);
        const unsigned flags = (unsigned)u64(argv[13]);
        std::vector<float> m((size_t)257 * 257 + 1, 0.25f);
        const bool sane = n_in >= 1 && n_in <= 256 && n_out >= 1 && n_out <= 256;
        if (flags & 8) m[sane ? (size_t)n_in * n_out - 1 : 0] = std::numeric_limits<float>::quiet_NaN();
        if (flags & 16) m[sane ? (size_t)n_in * n_out : m.size() - 1] = std::numeric_limits<float>::infinity();
        zflac_cepstra_desc d;
        std::memset(&d, 0, sizeof d);
        d.size = size < 0 ? (uint32_t)sizeof d : (uint32_t)size;
        d.in_dtype = (uint8_t)u64(argv[3]);
        d.out_dtype = (uint8_t)u64(argv[4]);
        d.layout = (uint8_t)u64(argv[5]);
        d.delta_order = (uint8_t)u64(argv[6]);
        d.n_in = (uint16_t)n_in;
        d.n_out = (uint16_t)n_out;
        d.delta_window = (uint8_t)u64(argv[9]);
        for (int i = 0; i < 3; i++) d.reserved[i] = (uint8_t)u64(argv[10 + i]);
        d.matrix = flags & 4 ? nullptr : m.data();
        CepstraPlan p;
        int out = 0;
        const int rc = cepstra_plan_create(flags & 1 ? nullptr : &d, flags & 2 ? nullptr : &out, p);
        std::printf("%d %u %u %u %d %u %u %u %u %u\n", rc, p.in_dtype, p.out_dtype, p.layout, p.has_matrix ? 1 : 0, p.n_in,
                    p.n_out, p.delta_order, p.delta_window, p.features());
        return 0;
    }
    if (cmd == "scales" && argc == 4) {
        const uint32_t order = (uint32_t)u64(argv[2]), window = (uint32_t)u64(argv[3]);
        const std::vector<float> table = cepstra_scale_table(order, window);
        const uint32_t off = cepstra_scale_offset(order, window);
        const std::vector<double> s = cepstra_delta_scales(order, window);
        if (order && table.size() != off + s.size()) return 3;
        for (size_t i = 0; i < s.size(); i++) {
            const float v = order ? table[off + i] : (float)s[i];
            if (v != (float)s[i]) return 4;  // the table holds each tap rounded once
            std::printf("%u ", bits_of(v));
        }
        std::printf("\n%u\n", off);
        return 0;
    }
    if (cmd == "project" && argc == 13) {
        const long size = std::strtol(argv[2], nullptr, 0);
        const unsigned flags = (unsigned)u64(argv[8]);
        CepstraPlan p;
        std::vector<float> m;
        const uint32_t n_in = (uint32_t)u64(argv[9]), n_out = (uint32_t)u64(argv[10]);
        const bool ok = flags & 4 ? good_plan(p, n_in, n_in, (uint32_t)u64(argv[12]), (uint32_t)u64(argv[12]), 0, 1, 2, false, m)
                                  : good_plan(p, n_in, n_out, (uint32_t)u64(argv[11]), (uint32_t)u64(argv[12]), 0, 0, 0, true, m);
        if (!ok) return 2;
        zflac_cepstra_project_desc r;
        std::memset(&r, 0, sizeof r);
        r.size = size < 0 ? (uint32_t)sizeof r : (uint32_t)size;
        r.reserved = (uint32_t)u64(argv[3]);
        r.src_device = reinterpret_cast<const void*>(uintptr_t(u64(argv[4])));
        r.dst_device = reinterpret_cast<void*>(uintptr_t(u64(argv[5])));
        r.rows = u64(argv[6]);
        r.frames = u64(argv[7]);
        CepstraGrid g;
        const int rc = cepstra_plan_project(flags & 1 ? nullptr : &p, flags & 2 ? nullptr : &r, g);
        std::printf("%d %llu %llu %u\n", rc, (unsigned long long)g.tiles, (unsigned long long)g.passes, g.blocks);
        return 0;
    }
    if (cmd == "deltas" && argc == 17) {
        const long size = std::strtol(argv[2], nullptr, 0);
        const unsigned flags = (unsigned)u64(argv[11]);
        CepstraPlan p;
        std::vector<float> m;
        const uint32_t C = (uint32_t)u64(argv[12]), dt = (uint32_t)u64(argv[13]), layout = (uint32_t)u64(argv[14]);
        const bool ok = flags & 4 ? good_plan(p, C, C, dt, dt, layout, 0, 0, true, m)
                                  : good_plan(p, C, C, dt, dt, layout, (uint32_t)u64(argv[15]), (uint32_t)u64(argv[16]), false, m);
        if (!ok) return 2;
        zflac_cepstra_delta_desc r;
        std::memset(&r, 0, sizeof r);
        r.size = size < 0 ? (uint32_t)sizeof r : (uint32_t)size;
        r.reserved = (uint32_t)u64(argv[3]);
        r.reserved2 = (uint32_t)u64(argv[4]);
        r.src_device = reinterpret_cast<const void*>(uintptr_t(u64(argv[5])));
        r.dst_device = reinterpret_cast<void*>(uintptr_t(u64(argv[6])));
        r.rows = u64(argv[7]);
        r.frames = u64(argv[8]);
        r.valid_device = reinterpret_cast<const uint64_t*>(uintptr_t(u64(argv[9])));
        r.pad_value = bits(argv[10]);
        CepstraGrid g;
        const int rc = cepstra_plan_deltas(flags & 1 ? nullptr : &p, flags & 2 ? nullptr : &r, g);
        std::printf("%d %llu %llu %u\n", rc, (unsigned long long)g.tiles, (unsigned long long)g.passes, g.blocks);
        return 0;
    }
    if (cmd == "cmvn" && argc == 18) {
        CepstraPlan p;
        std::vector<float> m;
        if (!good_plan(p, 7, (uint32_t)u64(argv[16]), ZFLAC_EXPORT_F32, (uint32_t)u64(argv[17]), (uint32_t)u64(argv[14]), 0, 0, true, m))
            return 2;
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
        const int rc = cepstra_plan_cmvn(flags & 1 ? nullptr : &p, flags & 2 ? nullptr : &c, passes);
        std::printf("%d %llu\n", rc, (unsigned long long)passes);
        return 0;
    }
    if (cmd == "grid" && argc == 3) {
        std::printf("%u\n", cepstra_grid_blocks(u64(argv[2])));
        return 0;
    }
    std::fprintf(stderr, "cepstra_probe: unknown case\n");
    return 64;
}
