// mel_run_probe.cpp -- tests/test_mel_run_plan.py's view of mel_plan_run_ex (zflac_amd/csrc/
// mel_plan.cpp): a program of its own (plain g++, no HIP; also built with
// -fsanitize=address,undefined) that takes one case on its command line and prints what the
// planner answers.
//
//   run_ex KEY=VALUE ...
//       a plan of n, hop, bins, dtype, scale, center (plan=0: no plan) and a descriptor of size
//       (-1 = sizeof(zflac_mel_run_desc)), pad, norm, reserved, wave, rows, wave_frames,
//       row_stride, lengths, first, frames, dst, dst_bytes, row_max, range, add, mul, reserved2
//       (desc=0: a NULL descriptor). Keys not given keep the defaults below.
//       prints: rc tiles blocks, then mel_plan_run's rc tiles blocks for the shared arguments,
//       then mel_run_is_plain (1: the descriptor is zflac_hip_mel_run's call)
//   short SIZE
//       a descriptor of only SIZE bytes (4 <= SIZE < 104) on the heap, size = SIZE. prints: rc tiles blocks
//   layout
//       prints sizeof(zflac_mel_run_desc) and the offset of every field
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "mel_plan.h"

using namespace zflac;

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "run_ex") {
        std::map<std::string, std::string> kv = {
            {"plan", "1"}, {"desc", "1"}, {"n", "400"}, {"hop", "160"}, {"bins", "80"}, {"dtype", "0"}, {"scale", "1"},
            {"center", "1"}, {"size", "-1"}, {"pad", "0"}, {"norm", "0"}, {"reserved", "0"}, {"wave", "0x7F4200000000"},
            {"rows", "5"}, {"wave_frames", "1000"}, {"row_stride", "1000"}, {"lengths", "0"}, {"first", "0"},
            {"frames", "7"}, {"dst", "0x7F5200000000"}, {"dst_bytes", "0xFFFFFFFFFFFF"}, {"row_max", "0"},
            {"range", "0"}, {"add", "0"}, {"mul", "0"}, {"reserved2", "0"}};
        for (int i = 2; i < argc; i++) {
            const char* eq = std::strchr(argv[i], '=');
            const std::string key = eq ? std::string(argv[i], (size_t)(eq - argv[i])) : std::string();
            if (!eq || !kv.count(key)) {
                std::fprintf(stderr, "mel_run_probe: unknown key in %s\n", argv[i]);
                return 64;
            }
            kv[key] = eq + 1;
        }
        auto u = [&](const char* k) { return std::strtoull(kv[k].c_str(), nullptr, 0); };
        auto f = [&](const char* k) { return std::strtof(kv[k].c_str(), nullptr); };
        const uint32_t n = (uint32_t)u("n"), bins = (uint32_t)u("bins");
        std::vector<float> w(n, 0.5f), filt((size_t)bins * (n / 2 + 1), 0.25f);
        zflac_mel_desc d;
        std::memset(&d, 0, sizeof d);
        d.size = sizeof d;
        d.dtype = (uint8_t)u("dtype");
        d.scale = (uint8_t)u("scale");
        d.center = (uint8_t)u("center");
        d.n_fft = (uint16_t)n;
        d.hop = (uint16_t)u("hop");
        d.n_bins = (uint16_t)bins;
        d.floor = d.scale == ZFLAC_MEL_POWER ? 0.0f : 1e-10f;
        d.window = w.data();
        d.filters = filt.data();
        MelPlan p;
        int out = 0;
        if (mel_plan_create(&d, &out, p)) return 2;
        zflac_mel_run_desc r;
        std::memset(&r, 0, sizeof r);
        const long size = std::strtol(kv["size"].c_str(), nullptr, 0);
        r.size = size < 0 ? (uint32_t)sizeof r : (uint32_t)size;
        r.pad = (uint8_t)u("pad");
        r.norm = (uint8_t)u("norm");
        r.reserved = (uint16_t)u("reserved");
        r.wave_device = reinterpret_cast<const float*>((uintptr_t)u("wave"));
        r.rows = u("rows");
        r.wave_frames = u("wave_frames");
        r.row_stride = u("row_stride");
        r.lengths_device = reinterpret_cast<const uint64_t*>((uintptr_t)u("lengths"));
        r.first_frame = u("first");
        r.frames = u("frames");
        r.dst_device = reinterpret_cast<void*>((uintptr_t)u("dst"));
        r.dst_bytes = (size_t)u("dst_bytes");
        r.row_max_device = reinterpret_cast<float*>((uintptr_t)u("row_max"));
        r.range = f("range");
        r.add = f("add");
        r.mul = f("mul");
        r.reserved2 = (uint32_t)u("reserved2");
        MelGrid g, g0;
        const MelPlan* pp = u("plan") ? &p : nullptr;
        const int rc = mel_plan_run_ex(pp, u("desc") ? &r : nullptr, g);
        const int rc0 = mel_plan_run(pp, (uintptr_t)u("wave"), r.rows, r.wave_frames, r.row_stride, r.first_frame, r.frames,
                                     (uintptr_t)u("dst"), r.dst_bytes, g0);
        std::printf("%d %u %llu %d %u %llu %d\n", rc, g.tiles, (unsigned long long)g.blocks, rc0, g0.tiles,
                    (unsigned long long)g0.blocks, (int)mel_run_is_plain(r));
        return 0;
    }
    if (cmd == "short" && argc == 3) {
        // a caller's older, shorter descriptor: SIZE bytes on the heap, size = SIZE. The size check
        // comes before any other field is read (the sanitized build would report the read).
        const size_t size = (size_t)std::strtoull(argv[2], nullptr, 0);
        if (size < sizeof(uint32_t) || size >= sizeof(zflac_mel_run_desc)) return 64;
        std::vector<float> w(2, 0.5f), filt(2, 0.25f);
        zflac_mel_desc d;
        std::memset(&d, 0, sizeof d);
        d.size = sizeof d;
        d.n_fft = 2;
        d.hop = 1;
        d.n_bins = 1;
        d.window = w.data();
        d.filters = filt.data();
        MelPlan p;
        int out = 0;
        if (mel_plan_create(&d, &out, p)) return 2;
        void* raw = std::malloc(size);
        if (!raw) return 2;
        std::memset(raw, 0, size);
        const uint32_t s32 = (uint32_t)size;
        std::memcpy(raw, &s32, sizeof s32);
        MelGrid g;
        const int rc = mel_plan_run_ex(&p, static_cast<const zflac_mel_run_desc*>(raw), g);
        std::free(raw);
        std::printf("%d %u %llu\n", rc, g.tiles, (unsigned long long)g.blocks);
        return 0;
    }
    if (cmd == "layout") {
#define OFF(f) offsetof(zflac_mel_run_desc, f)
        const size_t v[] = {sizeof(zflac_mel_run_desc), OFF(size), OFF(pad), OFF(norm), OFF(reserved), OFF(wave_device),
                            OFF(rows), OFF(wave_frames), OFF(row_stride), OFF(lengths_device), OFF(first_frame), OFF(frames),
                            OFF(dst_device), OFF(dst_bytes), OFF(row_max_device), OFF(range), OFF(add), OFF(mul),
                            OFF(reserved2)};
#undef OFF
        for (size_t x : v) std::printf("%zu ", x);
        std::printf("\n");
        return 0;
    }
    std::fprintf(stderr, "mel_run_probe: unknown case\n");
    return 64;
}
