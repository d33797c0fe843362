// tests/c/row_mask_probe.cpp -- the frame-mask to lane-mask function of the staged write-back
// (zflac::row_lane_mask, csrc/decode/row_mask.h: the function the kernels run), on the host.
// Reads lines "<mono 0|1> <row 0..3> <frame mask, hex>" and prints one lane mask (hex) per line.
// A program of its own, so that tests/test_row_mask.py can build it with the host sanitizers.
#include <cinttypes>
#include <cstdio>

#include "decode/row_mask.h"

// the same function in constant expressions
static_assert(zflac::double_bits(0x80000001u) == 0xC000000000000003ull);
static_assert(zflac::row_lane_mask<false>(0x00000100ull, 1) == 0x00000000000000FFull);
static_assert(zflac::row_lane_mask<false>(0x80000000ull, 3) == 0xFF00000000000000ull);
static_assert(zflac::row_lane_mask<true>(0x8000000000000000ull, 3) == 0xF000000000000000ull);
static_assert(zflac::row_lane_mask<true>(0x0000000000010000ull, 1) == 0x000000000000000Full);

int main() {
    int mono, row;
    uint64_t frames;
    while (std::scanf("%d %d %" SCNx64, &mono, &row, &frames) == 3) {
        if (row < 0 || row > 3) return 2;
        const uint64_t m = mono ? zflac::row_lane_mask<true>(frames, row) : zflac::row_lane_mask<false>(frames, row);
        std::printf("%016" PRIx64 "\n", m);
    }
    return 0;
}
