// crc16_probe.cpp -- test shim (tests/test_crc16_edges.py): hands out the constants k_crc16 is
// compiled with. Built with plain g++ against zflac_amd/csrc/crc16_math.h alone: that it compiles
// is the check that the header is free of HIP (and its static_asserts hold under a second compiler).
#include "crc16_math.h"

namespace {
constexpr zflac::Crc16Tabs TABS = zflac::make_crc16_tabs();
constexpr zflac::Crc16Pow POW = zflac::make_crc16_pow();
}  // namespace

extern "C" {

// t[k][v], k = 0..3, v = 0..255, row after row
void crc16_probe_tables(uint16_t* out) {
    for (int k = 0; k < 4; k++)
        for (int v = 0; v < 256; v++) out[k * 256 + v] = TABS.t[k][v];
}

// p[0..39]
void crc16_probe_pow(uint16_t* out) {
    for (int k = 0; k < 40; k++) out[k] = POW.p[k];
}

uint32_t crc16_probe_mulmod(uint32_t a, uint32_t b) { return zflac::crc16_mulmod(a, b); }

}  // extern "C"
