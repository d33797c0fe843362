// resample_probe.cpp -- test shim (tests/test_resample_plan.py): the library's resampling plan
// (ratio, tap tables, lengths, tile rule) without a GPU. Built with plain g++ together with
// zflac_amd/csrc/resample_plan.cpp.
#include "resample_plan.h"

extern "C" {

struct resample_probe_ratio {
    unsigned L, M, W;
    unsigned long long K;
    unsigned long long table_floats;
    int params_ok;     // zeros, rolloff, beta in range
    int rates_ok;      // both rates in 1 .. RESAMPLE_MAX_RATE
    int k_over_limit;  // K > RESAMPLE_MAX_TAPS: the export refuses the stream
    int table_over_budget;  // this table alone exceeds RESAMPLE_MAX_TABLE_FLOATS
};

void resample_probe_ratio_of(unsigned fin, unsigned fout, unsigned zeros, double rolloff, double beta,
                             resample_probe_ratio* out) {
    zflac::ResampleRatio r;
    *out = resample_probe_ratio{};
    out->params_ok = zflac::resample_params_ok(zeros, rolloff, beta) ? 1 : 0;
    if (!out->params_ok) return;
    out->rates_ok = zflac::resample_ratio(fin, fout, zeros, rolloff, r) ? 1 : 0;
    if (!out->rates_ok) return;
    out->L = r.L;
    out->M = r.M;
    out->W = r.W;
    out->K = r.K;
    out->table_floats = r.table_floats();
    out->k_over_limit = r.K > zflac::RESAMPLE_MAX_TAPS;
    out->table_over_budget = r.table_floats() > zflac::RESAMPLE_MAX_TABLE_FLOATS;
}

// h[L][K] into out (cap floats); returns the floats written, 0 when the plan is refused
unsigned long long resample_probe_taps(unsigned fin, unsigned fout, unsigned zeros, double rolloff, double beta,
                                       float* out, unsigned long long cap) {
    zflac::ResampleRatio r;
    if (!zflac::resample_params_ok(zeros, rolloff, beta) || !zflac::resample_ratio(fin, fout, zeros, rolloff, r)) return 0;
    if (r.K > zflac::RESAMPLE_MAX_TAPS || r.table_floats() > cap) return 0;
    std::vector<float> h;
    zflac::resample_taps(r, zeros, beta, h);
    for (size_t i = 0; i < h.size(); i++) out[i] = h[i];
    return h.size();
}

unsigned long long resample_probe_frames(unsigned long long n, unsigned fin, unsigned fout) {
    return zflac::resampled_frames(n, fin, fout);
}

// the kernel's tile rule and the LDS budget it is sized for
void resample_probe_tile(unsigned fin, unsigned fout, unsigned zeros, double rolloff, unsigned channels,
                         unsigned* tile, unsigned* cg, unsigned* tab_lds, unsigned* lds_floats) {
    zflac::ResampleRatio r;
    *tile = *cg = *tab_lds = 0;
    *lds_floats = zflac::RESAMPLE_LDS_FLOATS;
    if (!zflac::resample_ratio(fin, fout, zeros, rolloff, r)) return;
    const zflac::ResampleTile t = zflac::resample_tile(r, channels);
    *tile = t.tile;
    *cg = t.cg;
    *tab_lds = t.tab_lds;
}

}  // extern "C"
