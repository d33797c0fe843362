// export_plan_probe.cpp -- test shim (tests/test_export_plan.py): the dense exports' planning
// (verdict, shape, grid, coefficient table, ratios) and the row records it writes, without a GPU.
// Built with plain g++ together with zflac_amd/csrc/export_plan.cpp and resample_plan.cpp.
#include "export_plan.h"

extern "C" {

constexpr unsigned EXPORT_PROBE_NEEDS = 8;

struct export_probe_stream {  // zflac::ExportStream, field by field
    unsigned long long samples, n_frames;
    unsigned rate;
    unsigned char nch, kind;
};

struct export_probe_plan {
    unsigned long long C, T, tiles, need_floats;
    unsigned vec, mixed, table_len, n_needs;
    unsigned short at[zflac::MIX_MAX_CH + 1];
    float table[zflac::MIX_TABLE_FLOATS];
    unsigned need_fin[EXPORT_PROBE_NEEDS], need_L[EXPORT_PROBE_NEEDS], need_M[EXPORT_PROBE_NEEDS];
    unsigned need_W[EXPORT_PROBE_NEEDS], need_K[EXPORT_PROBE_NEEDS];
};

// Plans the call of `pd` (plain) or `rd` (resampled), whichever is not NULL, over s[n]; returns the
// verdict. With E_OK: *out is the plan, ratio_of[n] and n_out[n] (resampled call; may be NULL) its
// per-row vectors, and rows (may be NULL) receives the n records, ExportRow or ResampleRow, with
// taps_base + k * taps_step as the device table of ratio k.
int export_probe(const export_probe_stream* s, size_t n, const zflac_export_desc* pd, const zflac_resample_desc* rd,
                 const zflac_mix_desc* mix, unsigned long long dst, unsigned long long dst_bytes,
                 unsigned long long* valid_frames, export_probe_plan* out, int* ratio_of, unsigned long long* n_out,
                 void* rows, unsigned long long taps_base, unsigned long long taps_step) {
    std::vector<zflac::ExportStream> v(n);
    for (size_t i = 0; i < n; i++) {
        v[i].samples = reinterpret_cast<const void*>((uintptr_t)s[i].samples);
        v[i].n_frames = s[i].n_frames;
        v[i].rate = s[i].rate;
        v[i].nch = s[i].nch;
        v[i].kind = s[i].kind;
    }
    zflac::ExportPlan p;
    const int rc = zflac::plan_export(v.data(), n, rd ? zflac::export_call(rd) : zflac::export_call(pd), mix,
                                      (uintptr_t)dst, (size_t)dst_bytes, reinterpret_cast<uint64_t*>(valid_frames), p);
    if (rc) return rc;
    *out = export_probe_plan{};
    out->C = p.C;
    out->T = p.T;
    out->tiles = p.tiles;
    out->need_floats = p.need_floats;
    out->vec = p.vec;
    out->mixed = p.mixed;
    out->table_len = (unsigned)p.table.size();
    out->n_needs = (unsigned)p.needs.size();
    if (p.table.size() > zflac::MIX_TABLE_FLOATS || p.needs.size() > EXPORT_PROBE_NEEDS) return -1;
    for (unsigned i = 0; i <= zflac::MIX_MAX_CH; i++) out->at[i] = p.at[i];
    for (size_t i = 0; i < p.table.size(); i++) out->table[i] = p.table[i];
    std::vector<const float*> taps;
    for (size_t k = 0; k < p.needs.size(); k++) {
        out->need_fin[k] = p.needs[k].fin;
        out->need_L[k] = p.needs[k].ratio.L;
        out->need_M[k] = p.needs[k].ratio.M;
        out->need_W[k] = p.needs[k].ratio.W;
        out->need_K[k] = (unsigned)p.needs[k].ratio.K;
        taps.push_back(reinterpret_cast<const float*>((uintptr_t)(taps_base + k * taps_step)));
    }
    for (size_t i = 0; rd && i < n; i++) {
        if (ratio_of) ratio_of[i] = p.ratio_of[i];
        if (n_out) n_out[i] = p.n_out[i];
    }
    if (rows && rd) zflac::write_resample_rows(p, v.data(), taps.data(), static_cast<zflac::ResampleRow*>(rows));
    if (rows && !rd) zflac::write_export_rows(p, v.data(), static_cast<zflac::ExportRow*>(rows));
    return rc;
}

}  // extern "C"
