// plan_probe.cpp -- test shim (tests/test_stream_plan.py): runs the library's host planner on
// a stream, without a GPU. Built with plain g++ together with zflac_amd/csrc/stream_plan.cpp.
#include "stream_plan.h"

extern "C" {

struct plan_result {
    int host_err;   // error known without the GPU (0: none)
    int no_frames;  // empty frame section, total unknown: zero samples, no error
    int kind;       // 0 / 1 / 2: i8 / i16 / i32 container
    int nch;
    unsigned rate;  // the first frame's sample rate
    int bps;        // depth_bits of the first frame's depth code
};

void plan_probe(const unsigned char* data, size_t len, plan_result* out) {
    zflac::StreamPlan s;
    zflac::plan_stream(s, data, len);
    out->host_err = s.host_err;
    out->no_frames = s.no_frames ? 1 : 0;
    out->kind = s.kind;
    out->nch = s.nch;
    out->rate = s.first.rate;
    out->bps = zflac::depth_bits(s.first.dcode, (int)s.si.bps);
}

}  // extern "C"
