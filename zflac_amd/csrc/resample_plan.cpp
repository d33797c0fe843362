// resample_plan.cpp -- the resampler's host planning (resample_plan.h). Plain C++, no HIP.
#include "resample_plan.h"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace zflac {

namespace {

constexpr double PI = 3.14159265358979323846;

// modified Bessel function of the first kind, order 0: sum_j ((x/2)^j / j!)^2, to convergence
double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int j = 1; j < 1000; j++) {
        term *= q / ((double)j * (double)j);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

double sinc(double t) {
    if (t == 0.0) return 1.0;
    const double a = PI * t;
    return std::sin(a) / a;
}

}  // namespace

bool resample_params_ok(uint32_t zeros, double rolloff, double beta) {
    return zeros >= 1 && rolloff > 0.0 && rolloff <= 1.0 && beta >= 0.0 && std::isfinite(beta);
}

bool resample_ratio(uint32_t fin, uint32_t fout, uint32_t zeros, double rolloff, ResampleRatio& r) {
    if (!fin || !fout || fin > RESAMPLE_MAX_RATE || fout > RESAMPLE_MAX_RATE) return false;
    const uint32_t g = std::gcd(fin, fout);
    r.M = fin / g;
    r.L = fout / g;
    r.s = std::min(1.0, (double)r.L / (double)r.M) * rolloff;
    const double w = std::ceil((double)zeros / r.s);
    // (a tiny rolloff: far above any limit the caller checks K against, and within 32 bits)
    r.W = w < 1e9 ? (uint32_t)w : 1000000000u;
    r.K = 2 * (uint64_t)r.W + 1;
    return true;
}

uint64_t resampled_frames(uint64_t n_frames, uint32_t fin, uint32_t fout) {
    if (!fin || !fout) return 0;
    const uint32_t g = std::gcd(fin, fout);
    const uint64_t M = fin / g, L = fout / g;
    const unsigned __int128 n = ((unsigned __int128)n_frames * L + (M - 1)) / M;
    return n > (unsigned __int128)UINT64_MAX ? UINT64_MAX : (uint64_t)n;
}

void resample_taps(const ResampleRatio& r, uint32_t zeros, double beta, std::vector<float>& h) {
    const uint32_t K = (uint32_t)r.K;
    const double Z = (double)zeros, i0_beta = bessel_i0(beta);
    h.resize((size_t)r.L * K);
    std::vector<double> u(K);
    for (uint32_t p = 0; p < r.L; p++) {
        const double frac = (double)p / (double)r.L;
        double sum = 0;
        for (uint32_t k = 0; k < K; k++) {
            const double d = ((double)k - (double)r.W) - frac;
            const double t = r.s * d;
            double v = 0;
            if (std::fabs(t) < Z) {
                const double y = t / Z;
                v = r.s * sinc(t) * (bessel_i0(beta * std::sqrt(1.0 - y * y)) / i0_beta);
            }
            u[k] = v;
            sum += v;
        }
        for (uint32_t k = 0; k < K; k++) h[(size_t)p * K + k] = (float)(u[k] / sum);
    }
}

ResampleTile resample_tile(const ResampleRatio& r, uint32_t channels) {
    ResampleTile t;
    const uint64_t tab = (r.table_floats() + 3) & ~3ull;  // (the span starts 16-byte aligned behind it)
    // a frame's staged channels are one 4-, 8- or 16-byte LDS read: 1, 2 or 4 of them
    const uint32_t want = channels >= 3 ? RESAMPLE_MAX_CG : std::max(1u, channels);
    // the table in LDS when it fits its share and leaves one channel's K + 1 frames a place
    t.tab_lds = tab <= RESAMPLE_LDS_TABLE && r.K + 1 <= RESAMPLE_LDS_FLOATS - tab;
    const uint64_t span = RESAMPLE_LDS_FLOATS - (t.tab_lds ? tab : 0);
    uint32_t cg = want;
    while (cg > 1 && span / cg < r.K + 1) cg /= 2;
    t.cg = (uint8_t)cg;
    // ceil((n - 1) M / L) <= span / cg - K
    const uint64_t room = span / cg - r.K;
    const unsigned __int128 n = (unsigned __int128)room * r.L / r.M + 1;
    uint32_t tile = n > RESAMPLE_MAX_TILE ? RESAMPLE_MAX_TILE : (uint32_t)n;
    if (tile >= RESAMPLE_THREADS) tile -= tile % RESAMPLE_THREADS;  // no pass of the workgroup left part idle
    else if (tile >= 64) tile &= ~63u;
    t.tile = tile;
    return t;
}

}  // namespace zflac
