// host_tables_check.cpp -- stand-alone check of csrc/host_tables.cpp (no HIP):
// prints one "name value" line per figure for tests/test_host_tables.py.
// Every expected value here comes from the definition of what the table holds,
// not from the code under test.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "host_tables.hpp"

using namespace dspb;

// max |taps_spectrum - direct O(n^2) DFT| in float64, and the DFT's peak
static void check_spectrum() {
    const int n = 64;
    const uint32_t T = 23;  // zero-padded to n
    std::vector<float> taps(T);
    for (uint32_t i = 0; i < T; ++i) taps[i] = (float)std::sin(0.37 * i * i + 0.2) * (1.0f - 0.03f * i);
    std::vector<double> re, im;
    taps_spectrum(taps.data(), T, n, re, im);
    double err = 0.0, peak = 0.0;
    for (int k = 0; k < n; ++k) {
        double sr = 0.0, si = 0.0;
        for (uint32_t i = 0; i < T; ++i) {
            const double a = -2.0 * M_PI * (double)((k * i) % n) / n;
            sr += taps[i] * std::cos(a);
            si += taps[i] * std::sin(a);
        }
        err = std::max({err, std::fabs(sr - re[k]), std::fabs(si - im[k])});
        peak = std::max(peak, std::hypot(sr, si));
    }
    std::printf("spectrum_max_diff %.17g\nspectrum_peak %.17g\n", err, peak);
}

// One section with poles r e^(+-i th): the zero-input state (y1, y2) advances
// by A = [[-a1, -a2], [1, 0]] per sample, and A^m = [[u(m+1), -a2 u(m)],
// [u(m), -a2 u(m-1)]] with u(m) = r^(m-1) sin(m th) / sin(th) (u(0) = 0, u(1) = 1:
// the recurrence's own fundamental solution).  The tables hold A^(T l) for
// l <= 64 and A^(64 T k) for k <= 256, rounded to float.
static void check_biquad(double r, double th, uint32_t T) {
    const float cf[5] = {1.0f, 0.5f, 0.25f, (float)(-2.0 * r * std::cos(th)), (float)(r * r)};
    std::vector<float> h;
    const uint32_t W = biquad_tables(cf, 1, T, h);
    const double a1 = cf[3], a2 = cf[4];          // the rounded coefficients define the filter
    const double rr = std::sqrt(a2), tt = std::acos(-a1 / (2.0 * rr));
    auto u = [&](double m) { return m == 0.0 ? 0.0 : std::pow(rr, m - 1.0) * std::sin(m * tt) / std::sin(tt); };
    // error of a block relative to its largest entry; a float this small is a
    // multiple of 2^-149, so that much is granted on top
    auto block_err = [&](const float *o, double m) {
        const double want[4] = {u(m + 1), -a2 * u(m), u(m), m == 0.0 ? 1.0 : -a2 * u(m - 1)};
        double big = 0.0, err = 0.0;
        for (int q = 0; q < 4; ++q) big = std::max(big, std::fabs(want[q]));
        for (int q = 0; q < 4; ++q) err = std::max(err, std::fabs((double)o[q] - want[q]) - std::ldexp(1.0, -149));
        return big > 0.0 ? std::max(err, 0.0) / big : (err > 0.0 ? 1.0 : 0.0);
    };
    double eq = 0.0, ep = 0.0;
    for (int l = 0; l <= 64; ++l) eq = std::max(eq, block_err(h.data() + 20 + 4 * l, (double)T * l));
    for (int k = 0; k <= 256; ++k) ep = std::max(ep, block_err(h.data() + 20 + 4 * 65 + 4 * k, 64.0 * T * k));
    bool coef = h.size() == 20 + (65 + 257) * 4;
    for (int q = 0; q < 20; ++q) coef = coef && h[q] == (q < 5 ? cf[q] : 0.0f);
    std::printf("biquad_coef_ok %d\nbiquad_Q_rel_err %.17g\nbiquad_P_rel_err %.17g\nbiquad_W %u\n", (int)coef, eq, ep,
                W);
}

int main() {
    check_spectrum();
    check_biquad(0.9, 0.3, 32);
    const struct { float g, s; uint32_t B; } ramps[] = {{0.9f, 0.002f, 512},   {1.0f, 0.25f, 512}, {0.3f, 0.001f, 4096},
                                                       {0.9f, 0.002f, 65536}, {1.0f, 0.25f, 65537}};
    for (const auto &p : ramps) std::printf("ramp %.9g %.9g %u %d\n", p.g, p.s, p.B, (int)ramp_closed_form(p.g, p.s, p.B));
    return 0;
}
