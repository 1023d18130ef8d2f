// loudness_host.cpp -- dsp_loudness_plan and dsp_loudness_gate (dspbench.h) in
// float64 on the host.  No HIP.
#include "loudness_host.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

#include "host_tables.hpp"

namespace dspb {

void k_weighting(uint32_t sr, float out[10]) {
    const double pi = 3.14159265358979323846;
    {  // stage 1: the high shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / (double)sr);
        const double Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        out[0] = (float)((Vh + Vb * K / Q + K * K) / a0);
        out[1] = (float)(2.0 * (K * K - Vh) / a0);
        out[2] = (float)((Vh - Vb * K / Q + K * K) / a0);
        out[3] = (float)(2.0 * (K * K - 1.0) / a0);
        out[4] = (float)((1.0 - K / Q + K * K) / a0);
    }
    {  // stage 2: the high pass
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / (double)sr);
        const double a0 = 1.0 + K / Q + K * K;
        out[5] = 1.f;
        out[6] = -2.f;
        out[7] = 1.f;
        out[8] = (float)(2.0 * (K * K - 1.0) / a0);
        out[9] = (float)((1.0 - K / Q + K * K) / a0);
    }
}

int loudness_plan(uint32_t sr, uint64_t L, LoudnessPlan *plan, const char **why) {
    if (sr < kLoudMinRate || sr > kLoudMaxRate) {
        if (why) *why = "dsp_loudness: the rate must be 8000..384000";
        return 2;
    }
    LoudnessPlan p;
    p.hop = (sr + 5) / 10;
    p.hops = L / p.hop;
    p.oversample = sr < 88200 ? 4u : sr < 176400 ? 2u : 1u;
    k_weighting(sr, p.kcoef);
    std::vector<float> h;
    p.window = biquad_tables(p.kcoef, 2, kLoudTile / 64, h);
    if (p.window == 0) {  // (never in the range: 18 tiles at 192 kHz, 34 at 384 kHz, of biquad_tables' 192)
        if (why) *why = "dsp_loudness: the K-weighting cascade has no finite look-back window";
        return 2;
    }
    p.run = std::max<uint32_t>(32, 8 * p.window);
    p.tiles = L / kLoudTile + (L % kLoudTile ? 1 : 0);
    p.scratch_bytes = loudness_scratch_bytes(p.hops, p.tiles);
    if (plan) *plan = p;
    return 0;
}

void loudness_tables(const float kcoef[10], std::vector<float> &h) {
    constexpr int D = 4, T = (int)kLoudTile / 64;
    typedef std::vector<double> Mat;
    Mat M(D * D);
    for (int j = 0; j < D; ++j) {  // column j: the state after T zero inputs from unit state j
        double Y1[2], Y2[2], X1[2], X2[2];
        for (int k = 0; k < 2; ++k) Y1[k] = (2 * k == j) ? 1.0 : 0.0, Y2[k] = (2 * k + 1 == j) ? 1.0 : 0.0;
        X1[0] = X2[0] = 0.0;
        X1[1] = Y1[0], X2[1] = Y2[0];
        for (int n = 0; n < T; ++n) {
            double v = 0.0;
            for (int k = 0; k < 2; ++k) {
                const float *c = kcoef + 5 * k;
                const double y = (double)c[0] * v + (double)c[1] * X1[k] + (double)c[2] * X2[k] -
                                 (double)c[3] * Y1[k] - (double)c[4] * Y2[k];
                X2[k] = X1[k], X1[k] = v, Y2[k] = Y1[k], Y1[k] = y;
                v = y;
            }
        }
        for (int k = 0; k < 2; ++k) M[(2 * k) * D + j] = Y1[k], M[(2 * k + 1) * D + j] = Y2[k];
    }
    auto mul = [](const Mat &a, const Mat &b) {
        Mat r(D * D, 0.0);
        for (int i = 0; i < D; ++i)
            for (int k = 0; k < D; ++k)
                for (int j = 0; j < D; ++j) r[i * D + j] += a[i * D + k] * b[k * D + j];
        return r;
    };
    // T X T for T = identity but its last row (0, 0, 1, -1), rounded to float
    auto put = [](const Mat &x, float *o) {
        for (int i = 0; i < D; ++i) {
            const double *row = &x[i * D];
            double r[D];
            for (int j = 0; j < D; ++j) r[j] = i == 3 ? x[2 * D + j] - row[j] : row[j];
            o[i * D + 0] = (float)r[0];
            o[i * D + 1] = (float)r[1];
            o[i * D + 2] = (float)(r[2] + r[3]);
            o[i * D + 3] = (float)(-r[3]);
        }
    };
    h.assign(20 + (65 + 2) * (size_t)D * D, 0.f);
    for (int q = 0; q < 10; ++q) h[q] = kcoef[q];
    Mat P(D * D, 0.0);
    for (int i = 0; i < D; ++i) P[i * D + i] = 1.0;
    float *o = h.data() + 20;
    put(P, o + 65 * D * D);  // I
    for (int l = 0; l <= 64; ++l) {
        put(P, o + (size_t)l * D * D);
        if (l < 64) P = mul(M, P);
    }
    put(P, o + 66 * D * D);  // M^64: a tile
}

static double lufs(double w) { return w > 0.0 ? -0.691 + 10.0 * std::log10(w) : -HUGE_VAL; }

void loudness_gate(const double *const *z, uint32_t C, uint64_t hops, uint32_t hop, const float *weights,
                   dsp_loudness_result *res) {
    // e[j] = sum_c G_c z[c][j]
    std::vector<double> e(hops, 0.0);
    for (uint32_t c = 0; c < C; ++c) {
        const double g = weights ? (double)weights[c] : 1.0;
        for (uint64_t j = 0; j < hops; ++j) e[j] += g * z[c][j];
    }
    auto block_powers = [&](uint64_t len) {
        std::vector<double> w;
        if (hops < len) return w;
        w.resize(hops - len + 1);
        for (uint64_t i = 0; i < w.size(); ++i) {
            double s = 0.0;
            for (uint64_t k = 0; k < len; ++k) s += e[i + k];
            w[i] = s / ((double)len * (double)hop);
        }
        return w;
    };
    // the mean of the powers above `gate` (LUFS), and their count
    auto gated_mean = [](const std::vector<double> &w, double gate, uint64_t *count) {
        double s = 0.0;
        uint64_t n = 0;
        for (double v : w)
            if (lufs(v) > gate) s += v, ++n;
        *count = n;
        return n ? s / (double)n : 0.0;
    };

    const std::vector<double> wm = block_powers(4);
    res->blocks = wm.size();
    res->momentary_max = -HUGE_VAL;
    for (double v : wm) res->momentary_max = std::max(res->momentary_max, lufs(v));
    uint64_t n_abs = 0, n_rel = 0;
    const double mean_abs = gated_mean(wm, -70.0, &n_abs);
    double integrated = -HUGE_VAL;
    if (n_abs) {
        const double rel = std::max(-70.0, lufs(mean_abs) - 10.0);
        const double mean_rel = gated_mean(wm, rel, &n_rel);
        if (n_rel) integrated = lufs(mean_rel);
    }
    res->integrated = integrated;
    res->gated_blocks = n_rel;

    const std::vector<double> ws = block_powers(30);
    res->short_term_max = -HUGE_VAL;
    for (double v : ws) res->short_term_max = std::max(res->short_term_max, lufs(v));
    res->range = 0.0;
    uint64_t ns = 0;
    const double st_mean = gated_mean(ws, -70.0, &ns);
    if (ns) {
        const double rel = lufs(st_mean) - 20.0;
        std::vector<double> s;
        for (double v : ws) {
            const double l = lufs(v);
            if (l > -70.0 && l > rel) s.push_back(l);
        }
        if (!s.empty()) {
            std::sort(s.begin(), s.end());
            const size_t n = s.size();
            res->range = s[(size_t)((double)(n - 1) * 0.95 + 0.5)] - s[(size_t)((double)(n - 1) * 0.10 + 0.5)];
        }
    }
}

}  // namespace dspb
