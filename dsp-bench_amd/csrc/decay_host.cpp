// decay_host.cpp -- see decay_host.hpp.
#include "decay_host.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace dspb {

uint32_t decay_hop(uint32_t sr) {
    if (sr == 0 || sr % 100 != 0) return 0;
    const uint32_t ten = sr / 100;
    for (uint32_t h = sr / 1000; h >= 1; --h)
        if (ten % h == 0) return h;
    return 0;
}

int decay_plan(uint64_t L, uint32_t C, uint32_t sr, const dsp_decay_spec *spec, DecayPlan *p, const char **why) {
    *p = DecayPlan{};
    const dsp_decay_spec def{1u, -5, 4};
    if (!spec) spec = &def;
    if (C == 0 || L == 0) { *why = "dsp_decay: needs C >= 1 and L >= 1"; return 1; }
    if (spec->fraction != 1 && spec->fraction != 3) { *why = "dsp_decay: fraction must be 1 or 3"; return 1; }
    if (spec->k_hi < spec->k_lo || (int64_t)spec->k_hi - spec->k_lo + 1 > (int64_t)kDecayMaxBands ||
        spec->k_lo < -64 || spec->k_hi > 64) {
        *why = "dsp_decay: needs k_lo <= k_hi, at most 32 bands, indices within +-64";
        return 1;
    }
    if (sr == 0) { *why = "dsp_decay: sr is 0"; return 1; }
    p->hop = decay_hop(sr);
    if (!p->hop) { *why = "dsp_decay: the rate must be a multiple of 100 Hz"; return 2; }
    const double b = (double)spec->fraction, G = std::pow(10.0, 0.3), edge = std::pow(G, 1.0 / (2.0 * b));
    p->fraction = spec->fraction, p->k_lo = spec->k_lo, p->k_hi = spec->k_hi;
    p->bands = (uint32_t)(spec->k_hi - spec->k_lo + 1);
    for (uint32_t i = 0; i < p->bands; ++i) p->fm[i] = 1000.0 * std::pow(G, (double)(spec->k_lo + (int32_t)i) / b);
    if (p->fm[p->bands - 1] * edge > 0.5 * (double)sr) {
        *why = "dsp_decay: a band's upper edge lies above sr / 2";
        return 1;
    }
    p->Qr = 1.0 / (edge - 1.0 / edge);
    p->Qd = (M_PI / 6.0) / std::sin(M_PI / 6.0) * p->Qr;
    const double pad = std::ceil(8.0 * (double)sr * p->Qr / p->fm[0]);
    if (!(pad + (double)L <= (double)(1u << 24))) { *why = "dsp_decay: n = pow2(L + P) exceeds 2^24"; return 2; }
    p->P = (uint32_t)pad;
    uint64_t n = 1024;
    while (n < L + p->P) n <<= 1;
    p->n = (uint32_t)n;
    p->hops = (L + p->hop - 1) / p->hop + 1;
    p->Lp = (L + 1) & ~1ull;
    const uint64_t spec_bytes = 4ull * n + 8;
    const uint64_t row_bytes = 8ull * n + 2 * spec_bytes + 4 * p->Lp;
    p->rows = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(kDecayRowsBytes / row_bytes, 1), kDecayGroup);
    p->off_x = (uint64_t)p->rows * 8ull * n;
    p->off_y = p->off_x + p->rows * spec_bytes;
    p->off_ir = p->off_y + p->rows * spec_bytes;
    p->off_pre = p->off_ir + p->rows * 4 * p->Lp;
    p->scratch_bytes = p->off_pre + (uint64_t)p->rows * 2 * 8 * p->hops;
    return 0;
}

namespace {

// the least-squares line of lev against t over [a, b]: T = -60 / slope (NaN below 3 points or a flat line)
double fit_time(const std::vector<double> &lev, double dt, uint64_t a, uint64_t b) {
    if (b < a + 2) return std::nan("");
    const double m = (double)(b - a + 1);
    double st = 0.0, sl = 0.0;
    for (uint64_t k = a; k <= b; ++k) st += (double)k * dt, sl += lev[k];
    const double mt = st / m, ml = sl / m;
    double num = 0.0, den = 0.0;
    for (uint64_t k = a; k <= b; ++k) {
        const double d = (double)k * dt - mt;
        num += d * (lev[k] - ml), den += d * d;
    }
    const double slope = num / den;
    return slope < 0.0 ? -60.0 / slope : std::nan("");
}

}  // namespace

void decay_derive(const double *e, const double *mo, uint64_t F, uint32_t hop, uint32_t sr, dsp_decay_result *r) {
    const double nan = std::nan("");
    *r = dsp_decay_result{nan, nan, nan, nan, nan, nan, nan, nan, 0u, 0u, {0u, 0u}};
    const uint64_t W = (sr / 100) / hop;
    double total = 0.0;
    for (uint64_t j = 0; j < F; ++j) total += e[j];
    if (!(total > 0.0)) r->flags |= DSP_DECAY_SILENT;
    if (F < W || F == 0) r->flags |= DSP_DECAY_SHORT;
    if (r->flags) {
        r->flags |= DSP_DECAY_EDT_INVALID | DSP_DECAY_T20_INVALID | DSP_DECAY_T30_INVALID;
        return;
    }
    // the noise: the mean of the last tenth of the full hops
    const uint64_t tail = std::max<uint64_t>(1, F / 10), tail0 = F - tail;
    double N = 0.0;
    for (uint64_t j = tail0; j < F; ++j) N += e[j];
    N /= (double)tail;
    // the 10 ms window means, their first maximum, and the truncation
    const uint64_t nw = F - W + 1;
    std::vector<double> win(nw);
    {
        std::vector<double> cum(F + 1, 0.0);
        for (uint64_t j = 0; j < F; ++j) cum[j + 1] = cum[j] + e[j];
        for (uint64_t k = 0; k < nw; ++k) win[k] = (cum[k + W] - cum[k]) / (double)W;
    }
    uint64_t kmax = 0;
    for (uint64_t k = 1; k < nw; ++k)
        if (win[k] > win[kmax]) kmax = k;
    r->inr = N > 0.0 ? 10.0 * std::log10(win[kmax] / N) : std::numeric_limits<double>::infinity();
    uint64_t kt = tail0;
    const double floor2 = std::pow(10.0, 0.3) * N;
    for (uint64_t k = kmax; k < nw; ++k)
        if (win[k] <= floor2) { kt = k; break; }
    r->truncation = (uint32_t)std::min<uint64_t>(kt, 0xFFFFFFFFu);
    // Schroeder: EDC_k = sum_{j = k}^{kt - 1} e_j, from the end
    std::vector<double> lev(kt);
    {
        double s = 0.0;
        for (uint64_t k = kt; k-- > 0;) s += e[k], lev[k] = s;
        const double e0 = kt ? lev[0] : 0.0;
        for (uint64_t k = 0; k < kt; ++k) lev[k] = lev[k] > 0.0 ? 10.0 * std::log10(lev[k] / e0) : -HUGE_VAL;
    }
    const double dt = (double)hop / (double)sr;
    struct { double hi, lo, inr; double *out; uint32_t flag; } fits[3] = {
        {0.0, -10.0, 20.0, &r->edt, DSP_DECAY_EDT_INVALID},
        {-5.0, -25.0, 35.0, &r->t20, DSP_DECAY_T20_INVALID},
        {-5.0, -35.0, 45.0, &r->t30, DSP_DECAY_T30_INVALID},
    };
    for (auto &f : fits) {
        double T = nan;
        if (r->inr >= f.inr && kt >= 3) {
            uint64_t a = 0, b = 0;
            bool have = false;
            while (a < kt && !(lev[a] <= f.hi)) ++a;
            for (uint64_t k = a; k < kt; ++k)
                if (lev[k] >= f.lo) b = k, have = true;
            if (have && a < kt) T = fit_time(lev, dt, a, b);
        }
        *f.out = T;
        if (std::isnan(T)) r->flags |= f.flag;
    }
    // clarity, definition and the centre time up to the truncation
    auto sum = [&](const double *v, uint64_t a, uint64_t b) {
        double s = 0.0;
        for (uint64_t j = a; j < b; ++j) s += v[j];
        return s;
    };
    const uint64_t k50 = (uint64_t)sr / 20 / hop, k80 = (uint64_t)sr * 2 / 25 / hop;
    const double early50 = sum(e, 0, std::min(k50, F)), late50 = sum(e, std::min(k50, kt), kt);
    const double early80 = sum(e, 0, std::min(k80, F)), late80 = sum(e, std::min(k80, kt), kt);
    r->c50 = 10.0 * std::log10(early50 / late50);
    r->c80 = 10.0 * std::log10(early80 / late80);
    r->d50 = early50 / (early50 + late50);
    if (mo) r->ts = sum(mo, 0, kt) / sum(e, 0, kt) / (double)sr;
}

}  // namespace dspb
