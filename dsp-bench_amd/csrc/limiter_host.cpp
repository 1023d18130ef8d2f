// limiter_host.cpp -- dsp_limiter_plan's body and the limiter's tables
// (dspbench.h) in float64 on the host.  No HIP.
#include "limiter_host.hpp"

#include <algorithm>
#include <cmath>

#include "loudness_host.hpp"

namespace dspb {

int limiter_plan(uint32_t sr, uint64_t L, uint32_t C, const dsp_limiter_spec *spec, LimiterPlan *plan,
                 const char **why) {
    const char *dummy;
    if (!why) why = &dummy;
    if (!spec) return *why = "dsp_limiter: the spec is NULL", 1;
    if (C == 0) return *why = "dsp_limiter: needs C >= 1", 1;
    if (!(spec->ceiling > 0.f) || !std::isfinite(spec->ceiling))
        return *why = "dsp_limiter: the ceiling must be finite and positive", 1;
    if (spec->lookahead > kLimMaxLookahead) return *why = "dsp_limiter: the lookahead must be 0..1024 samples", 1;
    if (!(spec->release == 0.0 || (spec->release >= 1.0 && spec->release <= kLimMaxRelease)))
        return *why = "dsp_limiter: the release must be 0 or 1..2^22 samples", 1;
    if (spec->flags & ~(DSP_LIMITER_UNLINKED | DSP_LIMITER_TRUE_PEAK)) return *why = "dsp_limiter: unknown flags", 1;
    LimiterPlan p;
    if (spec->flags & DSP_LIMITER_TRUE_PEAK) {
        LoudnessPlan lp;
        if (loudness_plan(sr, 0, &lp, why)) return 2;  // the rate: the meter's own range
        p.oversample = lp.oversample;
    }
    p.groups = (spec->flags & DSP_LIMITER_UNLINKED) ? C : 1u;
    p.rho = spec->release == 0.0 ? 0.f : (float)std::exp(-1.0 / spec->release);
    p.lookahead = spec->lookahead;
    p.wpad = (spec->lookahead + 1 + 7) & ~7u;
    p.tiles = L / kLimTile + (L % kLimTile ? 1 : 0);
    p.rows = std::min(p.groups, kLimGroup);
    p.chunks = p.groups == 1 ? C / kLimGroup + (C % kLimGroup ? 1 : 0) : 1u;
    p.scratch_bytes = limiter_scratch_bytes(p.tiles, p.rows, p.chunks);
    if (p.tiles && p.scratch_bytes == 0) return *why = "dsp_limiter: the scratch does not fit 64 bits", 2;
    if (plan) *plan = p;
    return 0;
}

void limiter_window(uint32_t A, float *w) {
    const double pi = 3.14159265358979323846;
    double sum = 0.0;
    for (uint32_t k = 0; k <= A; ++k) {
        const double s = std::sin(pi * (double)(k + 1) / (double)(A + 2));
        sum += s * s;
    }
    for (uint32_t k = 0; k <= A; ++k) {
        const double s = std::sin(pi * (double)(k + 1) / (double)(A + 2));
        w[k] = (float)(s * s / sum);
    }
}

void limiter_table(const LimiterPlan &p, std::vector<float> &h) {
    h.assign(kLimTabWindow + p.wpad, 0.f);
    const double rho = (double)p.rho;
    auto pw = [&](double n) { return n == 0.0 ? 1.f : (float)std::pow(rho, n); };
    for (uint32_t k = 0; k <= kLimLane; ++k) h[k] = pw((double)k);
    for (uint32_t l = 0; l < 64; ++l) h[kLimTabLane + l] = pw((double)(kLimLane * l));
    h[kLimTabWave] = pw(64.0 * kLimLane);
    h[kLimTabTile] = pw((double)kLimTile);
    limiter_window(p.lookahead, h.data() + kLimTabWindow);
}

uint64_t limiter_scratch_bytes(uint64_t tiles, uint32_t rows, uint32_t chunks) {
    if (tiles > (~0ull >> 16) / (4ull * kLimTile)) return 0;
    const uint64_t row = tiles * kLimTile * 4;
    return row * rows + (chunks > 1 ? row : 0) + 2ull * rows * tiles * 4 + 16;
}

}  // namespace dspb
