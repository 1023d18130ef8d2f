// sweep_host.cpp -- dsp_sweep_plan / dsp_sweep / dsp_sweep_harmonic_offset
// (dspbench.h) in float64 on the host.  No HIP.
#include "sweep_host.hpp"

#include <cmath>

namespace dspb {

int sweep_plan(uint32_t sr, const dsp_sweep_spec *spec, SweepPlan *plan, const char **why) {
    const char *dummy;
    if (!why) why = &dummy;
    if (!spec) return *why = "dsp_sweep: the spec is NULL", 1;
    if (sr == 0) return *why = "dsp_sweep: needs a sample rate", 1;
    if (!(spec->f1 > 0.0) || !(spec->f1 < spec->f2) || !(spec->f2 <= 0.5 * (double)sr))
        return *why = "dsp_sweep: needs 0 < f1 < f2 <= sr / 2", 1;
    if (!std::isfinite(spec->amplitude)) return *why = "dsp_sweep: the amplitude must be finite", 1;
    if (!(spec->seconds > 0.0) || !std::isfinite(spec->seconds)) return *why = "dsp_sweep: needs seconds > 0", 1;
    const double len = std::floor(spec->seconds * (double)sr + 0.5);
    if (!(len >= 1.0)) return *why = "dsp_sweep: shorter than one sample", 1;
    if (len > (double)kSweepMaxLen) return *why = "dsp_sweep: more than 2^24 samples", 1;
    SweepPlan p;
    p.L = (uint64_t)len;
    if (2ull * spec->fade > p.L) return *why = "dsp_sweep: the two fades are longer than the sweep", 1;
    p.rate = std::log(spec->f2 / spec->f1) / spec->seconds;
    p.K = 2.0 * M_PI * spec->f1 * spec->seconds / std::log(spec->f2 / spec->f1);
    if (plan) *plan = p;
    return 0;
}

void sweep_fill(uint32_t sr, const dsp_sweep_spec *spec, const SweepPlan &p, float *out, uint64_t count) {
    const double R = std::log(spec->f2 / spec->f1);
    const uint32_t fade = spec->fade;
    for (uint64_t i = 0; i < count && i < p.L; ++i) {
        double x = spec->amplitude * std::sin(p.K * std::expm1((double)i / (double)sr * R / spec->seconds));
        // a raised cosine over `fade` samples at each end (half-sample centred: never 0 or 1)
        if (i < fade) x *= 0.5 - 0.5 * std::cos(M_PI * ((double)i + 0.5) / (double)fade);
        if (i >= p.L - fade) x *= 0.5 - 0.5 * std::cos(M_PI * ((double)(p.L - 1 - i) + 0.5) / (double)fade);
        out[i] = (float)x;
    }
}

double sweep_harmonic_offset(uint32_t sr, const SweepPlan &p, uint32_t order) {
    return std::log((double)order) / p.rate * (double)sr;
}

}  // namespace dspb
