// sweep_host.hpp -- the excitation of a swept-sine measurement (dspbench.h
// dsp_sweep): the exponential sine sweep, its length and rate, and where each
// harmonic order's response lands after deconvolution.  Float64 on the host,
// rounded once.  No HIP here: plain C++ (sweep_host.cpp).
#pragma once
#include <cstdint>

#include "dspbench/dspbench.h"

namespace dspb {

constexpr uint64_t kSweepMaxLen = 1ull << 24;

struct SweepPlan {
    uint64_t L = 0;     // round(seconds sr)
    double rate = 0.0;  // ln(f2 / f1) / seconds
    double K = 0.0;     // 2 pi f1 / rate: the phase is K (e^{rate t} - 1)
};

// dsp_sweep_plan's body.  Returns 0, or 1 (invalid) with *why set.
int sweep_plan(uint32_t sr, const dsp_sweep_spec *spec, SweepPlan *plan, const char **why);
// out[0..count), count <= L: samples [0, count) of the sweep
void sweep_fill(uint32_t sr, const dsp_sweep_spec *spec, const SweepPlan &p, float *out, uint64_t count);
// samples by which order m's response precedes the linear one: ln(m) / rate sr
double sweep_harmonic_offset(uint32_t sr, const SweepPlan &p, uint32_t order);

}  // namespace dspb
