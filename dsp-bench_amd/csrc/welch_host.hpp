// welch_host.hpp -- the host half of dsp_welch (dspbench.h): the plan (frames,
// run, chunk, scratch layout, the window's sums) and dsp_welch_derive's float64
// arithmetic.  No HIP here: plain C++ (welch_host.cpp), like loudness_host.cpp
// and limiter_host.cpp.
#pragma once
#include <cstdint>

#include "dspbench/dspbench.h"
#include "host_tables.hpp"

namespace dspb {

constexpr uint32_t kWelchN = 8192;
constexpr uint32_t kWelchBins = kWelchN / 2 + 1;  // 4097
constexpr uint32_t kWelchRun = 16;                // frames summed in float32 before float64 takes over
constexpr uint32_t kWelchSpec4 = kConvSpec4;      // float4 per scratch spectrum (conv_fdl.hip's layout)
constexpr uint32_t kWelchGroup = 16;              // rows per channel group (kMaxChannels: capi_grid.cpp asserts it)
// the spectra a chunk may hold: chunk = the largest multiple of kWelchRun with
// rows chunk 33792 bytes <= this (rows = min(C, 16) + has_ref; at least one run)
constexpr uint64_t kWelchSpectraBytes = 64ull << 20;

struct WelchPlan {
    uint32_t H = 0;
    int32_t window = 0;
    uint64_t frames = 0;
    uint32_t rows = 0;      // min(C, 16) + has_ref
    uint32_t chunk = 0;     // frames per chunk, a multiple of kWelchRun
    uint32_t runs_cap = 0;  // chunk / kWelchRun
    // the scratch, in bytes from its start: [rows][chunk] spectra, then the
    // partial sums [min(C, 16)][runs_cap][2112] of |X|^2 (float2) and of
    // conj(R) X (float4), and [runs_cap][2112] of |R|^2 (float2)
    uint64_t off_pxx = 0, off_pxy = 0, off_prr = 0;
    uint64_t scratch_bytes = 0;
    double win_sum = 0.0, win_sumsq = 0.0;
};

// dsp_welch_plan's body: 0, 1 (invalid) or 2 (unsupported) with *why set
int welch_plan(uint64_t L, uint32_t C, int has_ref, const dsp_welch_spec *spec, WelchPlan *plan, const char **why);
// dsp_welch_derive's body (arguments checked by the caller)
void welch_derive(const double *const *sxx, const double *srr, const double *const *sxy, uint32_t C, uint32_t bins,
                  uint64_t frames, double sr, double win_sum, double win_sumsq, uint32_t flags, double *const *psd,
                  double *const *H1, double *const *coherence);

}  // namespace dspb
