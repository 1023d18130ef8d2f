// limiter_host.hpp -- the float64 host half of dsp_limiter (dspbench.h): spec
// validation, link groups, the release coefficient, the attack window, the
// device table and the scratch size.  No HIP here: plain C++
// (limiter_host.cpp), like loudness_host.cpp.
#pragma once
#include <cstdint>
#include <vector>

#include "dspbench/dspbench.h"

namespace dspb {

constexpr uint32_t kLimTile = 2048;          // samples per tile (limiter.hip)
constexpr uint32_t kLimLane = 8;             // consecutive samples a thread scans serially
constexpr uint32_t kLimMaxLookahead = 1024;  // A
constexpr double kLimMaxRelease = 4194304.0; // tau: 2^22 samples
constexpr uint32_t kLimGroup = 16;           // rows per launch (kMaxChannels)

// the device table (limiter.hip), every entry float64 rounded once to float,
// rho the float of the plan taken back to float64:
//   [0, 9)    rho^k, k = 0..8           (a sample inside its lane's run)
//   [16, 80)  rho^(8 l), l = 0..63      (a lane inside its wave)
//   [80]      rho^512                   (a wave inside its tile)
//   [81]      rho^2048                  (a tile)
//   [96, 96 + wpad)  w[0..A], then zeros up to a multiple of 8
constexpr uint32_t kLimTabLane = 16, kLimTabWave = 80, kLimTabTile = 81, kLimTabWindow = 96;

struct LimiterPlan {
    uint32_t groups = 0;      // link groups: 1, or C with DSP_LIMITER_UNLINKED
    uint32_t oversample = 1;  // the detector's: 4 / 2 / 1 with DSP_LIMITER_TRUE_PEAK, else 1
    float rho = 0.f;          // (float)exp(-1 / tau); 0 for tau = 0
    uint32_t lookahead = 0;   // A
    uint32_t wpad = 0;        // (A + 1) rounded up to a multiple of 8
    uint64_t tiles = 0;       // ceil(L / kLimTile)
    uint32_t rows = 0;        // scratch rows of h: min(groups, 16)
    uint32_t chunks = 0;      // launches of pass 1 per linked group: ceil(C / 16)
    uint64_t scratch_bytes = 0;
};

// dsp_limiter_plan's body without the oversampler's own checks (the caller
// runs resample_plan for TRUE_PEAK).  Returns 0, 1 (invalid) or 2
// (unsupported) with *why set.
int limiter_plan(uint32_t sr, uint64_t L, uint32_t C, const dsp_limiter_spec *spec, LimiterPlan *plan,
                 const char **why);
// w[0..A]
void limiter_window(uint32_t A, float *w);
// the device table above
void limiter_table(const LimiterPlan &p, std::vector<float> &h);
// The scratch of a call: [rows][tiles 2048] h, [tiles 2048] p when a linked
// group takes more than one launch of pass 1, [rows][tiles] E, [rows][tiles]
// carry, 4 result words.  0 when it does not fit 64 bits.
uint64_t limiter_scratch_bytes(uint64_t tiles, uint32_t rows, uint32_t chunks);

}  // namespace dspb
