// loudness_host.hpp -- the float64 host half of dsp_loudness (dspbench.h):
// the plan (hop, K-weighting coefficients, look-back window, blocking) and the
// BS.1770-4 gating / EBU Tech 3342 range over hop energies.  No HIP here:
// plain C++ (loudness_host.cpp), like host_tables.cpp.
#pragma once
#include <cstdint>
#include <vector>

#include "dspbench/dspbench.h"

namespace dspb {

constexpr uint32_t kLoudMinRate = 8000, kLoudMaxRate = 384000;
constexpr uint32_t kLoudTile = 2048;      // samples per tile of the K-weighting scan (iir_scan.hpp)
constexpr uint32_t kLoudSlots = 4;        // hops a tile can touch (hop >= 800)
constexpr uint32_t kLoudGroup = 16;       // channels per group (kMaxChannels)

struct LoudnessPlan {
    uint32_t hop = 0;          // (sr + 5) / 10
    uint64_t hops = 0;         // L / hop
    uint32_t oversample = 0;   // 4, 2 or 1
    float kcoef[10] = {};      // two sections of {b0, b1, b2, a1, a2}
    uint32_t window = 0;       // dsp_biquad_plan's look-back of the cascade, in tiles (never 0 here)
    uint32_t run = 0;          // tiles a wave measures after `window` warm-up tiles
    uint64_t tiles = 0;        // ceil(L / kLoudTile)
    uint64_t scratch_bytes = 0;
};

// the cascade's coefficients for a rate, float64 rounded once to float
void k_weighting(uint32_t sr, float out[10]);
// dsp_loudness_plan's body: 0, or 2 (unsupported) with *why set
int loudness_plan(uint32_t sr, uint64_t L, LoudnessPlan *plan, const char **why);
// the layout of a group's scratch: [16 rows of hops doubles][32 peak words][16 rows of tiles x 4 floats]
inline uint64_t loudness_scratch_bytes(uint64_t hops, uint64_t tiles) {
    return kLoudGroup * hops * 8 + 2 * kLoudGroup * 4 + kLoudGroup * tiles * kLoudSlots * 4;
}
// The meter's device tables (loudness.hip): the K-weighting cascade's zero-input
// state transition M over 32 samples (biquad_tables' M, simulated in float64)
// in the coordinates u = (y1, y2 of stage 1; y1, y1 - y2 of stage 2), u = T s
// with T its own inverse:
//   [10 coefficients, padded to 20][T M^l T, l = 0..64][I, T M^64 T]
// each power float64 rounded once to float.  Stage 2's poles are a near-double
// pole just inside z = 1: a state's slope y1 - y2 is what later samples
// amplify (by up to 0.37 / (1 - r): 75 at 48 kHz, 300 at 192 kHz), and as a
// coordinate of its own it is rounded relative to itself, not to y1.
void loudness_tables(const float kcoef[10], std::vector<float> &h);
// dsp_loudness_gate's body (arguments checked by the caller)
void loudness_gate(const double *const *z, uint32_t C, uint64_t hops, uint32_t hop, const float *weights,
                   dsp_loudness_result *res);

}  // namespace dspb
