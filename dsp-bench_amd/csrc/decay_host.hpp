// decay_host.hpp -- the host half of dsp_decay (dspbench.h): the plan (bands,
// transform size, hop, the row group and the scratch layout) and
// dsp_decay_derive's float64 arithmetic.  No HIP here: plain C++
// (decay_host.cpp), like welch_host.cpp and loudness_host.cpp.
#pragma once
#include <cstdint>

#include "dspbench/dspbench.h"

namespace dspb {

constexpr uint32_t kDecayMaxBands = 32;
constexpr uint32_t kDecayGroup = 16;  // rows per launch (kMaxChannels: capi_bigfft.cpp asserts it)
// What a call's rows may hold of the scratch: the launches walk the (channel,
// band) pairs in groups of rows = clamp(kDecayRowsBytes / row_bytes, 1, 16),
// row_bytes = 8 n (the transform's two work buffers) + 2 (4 n + 8) (the
// channel's and the band's spectrum) + 4 roundup2(L) (the band IR).  One row at
// n = 2^24 is 320 MiB: the scratch never exceeds that plus the words.
constexpr uint64_t kDecayRowsBytes = 256ull << 20;

struct DecayPlan {
    uint32_t fraction = 1;
    int32_t k_lo = 0, k_hi = 0;
    uint32_t bands = 0;
    uint32_t n = 0, P = 0, hop = 0;
    uint64_t hops = 0;   // the length of an energy row: ceil(L / hop) + 1
    uint32_t rows = 0;   // (channel, band) pairs per launch group, channels per forward group
    uint64_t Lp = 0;     // floats between band IR rows: L rounded up to even
    // the scratch, in bytes from its start: [rows][2][n / 2] float2 work,
    // [rows][n / 2 + 1] float2 channel spectra, the same of band spectra,
    // [rows][Lp] band IRs, [rows][hops + 1] float64 pairs of pre-onset partial sums
    uint64_t off_x = 0, off_y = 0, off_ir = 0, off_pre = 0;
    uint64_t scratch_bytes = 0;
    double Qr = 0.0, Qd = 0.0;
    double fm[kDecayMaxBands] = {};
};

// dsp_decay_plan's body: 0, 1 (invalid) or 2 (unsupported) with *why set
int decay_plan(uint64_t L, uint32_t C, uint32_t sr, const dsp_decay_spec *spec, DecayPlan *plan, const char **why);
// hop alone (0: sr % 100 != 0)
uint32_t decay_hop(uint32_t sr);
// dsp_decay_derive's body (arguments checked by the caller)
void decay_derive(const double *energy, const double *moment, uint64_t hops_full, uint32_t hop, uint32_t sr,
                  dsp_decay_result *res);

}  // namespace dspb
