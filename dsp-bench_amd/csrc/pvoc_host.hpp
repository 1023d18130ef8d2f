// pvoc_host.hpp -- the host half of dsp_pvoc, dsp_time_stretch and
// dsp_pitch_ratio (dspbench.h): the output frame count, the chunk ranges, the
// scratch size, the composite's plan and the rational pitch ratio.  No HIP
// here: plain C++ (pvoc_host.cpp), like stft_cx_host.cpp.
#pragma once
#include <cstdint>

#include "dspbench/dspbench.h"
#include "stft_cx_host.hpp"

namespace dspb {

constexpr uint32_t kPvocGroup = 16;   // rows per channel group (kMaxChannels: capi_grid.cpp asserts it)
constexpr uint32_t kPvocChunk = 64;   // output frames a wavefront walks
constexpr uint32_t kPvocChunkMin = 8, kPvocChunkMax = 4096;  // what DSP_DEBUG_PVOC_CHUNK may set instead
constexpr double kPvocRateMin = 0.125, kPvocRateMax = 8.0;
// (double)t is exact and t rate cannot overflow for every output frame t of such a call
constexpr uint64_t kPvocMaxFrames = 1ull << 48;
constexpr uint32_t kPitchMaxTerm = 4096;  // p, q <= this (dsp_resample's largest `up`)
constexpr double kPitchMaxSemitones = 24.0;

// the position output frame t reads at: one float64 product (pvoc.hip forms the same one)
inline double pvoc_position(uint64_t t, double rate) {
    volatile double s = (double)t * rate;  // (volatile: one rounded product, never fused into what follows)
    return s;
}

struct PvocPlan {
    double rate = 0.0;
    uint64_t frames_in = 0;   // F
    uint64_t frames_out = 0;  // F': the t >= 0 with pvoc_position(t, rate) < F
    uint32_t rows = 0;        // min(C, 16)
    uint32_t chunk = 0;       // output frames per chunk
    uint64_t chunks = 0;      // ceil(F' / chunk)
    // the scratch: [rows][chunks][4097] uint32, a chunk's phase sums and then its carries
    uint64_t scratch_bytes = 0;
};

// the plan's body: 0, 1 (invalid) or 2 (unsupported) with *why set
int pvoc_plan(uint64_t F, uint32_t C, const dsp_pvoc_spec *spec, PvocPlan *plan, const char **why,
              uint32_t chunk = kPvocChunk);
// the row stride of either spectrogram against the plan (frames of it)
int pvoc_check_ld(uint64_t frames, uint64_t ld, const char **why);
// the output frames [t0, t1) of chunk c < chunks
struct PvocChunk {
    uint64_t t0 = 0, t1 = 0;
};
PvocChunk pvoc_chunk(const PvocPlan &p, uint64_t c);

// dsp_time_stretch: dsp_stft(H), dsp_pvoc(rate), dsp_istft(H) over two dense device spectrograms
struct StretchPlan {
    dsp_stft_spec fwd{};
    dsp_istft_spec inv{};
    dsp_pvoc_spec pv{};
    uint64_t frames_in = 0, frames_out = 0;
    uint64_t Lout_full = 0;     // N + (F' - 1) H
    uint64_t Lout_default = 0;  // min(Lout_full, round(L / rate))
    uint32_t rows = 0;          // min(C, 16)
    uint64_t ld = 0;            // 2 K floats: the scratch rows are dense
    uint64_t in_bytes = 0, out_bytes = 0;  // the two spectrograms of `rows` rows
    uint64_t device_bytes = 0;  // their sum
};
int stretch_plan(uint64_t L, uint32_t C, const dsp_stretch_spec *spec, StretchPlan *plan, const char **why);

// the best p / q ~ 2^(semitones / 12) with p, q <= 4096 (continued fractions
// with the last semiconvergent, fractions.Fraction.limit_denominator's rule on
// whichever of the ratio and its inverse is below 1); 0 or 1 (invalid)
int pitch_ratio(double semitones, uint32_t *p, uint32_t *q, const char **why);

// A pitch shift by p / q = pitch_ratio(semitones) that keeps the length: L samples,
// zero-padded to `padded` = the least max(L, N) + j H whose stretch at rate q / p
// reaches `stretched` = floor(L p / q + 1 / 2) samples (at least 1), are stretched
// to that many; dsp_resample(p, q) then gives them back at the pitch (its plan
// tells the final length, within a sample of L).  0, 1 (invalid) or 2 (unsupported)
struct PitchPlan {
    uint32_t p = 0, q = 0;
    dsp_stretch_spec stretch{};
    uint64_t padded = 0, stretched = 0;
};
int pitch_plan(uint64_t L, uint32_t C, double semitones, uint32_t H, int32_t window, PitchPlan *plan, const char **why);

}  // namespace dspb
