// host_tables.hpp -- the float64 host maths behind the C ABI's device tables
// (capi.cpp plugin_map): FIR spectra, the IR_test ramp's closed-form check,
// BIQUAD state-transition powers.  No HIP here: plain C++.
#pragma once
#include <cstdint>
#include <vector>

namespace dspb {

constexpr uint32_t kIirPairSections = 2;  // cascades of >= this many sections: channel pairs per wave

// FFT_n(taps zero-padded) in float64 (iterative radix-2, forward e^-i)
void taps_spectrum(const float *taps, uint32_t T, int n, std::vector<double> &re, std::vector<double> &im);
// the 8192-point table of fir_fft_kernel: 8192 + 2 floats
void ols_table(const float *taps, uint32_t T, float *out);
// the 4096-point table of fir_pair_kernel: 8192 floats
void pair_table(const float *taps, uint32_t T, float *out);
// whether IR_test's `gain -= step` recurrence equals (float)fma(-i, step, gain) for every i < B
bool ramp_closed_form(float gain, float step, uint32_t B);
// a cascade's tables for lanes of `lane_samples` samples (iir.hip biquad_lane_samples()); returns W
uint32_t biquad_tables(const float *cf, uint32_t S, uint32_t lane_samples, std::vector<float> &h);

}  // namespace dspb
