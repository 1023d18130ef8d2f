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
// DSP_PLUGIN_CONV (conv_fdl.hip): partitions and hop of 4096 samples, 8192-point
// frames; a spectrum is 2048 float4 of paired bins in ols_table's order and a
// padding slice of 64 float4 that holds bin 2048
constexpr uint32_t kConvHop = 4096;
constexpr uint32_t kConvSpec4 = 2048 + 64;
constexpr uint32_t kConvMaxTaps = 1u << 20;
// the partitioned table of conv_fdl.hip: ceil(T / kConvHop) spectra of
// 4 kConvSpec4 floats, each FFT_8192(partition zero-padded) / 16384 in float64,
// rounded once to fp32
void conv_table(const float *taps, uint32_t T, float *out);
// dsp_conv_plan's body, and the render's own sizing: partitions = ceil(taps /
// kConvHop), frames = ceil(ceil(L / B) B / kConvHop), scratch_bytes = the
// input's and the output's spectra of one channel group of <= 16 channels.
// Any out pointer may be null.  Returns null, or why the arguments are invalid.
const char *conv_plan(uint32_t taps, uint64_t L, uint32_t B, uint32_t C, uint32_t *partitions, uint64_t *frames,
                      uint64_t *scratch_bytes);
// whether IR_test's `gain -= step` recurrence equals (float)fma(-i, step, gain) for every i < B
bool ramp_closed_form(float gain, float step, uint32_t B);
// a cascade's tables for lanes of `lane_samples` samples (iir.hip biquad_lane_samples()); returns W
uint32_t biquad_tables(const float *cf, uint32_t S, uint32_t lane_samples, std::vector<float> &h);

}  // namespace dspb
