// host_tables.hpp -- the float64 host maths behind the C ABI's device tables
// (capi.cpp plugin_map): FIR spectra, the IR_test ramp's closed-form check,
// BIQUAD state-transition powers.  No HIP here: plain C++.
#pragma once
#include <cstdint>
#include <vector>

namespace dspb {

constexpr uint32_t kIirPairSections = 2;  // cascades of >= this many sections: channel pairs per wave

// the cosine windows w[n] = a - b cos(2 pi n / (valid - 1)) (dspbench.h dsp_window; anything else: Hamming)
void window_coefficients(int kind, double *a, double *b);
// The one window table (capi.cpp get_window's device tables, welch_host.cpp's
// sums): length `valid`, symmetric (ref ippsWinHamming_32f convention), times
// `scale`, zero-padded to N.  Computed in double, rounded once to float.
void window_table(int kind, uint32_t N, uint32_t valid, double scale, float *h);
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
// dsp_resample (resample.hip): the polyphase Kaiser-windowed sinc of
// dspbench.h.  up = sr_out / g, down = sr_in / g; rho = rolloff min(1, up /
// down), W = zeros / rho, half = ceil(W), taps = 2 half per phase
struct ResamplePlan {
    uint32_t up = 0, down = 0, half = 0, taps = 0;
    uint32_t zeros = 0;
    double beta = 0.0, rolloff = 0.0, rho = 0.0, W = 0.0;
    double inv_i0_beta = 1.0;  // 1 / I0(beta)
    uint64_t Lout = 0;         // ceil(L up / down)
    uint64_t table_bytes = 0;  // up taps floats
};
constexpr uint32_t kResampleMaxUp = 4096, kResampleMaxTaps = 8192;
constexpr uint64_t kResampleMaxTableBytes = 8ull << 20;
// dsp_resample_plan's body.  Returns 0, or 1 (invalid) / 2 (unsupported) with *why set.
int resample_plan(uint32_t sr_in, uint32_t sr_out, uint64_t L, uint32_t zeros, double beta, double rolloff,
                  ResamplePlan *plan, const char **why);
// h(u) of the plan in float64 (zero for |u| >= W)
double resample_h(const ResamplePlan &p, double u);
// table[phi][i] = (float)h(half - 1 - i + phi / up), phi < up, i < taps; row
// phi at out + phi * row_stride + row_offset (the other floats are left alone)
void resample_table(const ResamplePlan &p, float *out, uint64_t row_stride, uint64_t row_offset);
// dsp_rfft / dsp_irfft / dsp_deconvolve (fft_big.hip): n a power of two in
// [2^10, 2^24]; the M = n / 2 point complex transform runs as 2..4 Stockham
// passes of radix 64, 32 or 8, largest first
constexpr uint32_t kBigFftMinN = 1u << 10, kBigFftMaxN = 1u << 24;
constexpr uint32_t kBigTwShift = 12;  // W_n^K = hi[K >> 12] lo[K & 4095]
// the plan of n: *passes and radix[0..passes) (the rest 0).  Returns false for an n outside the range.
bool rfft_plan(uint32_t n, uint32_t *passes, uint32_t radix[4]);
// device scratch of one channel: two work buffers of M complex
inline uint64_t rfft_scratch_bytes(uint32_t n) { return 2ull * 8ull * (n / 2); }
// floats of the twiddle table of n: lo[k] = W_n^k for k < min(n, 4096), then
// hi[h] = W_n^(4096 h) for h < max(1, n / 4096), interleaved (re, im), float64 rounded once
inline uint32_t rfft_twiddle_lo(uint32_t n) { return n < (1u << kBigTwShift) ? n : (1u << kBigTwShift); }
inline uint32_t rfft_twiddle_hi(uint32_t n) { return n >> kBigTwShift ? n >> kBigTwShift : 1u; }
void rfft_twiddles(uint32_t n, std::vector<float> &h);
// dsp_deconv_plan's body: n = max(1024, the next power of two >= max(Ly, Ls));
// the scratch of a call: a group's work buffers and spectra, the excitation's
// spectrum, 16 bytes of words.  Returns 0, 1 (invalid) or 2 (unsupported) with *why set.
int deconv_plan(uint64_t Ly, uint64_t Ls, uint32_t C, uint32_t *n, uint64_t *scratch_bytes, const char **why);
// whether IR_test's `gain -= step` recurrence equals (float)fma(-i, step, gain) for every i < B
bool ramp_closed_form(float gain, float step, uint32_t B);
// a cascade's tables for lanes of `lane_samples` samples (iir.hip biquad_lane_samples()); returns W
uint32_t biquad_tables(const float *cf, uint32_t S, uint32_t lane_samples, std::vector<float> &h);

}  // namespace dspb
