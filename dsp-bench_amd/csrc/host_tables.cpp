// host_tables.cpp -- float64 host maths of the device tables (host_tables.hpp).
#include "host_tables.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>

namespace dspb {

// FFT(taps zero-padded to 8192) / 16384 in double, laid out for
// fir_fft.hip: for ka < 16 and lane l, 8 floats
//   (Re H[k1], Re H[k2], Im H[k1], Im H[k2], Re H[M-k1], Re H[M-k2], Im H[M-k1], Im H[M-k2])
// with k1 = l + 64 ka, k2 = k1 + 1024, M = 4096; then H[2048] (re, im).
// FFT_n(taps zero-padded) in float64 (iterative radix-2, forward e^-i)
void window_coefficients(int kind, double *a, double *b) {
    *a = 0.54, *b = 0.46;
    if (kind == 1) *a = 0.5, *b = 0.5;        // DSP_WIN_HANN
    else if (kind == 2) *a = 1.0, *b = 0.0;   // DSP_WIN_RECT
}

void window_table(int kind, uint32_t N, uint32_t valid, double scale, float *h) {
    double a, b;
    window_coefficients(kind, &a, &b);
    for (uint32_t n = 0; n < N; ++n)
        h[n] = n >= valid ? 0.f
               : valid == 1 ? (float)scale
                            : (float)(scale * (a - b * std::cos(2.0 * M_PI * (double)n / (double)(valid - 1))));
}

void taps_spectrum(const float *taps, uint32_t T, int n, std::vector<double> &re, std::vector<double> &im) {
    re.assign(n, 0.0);
    im.assign(n, 0.0);
    for (uint32_t i = 0; i < T; ++i) re[i] = taps[i];
    for (int i = 1, j = 0; i < n; ++i) {  // iterative radix-2, forward (e^-i)
        int bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
    }
    for (int len = 2; len <= n; len <<= 1) {
        const int hlen = len >> 1;
        for (int k = 0; k < hlen; ++k) {
            const double a = -2.0 * M_PI * k / len, wr = std::cos(a), wi = std::sin(a);
            for (int s0 = 0; s0 < n; s0 += len) {
                const double xr = re[s0 + k + hlen] * wr - im[s0 + k + hlen] * wi;
                const double xi = re[s0 + k + hlen] * wi + im[s0 + k + hlen] * wr;
                re[s0 + k + hlen] = re[s0 + k] - xr;
                im[s0 + k + hlen] = im[s0 + k] - xi;
                re[s0 + k] += xr;
                im[s0 + k] += xi;
            }
        }
    }
}

// the 8192-point table of fir_fft_kernel (kOlsHop 7168, one channel per frame)
void ols_table(const float *taps, uint32_t T, float *out) {
    std::vector<double> re, im;
    taps_spectrum(taps, T, 8192, re, im);
    const double sc = 1.0 / 16384.0;
    for (int ka = 0; ka < 16; ++ka)
        for (int l = 0; l < 64; ++l) {
            const int k1 = l + 64 * ka, k2 = k1 + 1024, m1 = 4096 - k1, m2 = 4096 - k2;
            float *o = out + 8 * (64 * ka + l);
            o[0] = (float)(re[k1] * sc); o[1] = (float)(re[k2] * sc);
            o[2] = (float)(im[k1] * sc); o[3] = (float)(im[k2] * sc);
            o[4] = (float)(re[m1] * sc); o[5] = (float)(re[m2] * sc);
            o[6] = (float)(im[m1] * sc); o[7] = (float)(im[m2] * sc);
        }
    out[8192] = (float)(re[2048] * sc);
    out[8193] = (float)(im[2048] * sc);
}

// the 4096-point table of fir_pair_kernel (two channels as one complex
// signal): H = FFT_4096(taps) / 4096 (the inverse's scale), as float4
// [q][lane] = (Re H[l + 64 q], Re H[l + 64 (q + 32)], Im .., Im ..), the
// pairing of the transform's packed last combine
void pair_table(const float *taps, uint32_t T, float *out) {
    std::vector<double> re, im;
    taps_spectrum(taps, T, 4096, re, im);
    const double sc = 1.0 / 4096.0;
    for (int q = 0; q < 32; ++q)
        for (int l = 0; l < 64; ++l) {
            const int k0 = l + 64 * q, k1 = k0 + 2048;
            float *o = out + 4 * (64 * q + l);
            o[0] = (float)(re[k0] * sc); o[1] = (float)(re[k1] * sc);
            o[2] = (float)(im[k0] * sc); o[3] = (float)(im[k1] * sc);
        }
}

// the partitioned table of conv_fdl.hip (DSP_PLUGIN_CONV): per partition p of
// kConvHop taps, H_p = FFT_8192(partition zero-padded) / 16384 (the inverse's
// 1/4096 and the two real-split halvings, as ols_table) in ols_table's pair
// order as float4 [2 (64 ka + l) + h], then the padding slice: bin 2048 as
// (re, 0, im, 0) and 63 zero float4
void conv_table(const float *taps, uint32_t T, float *out) {
    std::vector<double> re, im;
    const double sc = 1.0 / 16384.0;
    const uint32_t parts = (T + kConvHop - 1) / kConvHop;
    for (uint32_t p = 0; p < parts; ++p) {
        const uint32_t t0 = p * kConvHop;
        taps_spectrum(taps + t0, std::min(kConvHop, T - t0), 8192, re, im);
        float *sp = out + (size_t)p * 4 * kConvSpec4;
        for (int ka = 0; ka < 16; ++ka)
            for (int l = 0; l < 64; ++l) {
                const int k1 = l + 64 * ka, k2 = k1 + 1024, m1 = 4096 - k1, m2 = 4096 - k2;
                float *o = sp + 8 * (64 * ka + l);
                o[0] = (float)(re[k1] * sc); o[1] = (float)(re[k2] * sc);
                o[2] = (float)(im[k1] * sc); o[3] = (float)(im[k2] * sc);
                o[4] = (float)(re[m1] * sc); o[5] = (float)(re[m2] * sc);
                o[6] = (float)(im[m1] * sc); o[7] = (float)(im[m2] * sc);
            }
        float *pad = sp + 4 * 2048;
        std::fill(pad, pad + 4 * 64, 0.f);
        pad[0] = (float)(re[2048] * sc);
        pad[2] = (float)(im[2048] * sc);
    }
}

const char *conv_plan(uint32_t taps, uint64_t L, uint32_t B, uint32_t C, uint32_t *partitions, uint64_t *frames,
                      uint64_t *scratch_bytes) {
    if (taps == 0 || taps > kConvMaxTaps) return "DSP_PLUGIN_CONV: 1..2^20 taps";
    if (B == 0) return "block size B must be > 0";
    if (L > (1ull << 48)) return "DSP_PLUGIN_CONV: L > 2^48";
    const uint64_t F = ((L + B - 1) / B * B + kConvHop - 1) / kConvHop;
    if (partitions) *partitions = (taps + kConvHop - 1) / kConvHop;
    if (frames) *frames = F;
    if (scratch_bytes) *scratch_bytes = 2 * (uint64_t)std::min<uint32_t>(C, 16) * F * kConvSpec4 * 16;
    return nullptr;
}

static double bessel_i0(double x);

// dsp_resample: the plan of a rate pair and quality, all in integers and float64
int resample_plan(uint32_t sr_in, uint32_t sr_out, uint64_t L, uint32_t zeros, double beta, double rolloff,
                  ResamplePlan *plan, const char **why) {
    const char *dummy;
    if (!why) why = &dummy;
    if (sr_in == 0 || sr_out == 0) return *why = "dsp_resample: sample rates must be >= 1", 1;
    if (zeros < 4 || zeros > 64) return *why = "dsp_resample: zeros must be 4..64", 1;
    if (!(beta >= 0.0 && beta <= 20.0)) return *why = "dsp_resample: beta must be 0..20", 1;
    if (!(rolloff >= 0.5 && rolloff <= 1.0)) return *why = "dsp_resample: rolloff must be 0.5..1", 1;
    uint32_t a = sr_in, b = sr_out;
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    ResamplePlan p;
    p.up = sr_out / a;
    p.down = sr_in / a;
    p.zeros = zeros;
    p.beta = beta;
    p.rolloff = rolloff;
    p.rho = rolloff * std::min(1.0, (double)p.up / (double)p.down);
    p.W = (double)zeros / p.rho;
    if (p.up > kResampleMaxUp) return *why = "dsp_resample: sr_out / gcd > 4096", 2;
    if (std::ceil(p.W) * 2.0 > (double)kResampleMaxTaps) return *why = "dsp_resample: more than 8192 taps per phase", 2;
    p.half = (uint32_t)std::ceil(p.W);
    p.taps = 2 * p.half;
    p.table_bytes = (uint64_t)p.up * p.taps * sizeof(float);
    if (p.table_bytes > kResampleMaxTableBytes) return *why = "dsp_resample: table larger than 8 MiB", 2;
    if (L > ((1ull << 63) - p.down) / p.up) return *why = "dsp_resample: L up overflows 2^63", 2;
    p.Lout = (L * p.up + p.down - 1) / p.down;
    p.inv_i0_beta = 1.0 / bessel_i0(beta);
    if (plan) *plan = p;
    return 0;
}

// I0 by its power series sum ((x / 2)^k / k!)^2, to convergence in float64
static double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 1000; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

double resample_h(const ResamplePlan &p, double u) {
    if (!(std::fabs(u) < p.W)) return 0.0;
    const double t = p.rho * u, r = u / p.W;
    const double sinc = t == 0.0 ? 1.0 : std::sin(M_PI * t) / (M_PI * t);
    return p.rho * sinc * bessel_i0(p.beta * std::sqrt(std::max(0.0, 1.0 - r * r))) * p.inv_i0_beta;
}

void resample_table(const ResamplePlan &p, float *out, uint64_t row_stride, uint64_t row_offset) {
    for (uint32_t phi = 0; phi < p.up; ++phi) {
        float *row = out + phi * row_stride + row_offset;
        const double frac = (double)phi / (double)p.up;
        for (uint32_t i = 0; i < p.taps; ++i)
            row[i] = (float)resample_h(p, ((double)p.half - 1.0 - (double)i) + frac);
    }
}

// IR_test (build/IR_test.cpp:47-58) runs `gain -= step` in double from the
// float parameters.  The sequence is often exact -- every partial result a
// double -- and then table[i] = (float)(gain - i step) is one f64 FMA, with
// no sequential kernel.  This checks that bit for bit against the recurrence
// itself (B host f64 subtractions, cached per parameter set).
bool ramp_closed_form(float gain, float step, uint32_t B) {
    if (B > (1u << 16)) return false;
    static std::mutex mu;
    static struct { uint32_t g, s, B; bool ok; } last = {0, 0, 0, false};
    uint32_t gb, sb;
    std::memcpy(&gb, &gain, 4);
    std::memcpy(&sb, &step, 4);
    std::lock_guard<std::mutex> lk(mu);
    if (last.B == B && last.g == gb && last.s == sb) return last.ok;
    double g = gain;
    const double s = step;
    bool ok = true;
    for (uint32_t i = 0; i < B && ok; ++i) {
        const double c = std::fma(-(double)i, s, (double)gain);
        ok = std::memcmp(&c, &g, sizeof(double)) == 0;
        g -= s;
    }
    last = {gb, sb, B, ok};
    return ok;
}

// DSP_PLUGIN_BIQUAD (iir.hip): the cascade's zero-input state transition over
// T = lane_samples samples, M (D x D, D = 2 S, state = (y1, y2) per
// section; section k's x history is section k-1's y history), simulated in
// float64 from each unit state, then its powers:
//   [5 S coefficients, padded to 20][M^l, l = 0..64][M^(64 k), k = 0..256]
// Returns W, the number of preceding tiles (of 64 T samples) whose aggregate
// reaches a tile's entering state with a weight ||M^(64 k)||_inf above 2^-48
// (every later power below it too): 1..256, or 0 when the transition does not
// decay that fast (then the kernel's inclusive look-back).
uint32_t biquad_tables(const float *cf, uint32_t S, uint32_t lane_samples, std::vector<float> &h) {
    const int D = 2 * (int)S, T = (int)lane_samples;
    std::vector<double> M((size_t)D * D);
    for (int j = 0; j < D; ++j) {
        double Y1[4], Y2[4], X1[4], X2[4];
        for (int k = 0; k < (int)S; ++k) {
            Y1[k] = (2 * k == j) ? 1.0 : 0.0;
            Y2[k] = (2 * k + 1 == j) ? 1.0 : 0.0;
        }
        for (int k = 0; k < (int)S; ++k) {
            X1[k] = k ? Y1[k - 1] : 0.0;
            X2[k] = k ? Y2[k - 1] : 0.0;
        }
        for (int n = 0; n < T; ++n) {
            double v = 0.0;
            for (int k = 0; k < (int)S; ++k) {
                const float *c = cf + 5 * k;
                const double y = (double)c[0] * v + (double)c[1] * X1[k] + (double)c[2] * X2[k] -
                                 (double)c[3] * Y1[k] - (double)c[4] * Y2[k];
                X2[k] = X1[k];
                X1[k] = v;
                Y2[k] = Y1[k];
                Y1[k] = y;
                v = y;
            }
        }
        for (int k = 0; k < (int)S; ++k) {
            M[(size_t)(2 * k) * D + j] = Y1[k];
            M[(size_t)(2 * k + 1) * D + j] = Y2[k];
        }
    }
    auto mul = [D](const std::vector<double> &a, const std::vector<double> &b) {
        std::vector<double> r((size_t)D * D, 0.0);
        for (int i = 0; i < D; ++i)
            for (int k = 0; k < D; ++k)
                for (int j = 0; j < D; ++j) r[(size_t)i * D + j] += a[(size_t)i * D + k] * b[(size_t)k * D + j];
        return r;
    };
    std::vector<double> I((size_t)D * D, 0.0);
    for (int i = 0; i < D; ++i) I[(size_t)i * D + i] = 1.0;
    h.assign(20 + (65 + 257) * (size_t)D * D, 0.f);
    for (uint32_t q = 0; q < 5 * S; ++q) h[q] = cf[q];
    std::vector<double> Q = I;
    float *o = h.data() + 20;
    for (int l = 0; l <= 64; ++l) {
        for (int q = 0; q < D * D; ++q) o[(size_t)l * D * D + q] = (float)Q[q];
        Q = mul(M, Q);
    }
    std::vector<double> Pm = I, step = I;
    for (int l = 0; l < 64; ++l) step = mul(M, step);  // M^64 in float64
    o += (size_t)65 * D * D;
    uint32_t W = 0;  // the last k <= 256 whose weight is above the cut, + 1
    bool finite = true;
    for (int k = 0; k <= 256; ++k) {
        double nrm = 0.0;
        for (int i = 0; i < D; ++i) {
            double row = 0.0;
            for (int j = 0; j < D; ++j) row += std::fabs(Pm[(size_t)i * D + j]);
            nrm = std::max(nrm, row);
        }
        finite = finite && std::isfinite(nrm);
        if (nrm > std::ldexp(1.0, -48)) W = (uint32_t)k + 1;
        for (int q = 0; q < D * D; ++q) o[(size_t)k * D * D + q] = (float)Pm[q];
        Pm = mul(step, Pm);
    }
    // decayed within the table: the weights of the last 64 powers are all below the cut
    return (finite && W <= 192) ? std::max<uint32_t>(W, 1) : 0u;
}

bool rfft_plan(uint32_t n, uint32_t *passes, uint32_t radix[4]) {
    if (n < kBigFftMinN || n > kBigFftMaxN || (n & (n - 1))) return false;
    uint32_t m = 0;  // log2 M
    while ((2u << m) < n) ++m;
    const uint32_t p = (m + 5) / 6;
    uint32_t d = 6 * p - m;  // bits short of p passes of 64: a last pass of 8 takes 3, passes of 32 one each
    uint32_t bits[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < p; ++i) bits[i] = 6;
    uint32_t last = p;
    if (d >= 3) bits[--last] = 3, d -= 3;
    for (uint32_t i = 0; i < d; ++i) bits[--last] = 5;
    if (passes) *passes = p;
    if (radix)
        for (uint32_t i = 0; i < 4; ++i) radix[i] = bits[i] ? 1u << bits[i] : 0u;
    return true;
}

void rfft_twiddles(uint32_t n, std::vector<float> &h) {
    const uint32_t lo = rfft_twiddle_lo(n), hi = rfft_twiddle_hi(n);
    h.assign(2 * ((size_t)lo + hi), 0.f);
    const double w = -2.0 * M_PI / (double)n;
    for (uint32_t k = 0; k < lo; ++k) {
        h[2 * k] = (float)std::cos(w * (double)k);
        h[2 * k + 1] = (float)std::sin(w * (double)k);
    }
    for (uint32_t j = 0; j < hi; ++j) {
        const double a = w * (double)((uint64_t)j << kBigTwShift);
        h[2 * ((size_t)lo + j)] = (float)std::cos(a);
        h[2 * ((size_t)lo + j) + 1] = (float)std::sin(a);
    }
}

int deconv_plan(uint64_t Ly, uint64_t Ls, uint32_t C, uint32_t *n, uint64_t *scratch_bytes, const char **why) {
    const char *dummy;
    if (!why) why = &dummy;
    if (Ly == 0 || Ls == 0) return *why = "dsp_deconvolve: needs Ly >= 1 and Ls >= 1", 1;
    if (C == 0) return *why = "dsp_deconvolve: needs C >= 1", 1;
    const uint64_t len = std::max(Ly, Ls);
    if (len > kBigFftMaxN) return *why = "dsp_deconvolve: more than 2^24 samples", 2;
    uint32_t nn = kBigFftMinN;
    while (nn < len) nn <<= 1;
    const uint64_t g = std::min<uint32_t>(C, 16);
    if (n) *n = nn;
    if (scratch_bytes) *scratch_bytes = g * rfft_scratch_bytes(nn) + (g + 1) * 8ull * (nn / 2 + 1) + 16;
    return 0;
}

}  // namespace dspb
