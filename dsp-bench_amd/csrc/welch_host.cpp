// welch_host.cpp -- see welch_host.hpp.
#include "welch_host.hpp"

#include <algorithm>
#include <cmath>

namespace dspb {

int welch_plan(uint64_t L, uint32_t C, int has_ref, const dsp_welch_spec *spec, WelchPlan *p, const char **why) {
    const dsp_welch_spec def{kWelchN, 4096u, DSP_WIN_HANN};
    if (!spec) spec = &def;
    *p = WelchPlan{};
    if (spec->N != kWelchN) { *why = "dsp_welch: N must be 8192"; return 2; }
    if (spec->H == 0 || spec->H > kWelchN) { *why = "dsp_welch: needs 1 <= H <= N"; return 1; }
    if (spec->window != DSP_WIN_HAMMING && spec->window != DSP_WIN_HANN) {
        *why = "dsp_welch: the window must be DSP_WIN_HAMMING or DSP_WIN_HANN";
        return 1;
    }
    if (C == 0) { *why = "dsp_welch: needs C >= 1"; return 1; }
    if (L < kWelchN) { *why = "dsp_welch: no frame (L < N)"; return 1; }
    p->H = spec->H;
    p->window = spec->window;
    p->frames = (L - kWelchN) / spec->H + 1;
    const uint32_t cn = std::min<uint32_t>(C, kWelchGroup);
    p->rows = cn + (has_ref ? 1u : 0u);
    const uint64_t spec_bytes = (uint64_t)kWelchSpec4 * 16;
    const uint64_t fit = std::max<uint64_t>(kWelchSpectraBytes / (p->rows * spec_bytes) / kWelchRun, 1) * kWelchRun;
    const uint64_t need = (p->frames + kWelchRun - 1) / kWelchRun * kWelchRun;  // a short call takes less
    p->chunk = (uint32_t)std::min(fit, need);
    p->runs_cap = p->chunk / kWelchRun;
    p->off_pxx = (uint64_t)p->rows * p->chunk * spec_bytes;
    p->off_pxy = p->off_pxx + (uint64_t)cn * p->runs_cap * kWelchSpec4 * 8;
    p->off_prr = p->off_pxy + (has_ref ? (uint64_t)cn * p->runs_cap * kWelchSpec4 * 16 : 0);
    p->scratch_bytes = p->off_prr + (has_ref ? (uint64_t)p->runs_cap * kWelchSpec4 * 8 : 0);
    float w[kWelchN];  // the table the kernel reads (capi.cpp get_window at scale 1)
    window_table(spec->window, kWelchN, kWelchN, 1.0, w);
    for (uint32_t n = 0; n < kWelchN; ++n) {
        p->win_sum += (double)w[n];
        p->win_sumsq += (double)w[n] * (double)w[n];
    }
    return 0;
}

void welch_derive(const double *const *sxx, const double *srr, const double *const *sxy, uint32_t C, uint32_t bins,
                  uint64_t frames, double sr, double win_sum, double win_sumsq, uint32_t flags, double *const *psd,
                  double *const *H1, double *const *coherence) {
    const double den = (double)frames * ((flags & DSP_WELCH_SPECTRUM) ? win_sum * win_sum : sr * win_sumsq);
    for (uint32_t c = 0; c < C; ++c)
        for (uint32_t k = 0; k < bins; ++k) {
            if (psd) {
                const double g = (k == 0 || k == bins - 1) ? 1.0 : 2.0;  // one-sided: DC and Nyquist are not doubled
                psd[c][k] = g * sxx[c][k] / den;
            }
            if (H1) {
                const double d = srr[k];
                H1[c][2 * k] = d != 0.0 ? sxy[c][2 * k] / d : 0.0;
                H1[c][2 * k + 1] = d != 0.0 ? sxy[c][2 * k + 1] / d : 0.0;
            }
            if (coherence) {
                const double d = sxx[c][k] * srr[k];
                const double re = sxy[c][2 * k], im = sxy[c][2 * k + 1];
                coherence[c][k] = d != 0.0 ? (re * re + im * im) / d : 0.0;
            }
        }
}

}  // namespace dspb
