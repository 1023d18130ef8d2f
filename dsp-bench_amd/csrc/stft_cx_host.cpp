// stft_cx_host.cpp -- see stft_cx_host.hpp.
#include "stft_cx_host.hpp"

#include <algorithm>
#include <cmath>

namespace dspb {

static const char *window_rule(bool inverse, int32_t window) {
    if (window == DSP_WIN_HAMMING || window == DSP_WIN_HANN) return nullptr;
    return inverse ? "dsp_istft: the window must be DSP_WIN_HAMMING or DSP_WIN_HANN"
                   : "dsp_stft: the window must be DSP_WIN_HAMMING or DSP_WIN_HANN";
}

int stft_cx_plan(uint64_t L, uint32_t C, const dsp_stft_spec *spec, StftCxPlan *p, const char **why) {
    const dsp_stft_spec def{kStftCxN, 4096u, DSP_WIN_HANN};
    if (!spec) spec = &def;
    *p = StftCxPlan{};
    if (spec->N != kStftCxN) { *why = "dsp_stft: N must be 8192"; return 2; }
    if (spec->H == 0 || spec->H > kStftCxN) { *why = "dsp_stft: needs 1 <= H <= N"; return 1; }
    if (const char *w = window_rule(false, spec->window)) { *why = w; return 1; }
    if (C == 0) { *why = "dsp_stft: needs C >= 1"; return 1; }
    if (L < kStftCxN) { *why = "dsp_stft: no frame (L < N)"; return 1; }
    p->H = spec->H;
    p->window = spec->window;
    p->frames = (L - kStftCxN) / spec->H + 1;
    p->min_ld = 2ull * kStftCxBins;
    return 0;
}

int istft_plan(uint64_t F, uint32_t C, const dsp_istft_spec *spec, IstftPlan *p, const char **why) {
    const dsp_istft_spec def{kStftCxN, 4096u, DSP_WIN_HANN, 1e-10};
    if (!spec) spec = &def;
    *p = IstftPlan{};
    if (spec->N != kStftCxN) { *why = "dsp_istft: N must be 8192"; return 2; }
    if (spec->H == 0 || spec->H > kStftCxN) { *why = "dsp_istft: needs 512 <= H <= N"; return 1; }
    if (spec->H < kIstftMinHop) { *why = "dsp_istft: H < 512 (more than 16 frames on a sample)"; return 2; }
    if (const char *w = window_rule(true, spec->window)) { *why = w; return 1; }
    if (!(std::isfinite(spec->floor) && spec->floor >= 1e-12 && spec->floor <= 1.0)) {
        *why = "dsp_istft: floor must be finite and in [1e-12, 1]";
        return 1;
    }
    if (C == 0) { *why = "dsp_istft: needs C >= 1"; return 1; }
    if (F == 0) { *why = "dsp_istft: no frame (F = 0)"; return 1; }
    if (F - 1 > (UINT64_MAX - kStftCxN) / spec->H) { *why = "dsp_istft: Lout does not fit 64 bits"; return 2; }
    p->H = spec->H;
    p->window = spec->window;
    p->floor = (float)spec->floor;
    p->frames = F;
    p->Lout_full = kStftCxN + (F - 1) * spec->H;
    p->overlap = (kStftCxN + spec->H - 1) / spec->H;
    p->rows = std::min<uint32_t>(C, kStftCxGroup);
    p->chunk = (uint32_t)(kIstftChunkBytes / (p->rows * kIstftFrameBytes));
    p->slots = (uint32_t)std::min<uint64_t>(F, (uint64_t)p->chunk + p->overlap - 1);
    p->scratch_bytes = (uint64_t)p->rows * p->slots * kIstftFrameBytes;
    return 0;
}

int stft_cx_check_ld(bool inv, uint64_t frames, uint64_t ld, const char **why) {
    if (ld & 1u) { *why = inv ? "dsp_istft: ld must be even" : "dsp_stft: ld must be even"; return 1; }
    if (ld < 2ull * kStftCxBins) {
        *why = inv ? "dsp_istft: ld < 2 K = 8194" : "dsp_stft: ld < 2 K = 8194 (dsp_stft_plan's min_ld)";
        return 1;
    }
    if (frames > (UINT64_MAX >> 3) / ld) {
        *why = inv ? "dsp_istft: F ld does not fit" : "dsp_stft: frames ld does not fit";
        return 2;
    }
    return 0;
}

int istft_check_lout(const IstftPlan &p, uint64_t Lout, const char **why) {
    if (Lout == 0) { *why = "dsp_istft: needs Lout >= 1"; return 1; }
    if (Lout > p.Lout_full) { *why = "dsp_istft: Lout > N + (F - 1) H"; return 1; }
    return 0;
}

IstftChunk istft_chunk(const IstftPlan &p, uint64_t f0, uint64_t Lout) {
    IstftChunk c;
    if (f0 >= p.frames || p.chunk == 0) return c;
    const uint64_t nf = std::min<uint64_t>(p.frames - f0, p.chunk);
    const uint64_t i0 = f0 * p.H;
    if (i0 >= Lout) return c;
    const bool last = f0 + nf == p.frames;
    c.f0 = f0;
    c.i0 = i0;
    c.i1 = last ? Lout : std::min<uint64_t>(Lout, (f0 + nf) * p.H);
    c.fa = f0 >= p.overlap - 1 ? f0 - (p.overlap - 1) : 0;
    const uint64_t fe = std::min<uint64_t>(f0 + nf, (c.i1 - 1) / p.H + 1);  // one past the last frame a sample < i1 touches
    c.nf = (uint32_t)nf;
    c.ns = (uint32_t)(fe - c.fa);
    return c;
}

}  // namespace dspb
