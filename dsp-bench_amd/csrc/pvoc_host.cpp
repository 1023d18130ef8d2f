// pvoc_host.cpp -- see pvoc_host.hpp.
#include "pvoc_host.hpp"

#include <algorithm>
#include <cmath>

namespace dspb {

// F' = the number of t >= 0 with fl(t rate) < F.  fl(t rate) does not decrease
// with t, so the count is the least t that fails; ceil(F / rate) is within a
// step or two of it and the walk settles the rounding.
static uint64_t pvoc_frames_out(uint64_t F, double rate) {
    const double Fd = (double)F;  // exact: F <= 2^48
    uint64_t t = (uint64_t)std::ceil(Fd / rate);
    while (t > 0 && !(pvoc_position(t - 1, rate) < Fd)) --t;
    while (pvoc_position(t, rate) < Fd) ++t;
    return t;
}

int pvoc_plan(uint64_t F, uint32_t C, const dsp_pvoc_spec *spec, PvocPlan *p, const char **why, uint32_t chunk) {
    *p = PvocPlan{};
    if (!spec) { *why = "dsp_pvoc: spec is NULL"; return 1; }
    if (!(std::isfinite(spec->rate) && spec->rate >= kPvocRateMin && spec->rate <= kPvocRateMax)) {
        *why = "dsp_pvoc: rate must be finite and in [1/8, 8]";
        return 1;
    }
    if (C == 0) { *why = "dsp_pvoc: needs C >= 1"; return 1; }
    if (F == 0) { *why = "dsp_pvoc: no frame (F = 0)"; return 1; }
    if (F > kPvocMaxFrames) { *why = "dsp_pvoc: more than 2^48 frames"; return 2; }
    p->rate = spec->rate;
    p->frames_in = F;
    p->frames_out = pvoc_frames_out(F, spec->rate);
    p->rows = std::min<uint32_t>(C, kPvocGroup);
    p->chunk = chunk >= kPvocChunkMin && chunk <= kPvocChunkMax ? chunk : kPvocChunk;
    p->chunks = (p->frames_out + p->chunk - 1) / p->chunk;
    p->scratch_bytes = (uint64_t)p->rows * p->chunks * kStftCxBins * sizeof(uint32_t);
    return 0;
}

int pvoc_check_ld(uint64_t frames, uint64_t ld, const char **why) {
    if (ld & 1u) { *why = "dsp_pvoc: ld must be even"; return 1; }
    if (ld < 2ull * kStftCxBins) { *why = "dsp_pvoc: ld < 2 K = 8194"; return 1; }
    if (frames > (UINT64_MAX >> 3) / ld) { *why = "dsp_pvoc: frames ld does not fit"; return 2; }
    return 0;
}

PvocChunk pvoc_chunk(const PvocPlan &p, uint64_t c) {
    PvocChunk ch;
    if (c >= p.chunks) return ch;
    ch.t0 = c * p.chunk;
    ch.t1 = std::min<uint64_t>(p.frames_out, ch.t0 + p.chunk);
    return ch;
}

int stretch_plan(uint64_t L, uint32_t C, const dsp_stretch_spec *spec, StretchPlan *p, const char **why) {
    *p = StretchPlan{};
    if (!spec) { *why = "dsp_time_stretch: spec is NULL"; return 1; }
    p->fwd = dsp_stft_spec{spec->N, spec->H, spec->window};
    p->inv = dsp_istft_spec{spec->N, spec->H, spec->window, spec->floor};
    p->pv = dsp_pvoc_spec{spec->rate};
    StftCxPlan fp;
    PvocPlan vp;
    IstftPlan ip;
    // the inverse's rules on H, the window and the floor are the composite's; F = 1 stands in until F' is known
    if (int r = istft_plan(1, C, &p->inv, &ip, why)) return r;
    if (int r = stft_cx_plan(L, C, &p->fwd, &fp, why)) return r;
    if (int r = pvoc_plan(fp.frames, C, &p->pv, &vp, why)) return r;
    if (int r = istft_plan(vp.frames_out, C, &p->inv, &ip, why)) return r;
    p->frames_in = fp.frames;
    p->frames_out = vp.frames_out;
    p->Lout_full = ip.Lout_full;
    const double want = std::round((double)L / spec->rate);
    p->Lout_default = std::max<uint64_t>(1, std::min<uint64_t>(p->Lout_full, want >= 1.8e19 ? UINT64_MAX : (uint64_t)want));
    p->rows = std::min<uint32_t>(C, kPvocGroup);
    p->ld = 2ull * kStftCxBins;
    const uint64_t row = p->ld * sizeof(float);
    if (p->frames_in > (UINT64_MAX >> 8) / row || p->frames_out > (UINT64_MAX >> 8) / row) {
        *why = "dsp_time_stretch: the spectrograms do not fit 64 bits";
        return 2;
    }
    p->in_bytes = p->rows * p->frames_in * row;
    p->out_bytes = p->rows * p->frames_out * row;
    p->device_bytes = p->in_bytes + p->out_bytes;
    return 0;
}

int pitch_ratio(double semitones, uint32_t *p, uint32_t *q, const char **why) {
    if (!(std::isfinite(semitones) && std::fabs(semitones) <= kPitchMaxSemitones)) {
        *why = "dsp_pitch_ratio: semitones must be finite and in [-24, 24]";
        return 1;
    }
    // x = 2^(-|semitones| / 12) in [1/4, 1], as the exact rational n0 / d0 the double is
    const double x = std::exp2(-std::fabs(semitones) / 12.0);
    int e;
    const double m = std::frexp(x, &e);  // x = m 2^e, m in [1/2, 1), e in -1..1
    uint64_t n0 = (uint64_t)std::ldexp(m, 53), d0 = 1ull << (53 - e);
    while (!(n0 & 1u) && d0 > 1) n0 >>= 1, d0 >>= 1;
    uint64_t bn, bd;
    if (d0 <= kPitchMaxTerm) {
        bn = n0, bd = d0;
    } else {
        uint64_t p0 = 0, q0 = 1, p1 = 1, q1 = 0, n = n0, d = d0;
        for (;;) {
            const uint64_t a = n / d, q2 = q0 + a * q1;
            if (q2 > kPitchMaxTerm) break;
            const uint64_t p2 = p0 + a * p1, r = n - a * d;
            p0 = p1, q0 = q1, p1 = p2, q1 = q2;
            n = d, d = r;
        }
        const uint64_t k = (kPitchMaxTerm - q0) / q1;
        const uint64_t n1 = p0 + k * p1, d1 = q0 + k * q1;  // the last semiconvergent
        typedef unsigned __int128 u128;
        auto dist = [&](uint64_t an, uint64_t ad) {  // |an / ad - n0 / d0| ad d0
            const u128 l = (u128)an * d0, r = (u128)n0 * ad;
            return l > r ? l - r : r - l;
        };
        // |p1 / q1 - x| <= |n1 / d1 - x|, cross-multiplied
        if (dist(p1, q1) * d1 <= dist(n1, d1) * q1) bn = p1, bd = q1;
        else bn = n1, bd = d1;
    }
    // bn / bd <= 1 approximates the ratio of a downward shift; an upward one is its inverse
    const bool up = semitones > 0;
    if (p) *p = (uint32_t)(up ? bd : bn);
    if (q) *q = (uint32_t)(up ? bn : bd);
    return 0;
}

int pitch_plan(uint64_t L, uint32_t C, double semitones, uint32_t H, int32_t window, PitchPlan *pl, const char **why) {
    *pl = PitchPlan{};
    if (int r = pitch_ratio(semitones, &pl->p, &pl->q, why)) return r;
    if (L == 0) { *why = "dsp_pitch_shift_plan: needs L >= 1"; return 1; }
    if (L > (1ull << 60)) { *why = "dsp_pitch_shift_plan: L > 2^60"; return 2; }
    const double rate = (double)pl->q / (double)pl->p;
    pl->stretch = dsp_stretch_spec{rate, kStftCxN, H, window, 1e-10};
    // one rounding rule for every caller: floor(x + 1 / 2) of the exact quotient L p / q
    typedef unsigned __int128 u128;
    const u128 num = (u128)L * pl->p * 2 + pl->q;
    pl->stretched = std::max<uint64_t>(1, (uint64_t)(num / (2 * (u128)pl->q)));
    StretchPlan sp;
    uint64_t Lp = std::max<uint64_t>(L, kStftCxN);
    if (int r = stretch_plan(Lp, C, &pl->stretch, &sp, why)) return r;
    if (sp.Lout_full < pl->stretched) {
        // Lout_full = N + (F' - 1) H grows by about H / rate per hop of padding: jump close, then step
        const uint64_t missing = pl->stretched - sp.Lout_full;
        const uint64_t hops = (uint64_t)((double)missing * rate / (double)H);
        Lp += (hops > 2 ? hops - 2 : 0) * H;
        for (;; Lp += H) {
            if (int r = stretch_plan(Lp, C, &pl->stretch, &sp, why)) return r;
            if (sp.Lout_full >= pl->stretched) break;
        }
    }
    pl->padded = Lp;
    return 0;
}

}  // namespace dspb
