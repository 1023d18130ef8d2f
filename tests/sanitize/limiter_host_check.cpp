// limiter_host_check.cpp -- dsp_limiter's host code under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program (no GPU, nothing loaded
// into another process) over limiter_plan / limiter_window / limiter_table /
// limiter_scratch_bytes at the spec's corners.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Idsp-bench_amd/csrc tests/sanitize/limiter_host_check.cpp \
//       dsp-bench_amd/csrc/limiter_host.cpp dsp-bench_amd/csrc/loudness_host.cpp \
//       dsp-bench_amd/csrc/host_tables.cpp -o limiter_host_check && ./limiter_host_check
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "limiter_host.hpp"

using namespace dspb;

static dsp_limiter_spec spec(float c, uint32_t A, double tau, uint32_t flags) {
    dsp_limiter_spec s{};
    s.ceiling = c, s.lookahead = A, s.release = tau, s.flags = flags;
    return s;
}

int main() {
    const char *why = nullptr;
    LimiterPlan p;
    // every corner that plans
    const uint32_t As[] = {0, 1, 7, 8, 63, 64, 1023, 1024};
    const double taus[] = {0.0, 1.0, 64.0, 4800.0, 4194304.0};
    const uint64_t lens[] = {0, 1, 2047, 2048, 2049, 1ull << 40};
    const uint32_t Cs[] = {1, 2, 16, 17, 33, 1000};
    for (uint32_t A : As)
        for (double tau : taus)
            for (uint64_t L : lens)
                for (uint32_t C : Cs)
                    for (uint32_t flags = 0; flags < 4; ++flags) {
                        const dsp_limiter_spec s = spec(0.5f, A, tau, flags);
                        if (limiter_plan(48000, L, C, &s, &p, &why)) return 10;
                        if (p.groups != ((flags & DSP_LIMITER_UNLINKED) ? C : 1u)) return 11;
                        if (p.oversample != ((flags & DSP_LIMITER_TRUE_PEAK) ? 4u : 1u)) return 12;
                        if (p.wpad % 8 || p.wpad < A + 1 || p.wpad > A + 8) return 13;
                        if (p.tiles != L / 2048 + (L % 2048 ? 1 : 0)) return 14;
                        if (p.rows == 0 || p.rows > 16 || p.rows > p.groups) return 15;
                        if ((tau == 0.0) != (p.rho == 0.f) || !(p.rho >= 0.f && p.rho < 1.f)) return 16;
                        if (p.scratch_bytes < p.tiles * 2048 * 4 * p.rows + 16) return 17;
                        std::vector<float> tab;
                        limiter_table(p, tab);  // exactly kLimTabWindow + wpad floats
                        if (tab.size() != kLimTabWindow + p.wpad) return 18;
                        double sum = 0.0;
                        for (uint32_t k = 0; k < p.wpad; ++k) {
                            const float w = tab[kLimTabWindow + k];
                            if (!(w >= 0.f) || (k > A && w != 0.f)) return 19;
                            sum += (double)w;
                        }
                        if (std::fabs(sum - 1.0) > (A + 1) * std::ldexp(1.0, -24)) return 20;
                        if (tab[0] != 1.f || tab[1] != p.rho || tab[kLimTabLane] != 1.f) return 21;
                        for (uint32_t k = 1; k < kLimTabWindow; ++k)
                            if (!(tab[k] >= 0.f && tab[k] <= 1.f)) return 22;
                    }
    // the window alone, into exactly A + 1 floats
    for (uint32_t A : As) {
        std::vector<float> w(A + 1);
        limiter_window(A, w.data());
        if (A == 0 && w[0] != 1.f) return 30;
        for (uint32_t k = 0; k <= A; ++k)
            if (w[k] != w[A - k] && std::fabs(w[k] - w[A - k]) > 1e-9f) return 31;  // symmetric
    }
    // the oversampling classes and the rates the meter refuses
    const dsp_limiter_spec tp = spec(1.f, 72, 4800.0, DSP_LIMITER_TRUE_PEAK), sp = spec(1.f, 72, 4800.0, 0);
    if (limiter_plan(96000, 10, 2, &tp, &p, &why) || p.oversample != 2) return 40;
    if (limiter_plan(192000, 10, 2, &tp, &p, &why) || p.oversample != 1) return 41;
    if (limiter_plan(7999, 10, 2, &tp, &p, &why) != 2 || !why) return 42;
    if (limiter_plan(384001, 10, 2, &tp, nullptr, nullptr) != 2) return 43;
    if (limiter_plan(0, 10, 2, &sp, &p, &why) || p.oversample != 1) return 44;  // the rate matters to the detector only
    // every refusal
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const dsp_limiter_spec bad[] = {spec(0.f, 1, 0, 0),      spec(-1.f, 1, 0, 0),       spec(inf, 1, 0, 0),
                                    spec(nan, 1, 0, 0),      spec(1.f, 1025, 0, 0),     spec(1.f, ~0u, 0, 0),
                                    spec(1.f, 1, 0.5, 0),    spec(1.f, 1, -1.0, 0),     spec(1.f, 1, 4194305.0, 0),
                                    spec(1.f, 1, (double)nan, 0), spec(1.f, 1, (double)inf, 0), spec(1.f, 1, 0, 4),
                                    spec(1.f, 1, 0, ~0u)};
    for (const dsp_limiter_spec &s : bad) {
        why = nullptr;
        if (limiter_plan(48000, 100, 2, &s, &p, &why) != 1 || !why) return 50;
    }
    if (limiter_plan(48000, 100, 0, &sp, &p, &why) != 1) return 51;
    if (limiter_plan(48000, 100, 2, nullptr, &p, &why) != 1) return 52;
    if (limiter_plan(48000, 100, 2, nullptr, nullptr, nullptr) != 1) return 53;
    // sizes that do not fit
    if (limiter_scratch_bytes(~0ull / 2048, 16, 2) != 0) return 60;
    if (limiter_plan(48000, ~0ull, 2, &sp, &p, &why) != 2) return 61;
    std::printf("limiter host check ok\n");
    return 0;
}
