// loudness_host_check.cpp -- dsp_loudness's host code under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program (no GPU, nothing loaded
// into another process) over loudness_plan / loudness_gate at edge sizes.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Idsp-bench_amd/csrc tests/sanitize/loudness_host_check.cpp \
//       dsp-bench_amd/csrc/loudness_host.cpp dsp-bench_amd/csrc/host_tables.cpp \
//       -o loudness_host_check && ./loudness_host_check
#include <cmath>
#include <cstdio>
#include <vector>

#include "loudness_host.hpp"

using namespace dspb;

// the gate over C rows of `hops` hops at one level; every field written
static int gate_ok(uint32_t C, uint64_t hops, uint32_t hop, double level, const float *weights) {
    std::vector<std::vector<double>> z(C, std::vector<double>(hops, level * hop));  // exactly hops doubles a row
    std::vector<const double *> rows(C);
    for (uint32_t c = 0; c < C; ++c) rows[c] = z[c].data();
    dsp_loudness_result r;
    r.sample_peak = 0.125, r.true_peak = 0.25;
    loudness_gate(rows.data(), C, hops, hop, weights, &r);
    if (r.sample_peak != 0.125 || r.true_peak != 0.25) return 1;
    if (r.blocks != (hops >= 4 ? hops - 3 : 0)) return 2;
    if (r.gated_blocks > r.blocks) return 3;
    if (std::isnan(r.integrated) || std::isnan(r.range) || std::isnan(r.momentary_max) ||
        std::isnan(r.short_term_max))
        return 4;
    if ((hops < 30) != (r.short_term_max == -HUGE_VAL) && level > 0.0) return 5;
    if (r.range < 0.0) return 6;
    return 0;
}

int main() {
    int r;
    // plans: both ends of the range, every oversampling class, lengths around a hop and a tile
    const uint32_t rates[] = {8000, 11025, 44100, 48000, 88199, 88200, 176399, 176400, 192000, 384000};
    for (uint32_t sr : rates) {
        const uint32_t hop = (sr + 5) / 10;
        const uint64_t lens[] = {0, 1, hop - 1, hop, 4ull * hop - 1, 4ull * hop, 2047, 2048, 2049, 1ull << 40, ~0ull};
        for (uint64_t L : lens) {
            LoudnessPlan p;
            const char *why = nullptr;
            if (loudness_plan(sr, L, &p, &why)) return 10;
            if (p.hop != hop || p.hops != L / hop) return 11;
            if (p.oversample != (sr < 88200 ? 4u : sr < 176400 ? 2u : 1u)) return 12;
            if (p.window == 0 || p.window > 192 || p.run < 8 * p.window) return 13;
            if (p.tiles != L / 2048 + (L % 2048 ? 1 : 0)) return 14;
            for (float v : p.kcoef)
                if (!std::isfinite(v)) return 15;
        }
        LoudnessPlan p;
        if (loudness_plan(sr, 1000, &p, nullptr)) return 16;  // a NULL reason
        if (loudness_plan(sr, 1000, nullptr, nullptr)) return 17;  // and a NULL plan
        std::printf("%u Hz: hop %u, oversample %u, window %u tiles, run %u tiles ok\n", sr, p.hop, p.oversample,
                    p.window, p.run);
    }
    const char *why = nullptr;
    LoudnessPlan p;
    if (loudness_plan(7999, 1, &p, &why) != 2 || !why) return 20;
    if (loudness_plan(384001, 1, &p, &why) != 2) return 21;
    if (loudness_plan(0, 1, nullptr, nullptr) != 2) return 22;
    if (loudness_plan(~0u, 1, &p, &why) != 2) return 23;

    // the gate: no block, one block, just below and at a short-term block, many
    const float w3[3] = {1.f, 0.f, 1.41f};
    const uint64_t hops[] = {0, 1, 3, 4, 5, 29, 30, 31, 33, 1000};
    for (uint64_t h : hops) {
        if ((r = gate_ok(1, h, 4800, 0.01, nullptr))) return 30 + r;
        if ((r = gate_ok(3, h, 800, 0.01, w3))) return 40 + r;
        if ((r = gate_ok(2, h, 38400, 0.0, nullptr))) return 50 + r;     // silence: log of 0 never taken
        if ((r = gate_ok(17, h, 4410, 1e-9, nullptr))) return 60 + r;    // below the absolute gate
    }
    // hops = 0 with no rows at all
    dsp_loudness_result res;
    loudness_gate(nullptr, 1, 0, 4800, nullptr, &res);
    if (res.blocks != 0 || res.integrated != -HUGE_VAL || res.range != 0.0) return 70;
    std::printf("loudness host check ok\n");
    return 0;
}
