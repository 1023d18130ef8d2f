// resample_host_check.cpp -- dsp_resample's host code under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program (no GPU, nothing loaded
// into another process) over resample_plan / resample_table at the extreme
// accepted plans and at the refusals.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Idsp-bench_amd/csrc tests/sanitize/resample_host_check.cpp \
//       dsp-bench_amd/csrc/host_tables.cpp -o resample_host_check && ./resample_host_check
#include <cmath>
#include <cstdio>
#include <vector>

#include "host_tables.hpp"

using namespace dspb;

static const double kBeta = 14.769656459379492, kRoll = 0.9475937167399596;

// the table into exactly up * taps floats; every value written, finite, |.| <= 1
static int table_ok(uint32_t sr_in, uint32_t sr_out, uint32_t zeros, double beta, double rolloff) {
    ResamplePlan p;
    const char *why = nullptr;
    if (resample_plan(sr_in, sr_out, 1000, zeros, beta, rolloff, &p, &why)) return 1;
    if (p.taps != 2 * p.half || p.table_bytes != (uint64_t)p.up * p.taps * 4) return 2;
    if (p.Lout != (1000ull * p.up + p.down - 1) / p.down) return 3;
    std::vector<float> t((size_t)p.up * p.taps, 7.f);
    resample_table(p, t.data(), p.taps, 0);
    for (float v : t)
        if (!std::isfinite(v) || v == 7.f || std::fabs(v) > 1.f) return 4;
    // the centre tap of phase 0 is h(0) = rho
    if (std::fabs(t[p.half - 1] - p.rho) > 1e-6) return 5;
    std::printf("%u -> %u Z=%u: up=%u down=%u taps=%u table=%llu bytes ok\n", sr_in, sr_out, zeros, p.up, p.down,
                p.taps, (unsigned long long)p.table_bytes);
    return 0;
}

int main() {
    int r;
    // the defaults; the most taps (8192: W = 4096 exactly); the most phases
    // (up = 4096); the largest table (4096 x 510 floats < 8 MiB); the spec's corners
    if ((r = table_ok(44100, 48000, 64, kBeta, kRoll))) return r;
    if ((r = table_ok(48000, 48000, 64, kBeta, kRoll))) return 10 + r;
    if ((r = table_ok(1024, 1, 4, 0.0, 1.0))) return 20 + r;
    if ((r = table_ok(4097, 4096, 64, 20.0, 0.5))) return 30 + r;
    if ((r = table_ok(15361, 4096, 64, kBeta, kRoll))) return 40 + r;
    if ((r = table_ok(192000, 8000, 64, kBeta, kRoll))) return 50 + r;
    ResamplePlan p;
    const char *why = nullptr;
    // rows at a stride with an offset (the caller's padding stays untouched)
    if (resample_plan(2, 3, 10, 4, 5.0, 0.9, &p, &why)) return 60;
    std::vector<float> t((size_t)p.up * (p.taps + 5), 7.f);
    resample_table(p, t.data(), p.taps + 5, 3);
    for (uint32_t phi = 0; phi < p.up; ++phi)
        for (uint32_t i = 0; i < p.taps + 5; ++i)
            if ((t[(size_t)phi * (p.taps + 5) + i] == 7.f) != (i < 3 || i >= 3 + p.taps)) return 61;
    // refusals: invalid (1) and unsupported (2), each with a reason; NULL plan and reason accepted
    if (resample_plan(0, 48000, 1, 64, kBeta, kRoll, &p, &why) != 1 || !why) return 70;
    if (resample_plan(48000, 0, 1, 64, kBeta, kRoll, nullptr, nullptr) != 1) return 71;
    if (resample_plan(1, 2, 1, 3, kBeta, kRoll, &p, &why) != 1) return 72;
    if (resample_plan(1, 2, 1, 65, kBeta, kRoll, &p, &why) != 1) return 73;
    if (resample_plan(1, 2, 1, 64, std::nan(""), kRoll, &p, &why) != 1) return 74;
    if (resample_plan(1, 2, 1, 64, 20.5, kRoll, &p, &why) != 1) return 75;
    if (resample_plan(1, 2, 1, 64, kBeta, 0.4, &p, &why) != 1) return 76;
    if (resample_plan(4099, 4097, 1, 64, kBeta, kRoll, &p, &why) != 2) return 77;     // up
    if (resample_plan(192000, 1000, 1, 64, kBeta, kRoll, &p, &why) != 2) return 78;   // taps
    if (resample_plan(4294967295u, 1, 1, 4, kBeta, 1.0, &p, &why) != 2) return 79;    // taps, the largest down
    if (resample_plan(16385, 4096, 1, 64, kBeta, kRoll, &p, &why) != 2) return 80;    // table
    if (resample_plan(44100, 48000, 1ull << 62, 64, kBeta, kRoll, &p, &why) != 2) return 81;  // L up
    if (resample_plan(1, 4096, ~0ull, 64, kBeta, kRoll, &p, &why) != 2) return 82;
    if (resample_plan(44100, 48000, ((1ull << 63) - 147) / 160, 64, kBeta, kRoll, &p, &why) != 0) return 83;
    std::printf("resample host check ok\n");
    return 0;
}
