// pvoc_host_check.cpp -- a stand-alone program over the host half of dsp_pvoc,
// dsp_time_stretch and dsp_pitch_ratio (pvoc_host.cpp), compiled by
// tests/test_pvoc_host.py with -fsanitize=address,undefined: the output frame
// count, the chunk ranges and the scratch sizes at the extremes (F = 1,
// F = 2^32 + 1, F = 2^48, both ends of the rate range, C = 1, 16 and 17), the
// composite's plan and every pitch ratio.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "pvoc_host.hpp"

using namespace dspb;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static void walk(uint64_t F, double rate, uint32_t C) {
    const char *why = nullptr;
    dsp_pvoc_spec sp{rate};
    PvocPlan p;
    CHECK(pvoc_plan(F, C, &sp, &p, &why) == 0);
    // F' is the count: the last frame reads inside, the next one does not
    CHECK(p.frames_out >= 1);
    CHECK(pvoc_position(p.frames_out - 1, rate) < (double)F);
    CHECK(!(pvoc_position(p.frames_out, rate) < (double)F));
    CHECK(p.rows == (C < 16 ? C : 16) && p.chunk == kPvocChunk);
    CHECK(p.chunks == (p.frames_out + p.chunk - 1) / p.chunk);
    CHECK(p.scratch_bytes == (uint64_t)p.rows * p.chunks * 4097 * 4);
    // the chunks tile [0, F'): the first ones, the last ones, and nothing past them
    uint64_t next = 0;
    const uint64_t head = p.chunks < 1000 ? p.chunks : 1000;
    for (uint64_t c = 0; c < head; ++c) {
        const PvocChunk ch = pvoc_chunk(p, c);
        CHECK(ch.t0 == next && ch.t1 > ch.t0 && ch.t1 - ch.t0 <= p.chunk && ch.t1 <= p.frames_out);
        next = ch.t1;
    }
    const PvocChunk last = pvoc_chunk(p, p.chunks - 1);
    CHECK(last.t1 == p.frames_out && last.t0 == (p.chunks - 1) * p.chunk);
    const PvocChunk past = pvoc_chunk(p, p.chunks);
    CHECK(past.t0 == 0 && past.t1 == 0);
    // a row of F frames of ld floats must fit 2^61 floats
    CHECK(pvoc_check_ld(F, 8194, &why) == (F > (UINT64_MAX >> 3) / 8194 ? 2 : 0));
    CHECK(pvoc_check_ld(p.frames_out, 8200, &why) == (p.frames_out > (UINT64_MAX >> 3) / 8200 ? 2 : 0));
}

int main() {
    const char *why = nullptr;
    const uint64_t Fs[] = {1, 2, 63, 64, 65, 4097, (1ull << 32) + 1, 1ull << 48};
    const double rates[] = {0.125, 0.3, 0.5, 0.8, 1.0, 1.2599, 3.0, 8.0};
    const uint32_t Cs[] = {1, 16, 17};
    for (uint64_t F : Fs)
        for (double r : rates)
            for (uint32_t C : Cs) walk(F, r, C);

    PvocPlan p;
    dsp_pvoc_spec bad{0.1249};
    CHECK(pvoc_plan(5, 1, &bad, &p, &why) == 1);
    bad.rate = 8.0001;
    CHECK(pvoc_plan(5, 1, &bad, &p, &why) == 1);
    bad.rate = std::nan("");
    CHECK(pvoc_plan(5, 1, &bad, &p, &why) == 1);
    bad.rate = INFINITY;
    CHECK(pvoc_plan(5, 1, &bad, &p, &why) == 1);
    bad.rate = 1.0;
    CHECK(pvoc_plan(0, 1, &bad, &p, &why) == 1 && pvoc_plan(5, 0, &bad, &p, &why) == 1);
    CHECK(pvoc_plan(5, 1, nullptr, &p, &why) == 1);
    CHECK(pvoc_plan((1ull << 48) + 1, 1, &bad, &p, &why) == 2);
    CHECK(pvoc_check_ld(5, 8193, &why) == 1 && pvoc_check_ld(5, 8192, &why) == 1 && pvoc_check_ld(5, 0, &why) == 1);
    CHECK(pvoc_check_ld(1ull << 48, 1ull << 20, &why) == 2);

    // the composite: an hour of 48 kHz, and the extremes of L
    StretchPlan s;
    dsp_stretch_spec ss{0.8, 8192, 2048, DSP_WIN_HANN, 1e-10};
    CHECK(stretch_plan(48000ull * 3600, 2, &ss, &s, &why) == 0);
    CHECK(s.frames_in == (48000ull * 3600 - 8192) / 2048 + 1 && s.rows == 2 && s.ld == 8194);
    CHECK(s.Lout_full == 8192 + (s.frames_out - 1) * 2048);
    CHECK(s.Lout_default == (s.Lout_full < 216000000 ? s.Lout_full : 216000000));
    CHECK(s.device_bytes == 2 * (s.frames_in + s.frames_out) * 8194 * 4);
    CHECK(stretch_plan(8192, 17, &ss, &s, &why) == 0 && s.frames_in == 1 && s.frames_out == 2 && s.rows == 16);
    CHECK(stretch_plan(8191, 1, &ss, &s, &why) == 1);
    CHECK(stretch_plan(UINT64_MAX, 1, &ss, &s, &why) != 0);
    ss.H = 511;
    CHECK(stretch_plan(100000, 1, &ss, &s, &why) == 2);
    ss.H = 512, ss.rate = 8.0;
    CHECK(stretch_plan(100000, 1, &ss, &s, &why) == 0 && s.Lout_default == 12500);
    ss.rate = 0.125;
    CHECK(stretch_plan((1ull << 48) * 512, 40, &ss, &s, &why) == 0 || why != nullptr);
    CHECK(stretch_plan(100000, 1, nullptr, &s, &why) == 1);

    // every ratio is in range and within 1 / (q 4096) of the target
    for (int i = -2400; i <= 2400; ++i) {
        uint32_t a = 0, b = 0;
        const double st = i / 100.0;
        CHECK(pitch_ratio(st, &a, &b, &why) == 0);
        CHECK(a >= 1 && a <= 4096 && b >= 1 && b <= 4096);
        const double x = std::exp2(st / 12.0);
        CHECK(std::fabs((double)a / b - x) <= x / 4096.0);
    }
    uint32_t a, b;
    CHECK(pitch_ratio(0.0, &a, &b, &why) == 0 && a == 1 && b == 1);
    CHECK(pitch_ratio(12.0, &a, &b, &why) == 0 && a == 2 && b == 1);
    CHECK(pitch_ratio(-24.0, &a, &b, &why) == 0 && a == 1 && b == 4);
    CHECK(pitch_ratio(24.01, &a, &b, &why) == 1 && pitch_ratio(std::nan(""), &a, &b, &why) == 1);
    CHECK(pitch_ratio(3.0, nullptr, nullptr, &why) == 0);

    // the pitch plan: the exact rounded quotient, the least padding, at the extremes of L
    PitchPlan pp;
    const uint64_t Ls[] = {1, 8191, 8192, 24577, 48000ull * 3600, 1ull << 40};
    const double sts[] = {-24.0, -12.0, -2.0, 0.0, 3.0, 12.0, 24.0};
    for (uint64_t L : Ls)
        for (double st : sts)
            for (uint32_t H : {512u, 2048u, 8192u}) {
                CHECK(pitch_plan(L, 2, st, H, DSP_WIN_HANN, &pp, &why) == 0);
                typedef unsigned __int128 u128;
                const uint64_t want = (uint64_t)(((u128)L * pp.p * 2 + pp.q) / (2 * (u128)pp.q));
                CHECK(pp.stretched == (want ? want : 1));
                const uint64_t base = L > 8192 ? L : 8192;
                CHECK(pp.padded >= base && (pp.padded - base) % H == 0);
                StretchPlan sp;
                CHECK(stretch_plan(pp.padded, 2, &pp.stretch, &sp, &why) == 0 && sp.Lout_full >= pp.stretched);
                if (pp.padded > base)
                    CHECK(stretch_plan(pp.padded - H, 2, &pp.stretch, &sp, &why) == 0 && sp.Lout_full < pp.stretched);
            }
    CHECK(pitch_plan(0, 1, 3.0, 2048, DSP_WIN_HANN, &pp, &why) == 1);
    CHECK(pitch_plan(100, 1, 25.0, 2048, DSP_WIN_HANN, &pp, &why) == 1);
    CHECK(pitch_plan(100, 1, 3.0, 100, DSP_WIN_HANN, &pp, &why) == 2);
    CHECK(pitch_plan((1ull << 60) + 1, 1, 3.0, 2048, DSP_WIN_HANN, &pp, &why) == 2);
    // the chunk override: inside 8..4096 it is taken, else the default
    dsp_pvoc_spec one{1.0};
    CHECK(pvoc_plan(1000, 1, &one, &p, &why, 128) == 0 && p.chunk == 128 && p.chunks == 8);
    CHECK(pvoc_plan(1000, 1, &one, &p, &why, 0) == 0 && p.chunk == 64);
    CHECK(pvoc_plan(1000, 1, &one, &p, &why, 5000) == 0 && p.chunk == 64);
    std::printf("pvoc host check ok\n");
    return 0;
}
