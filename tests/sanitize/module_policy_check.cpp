// module_policy_check.cpp -- csrc/module_policy.cpp driven on the CPU: every
// rule of the speculative segments' learner, the level / geometry planning,
// the block-class probes and classifier, and affine_ramp.  Prints `name value`
// lines; tests/test_module_policy.py builds it with g++ alone (plain, and with
// -fsanitize=address,undefined -fno-sanitize-recover=all), runs it and asserts
// the values:
//   g++ -std=c++17 -Iinclude -Idsp-bench_amd/csrc tests/sanitize/module_policy_check.cpp
//       dsp-bench_amd/csrc/module_policy.cpp
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "module_policy.hpp"

using namespace dspb;

namespace {

const unsigned char kP1[4] = {1, 2, 3, 4}, kP2[4] = {1, 2, 3, 5};
constexpr uint64_t kK = 1024, kSeg = 8;  // 1024 segments of 8 blocks

struct Stats {
    unsigned w[DSPB_STAT_PINNED] = {};
    Stats &set(unsigned slot, unsigned v) {
        w[slot] = v;
        return *this;
    }
};

SegLearner fresh() {
    SegLearner T;
    T.begin(kP1, 4, 2, 512);
    return T;
}
// one render: launched into the learner's slot with `levels` levels (0: the
// State chain alone), its counters landed at once
int render(SegLearner &T, uint32_t levels, const Stats &st) {
    const int slot = T.slot();
    T.launched(slot, kK, kSeg, levels, levels == 0, false);
    T.landed(slot, st.w);
    return slot;
}
void show(const char *tag, const SegLearner &T) {
    std::printf("%s_warm %u\n%s_one_level %d\n%s_off %d\n%s_chain_bad %d\n%s_bumps %u\n", tag, T.warm, tag,
                (int)T.one_level, tag, (int)T.off, tag, (int)T.chain_bad, tag, T.bumps);
    std::printf("%s_last_levels %u\n%s_last_warmup %u\n%s_last_chain %u\n%s_last_used %u\n", tag, T.last.levels, tag,
                T.last.warmup_blocks, tag, T.last.chain, tag, T.last.used);
}
Stats stats_a() { return Stats(); }  // LEVEL_RAN[1] = 0, LEVEL_DIFFERED[0] = 0
Stats stats_b() { return Stats().set(DSPB_STAT_LEVEL_RAN + 1, 1).set(DSPB_STAT_LEVEL_DIFFERED + 1, 10); }

void learner() {
    {
        SegLearner T = fresh();
        std::printf("begin_warm %u\nbegin_gen %llu\n", T.warm, (unsigned long long)T.gen);
        render(T, 3, stats_a());
        show("A", T);
    }
    {
        SegLearner T = fresh();
        render(T, 3, stats_b());
        show("B", T);
    }
    {
        SegLearner T = fresh();
        render(T, 3, Stats().set(DSPB_STAT_LEVEL_RAN + 1, 1).set(DSPB_STAT_LEVEL_RAN + 2, 1)
                         .set(DSPB_STAT_LEVEL_DIFFERED + 2, 200));
        show("C", T);
    }
    {   // D: after A, three renders under one_level whose few misses took a rerun
        SegLearner T = fresh();
        render(T, 3, stats_a());
        const Stats miss = Stats().set(DSPB_STAT_LEVEL_DIFFERED, 3);
        for (int i = 0; i < 3; ++i) {
            uint32_t lw[kSegLevels] = {};
            const uint32_t levels = T.levels(kK * kSeg, kSeg, false, lw);
            const int slot = render(T, levels, miss);
            std::printf("D%d_levels %u\nD%d_slot_one %d\nD%d_warm %u\n", i, levels, i, (int)T.slot_one[slot], i, T.warm);
        }
        show("D", T);
        // two renders launched with warm 4; the second lands after the first made it 5
        SegLearner U = fresh();
        render(U, 3, stats_a());
        const int s0 = U.slot();
        U.launched(s0, kK, kSeg, 2, false, false);
        const int s1 = U.slot();
        U.launched(s1, kK, kSeg, 2, false, false);
        U.landed(s0, miss.w);
        std::printf("Dstale_first_warm %u\n", U.warm);
        U.landed(s1, miss.w);
        std::printf("Dstale_warm %u\nDstale_bumps %u\nDstale_last_warmup %u\n", U.warm, U.bumps, U.last.warmup_blocks);
    }
    {   // E: a one_level render whose second level ran
        SegLearner T = fresh();
        render(T, 3, stats_a());
        render(T, 2, Stats().set(DSPB_STAT_LEVEL_RAN + 1, 1));
        show("E", T);
    }
    {   // F: other Parameters between a launch and its landing
        SegLearner T = fresh();
        const int slot = T.slot();
        T.launched(slot, kK, kSeg, 3, false, false);
        const uint64_t gen = T.gen;
        T.begin(kP2, 4, 2, 512);
        std::printf("F_gen_bumped %d\n", (int)(T.gen == gen + 1));
        T.landed(slot, stats_b().w);
        show("F", T);
        SegLearner S = fresh();
        render(S, 3, stats_a());
        const uint64_t g0 = S.gen;
        S.begin(kP1, 4, 2, 512);
        std::printf("Fsame_one_level %d\nFsame_gen_kept %d\n", (int)S.one_level, (int)(S.gen == g0));
        S.begin(kP1, 4, 1, 512);
        std::printf("FC_one_level %d\nFC_gen_bumped %d\nFC_warm %u\n", (int)S.one_level, (int)(S.gen == g0 + 1), S.warm);
        render(S, 3, stats_a());
        S.begin(kP1, 4, 1, 256);
        std::printf("FB_one_level %d\nFB_gen_bumped %d\n", (int)S.one_level, (int)(S.gen == g0 + 2));
        render(S, 3, stats_a());
        S.begin(kP1, 3, 1, 256);  // a shorter blob
        std::printf("Fsize_gen_bumped %d\n", (int)(S.gen == g0 + 3));
    }
    {   // G: the State chain alone, its records failing either check
        SegLearner T = fresh();
        render(T, 0, Stats().set(DSPB_STAT_CHAIN_MISMATCH, 1));
        show("Gm", T);
        SegLearner U = fresh();
        render(U, 0, Stats().set(DSPB_STAT_CHAIN_RECORDS, 1));
        show("Gr", U);
        SegLearner V = fresh();
        render(V, 0, Stats());
        show("Gok", V);
    }
    {   // H: slots and the order of landings
        SegLearner T = fresh();
        const int a = T.slot();
        T.launched(a, kK, kSeg, 3, false, false);
        const int b = T.slot();
        T.launched(b, kK, kSeg, 3, false, false);
        std::printf("H_slots %d%d\nH_order %d%d\n", a, b, T.slot(), 1 - T.slot());
        const int c = T.slot();
        T.landed(c, stats_a().w);
        T.launched(c, kK, kSeg, 3, false, false);
        std::printf("H_third %d\nH_order_after %d%d\nH_pending %d%d\n", c, T.slot(), 1 - T.slot(), (int)T.pending[0],
                    (int)T.pending[1]);
    }
}

void show_levels(const char *tag, uint32_t warm, uint64_t nblocks, uint64_t seg, bool has_chain, bool one_level) {
    SegLearner T = fresh();
    T.warm = warm;
    T.one_level = one_level;
    uint32_t lw[kSegLevels] = {};
    const uint32_t n = T.levels(nblocks, seg, has_chain, lw);
    std::printf("%s", tag);
    for (uint32_t i = 0; i < n; ++i) std::printf("%s%u", i ? "," : " ", lw[i]);
    std::printf("\n");
}
void show_geometry(const char *tag, uint64_t nblocks, uint64_t lanes, uint64_t state_size) {
    uint64_t seg = 0, K = 0;
    const bool ok = SegLearner::geometry(nblocks, lanes, state_size, &seg, &K);
    std::printf("%s_ok %d\n%s_seg %llu\n%s_K %llu\n", tag, (int)ok, tag, (unsigned long long)seg, tag,
                (unsigned long long)K);
}
void planning() {
    show_levels("levels_long", 4, 100000, 8, false, false);
    show_levels("levels_long_one", 4, 100000, 8, false, true);
    show_levels("levels_chain", 4, 10000, 8, true, false);
    show_levels("levels_short", 4, 100, 8, false, false);
    show_levels("levels_max", 4096, 1000000, 8, false, false);
    show_geometry("geo_min_seg", 100, 1000, 16);
    show_geometry("geo_large", 1000000, 1000, 16);
    show_geometry("geo_one_segment", 4, 1000, 16);
    show_geometry("geo_2p32", 1ull << 32, 1ull << 20, 1);
    show_geometry("geo_below_2p32", (1ull << 32) - 1, 1ull << 20, 1);
    show_geometry("geo_8gib", 8ull << 20, 1ull << 16, 1024);
    show_geometry("geo_over_8gib", (8ull << 20) + 1, 1ull << 16, 1024);
}

void classifier() {
    constexpr uint32_t C = 2, B = 8;
    constexpr uint64_t n = C * B;
    const std::vector<float> h = make_probes(C, B);
    std::printf("probes_size %zu\n", h.size());
    int zeros = 0, firsts = 0;
    for (uint64_t i = n; i < 3 * n; ++i) zeros += h[i] == 0.f;
    for (uint32_t c = 0; c < C; ++c) firsts += same_bits(h[n + (uint64_t)c * B], 1.0f);
    std::printf("probes_zeros_in_noise %d\nprobes_first_is_one %d\nprobes_negative_zero %d\nprobes_zero_probe %d\n"
                "probes_ones_probe %d\n",
                zeros, firsts, (int)same_bits(h[3 * n + 1], -0.0f), (int)same_bits(h[0], 0.f),
                (int)same_bits(h[4 * n + n - 1], 1.0f));
    auto kind = [&](const std::vector<float> &r, bool t, bool g, bool gt, bool have, float gv, float *gain) {
        const BlockClass c = classify(h.data(), r.data(), C, B, t, g, gt, have, gv);
        if (gain) *gain = c.gain;
        return (int)c.kind;
    };
    std::vector<float> r(h.size());
    for (uint64_t i = 0; i < r.size(); ++i) r[i] = 1.0f + 0.25f * (float)(i % B);  // one row, every channel and probe
    std::printf("class_table %d\nclass_table_not_proved %d\n", kind(r, true, false, false, false, 0.f, nullptr),
                kind(r, false, false, false, false, 0.f, nullptr));
    r[n + B + 3] += 1.0f;  // probe 1, channel 1
    std::printf("class_table_channel_differs %d\n", kind(r, true, false, false, false, 0.f, nullptr));
    float gain = 0.f;
    for (uint64_t i = 0; i < r.size(); ++i) r[i] = h[i] * 0.5f;
    std::printf("class_gain %d\n", kind(r, false, true, false, true, 0.5f, &gain));
    std::printf("class_gain_value %.9g\nclass_gain_no_g %d\n", gain, kind(r, false, true, false, false, 0.5f, nullptr));
    std::printf("class_gain_table_allowed %d\n", kind(r, true, true, false, true, 0.5f, nullptr));
    r[4 * n + 5] = 0.25f;  // the ones probe: one element scaled twice
    std::printf("class_gain_twice %d\n", kind(r, false, true, false, true, 0.5f, nullptr));
    for (uint64_t i = 0; i < r.size(); ++i) r[i] = h[i] * (0.5f + 0.125f * (float)(i % n));
    std::printf("class_gain_table %d\nclass_gain_table_not_proved %d\n", kind(r, false, true, true, true, 0.5f, nullptr),
                kind(r, false, true, false, true, 0.5f, nullptr));
    for (float &v : r) v = 0.f;  // zeros: a table, and x * 0 -- the table comes first
    std::printf("class_zero_block %d\n", kind(r, true, true, true, true, 0.f, nullptr));
}

void ramps() {
    constexpr uint32_t B = 512;
    const float g0 = 0.9f, s = 0.002f;
    std::vector<float> t(B);
    for (uint32_t i = 0; i < B; ++i) t[i] = (float)std::fma(-(double)i, (double)s, (double)g0);
    double rg = -1, rs = -1;
    std::printf("ramp_found %d\n", (int)affine_ramp(t.data(), B, &rg, &rs));
    std::printf("ramp_g0_exact %d\nramp_s_exact %d\n", (int)(rg == (double)g0), (int)(rs == (double)s));
    t[200] = std::nextafterf(t[200], 2.f);
    std::printf("ramp_one_ulp_off %d\n", (int)affine_ramp(t.data(), B, &rg, &rs));
    // multiples of a subnormal step: affine bit for bit, but not taken
    const float tiny = 1e-41f;
    std::vector<float> u(8);
    for (uint32_t i = 0; i < 8; ++i) u[i] = (float)std::fma(-(double)i, -(double)tiny, 0.0);
    std::printf("ramp_subnormal_input %d\nramp_subnormal %d\n", (int)(u[3] != 0.f && std::fabs(u[3]) < 1.17549435e-38f),
                (int)affine_ramp(u.data(), 8, &rg, &rs));
    const float one[1] = {0.75f};
    rg = rs = -1;
    std::printf("ramp_b1 %d\n", (int)affine_ramp(one, 1, &rg, &rs));
    std::printf("ramp_b1_g0 %.9g\nramp_b1_s %.9g\n", rg, rs);
    const float inf[2] = {INFINITY, 0.f};
    std::printf("ramp_inf %d\n", (int)affine_ramp(inf, 2, &rg, &rs));
}

}  // namespace

int main() {
    learner();
    planning();
    classifier();
    ramps();
    return 0;
}
