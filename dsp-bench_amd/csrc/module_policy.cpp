// module_policy.cpp -- the segment learner and the block-class classifier of
// the plugin module host (module_policy.hpp): host arithmetic only, no HIP.
#include "module_policy.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

namespace dspb {

void SegLearner::begin(const void *blob, uint32_t blob_size, uint32_t C_, uint32_t B_) {
    const unsigned char *pb = (const unsigned char *)blob;
    if (warm && C == C_ && B == B_ && params.size() == blob_size &&
        !(blob_size && std::memcmp(params.data(), pb, blob_size)))
        return;
    params.assign(pb, pb + blob_size);
    C = C_, B = B_;
    warm = kSegWarm0;
    off = chain_bad = one_level = false;
    bumps = 0;
    ++gen;
}

bool SegLearner::geometry(uint64_t nblocks, uint64_t lanes, uint64_t state_size, uint64_t *seg, uint64_t *K) {
    *seg = std::max<uint64_t>((nblocks + lanes - 1) / lanes, kSegMinBlocks);
    *K = (nblocks + *seg - 1) / *seg;
    return !(*K < 2 || nblocks >= (1ull << 32) || nblocks * state_size > (8ull << 30));
}

uint32_t SegLearner::levels(uint64_t nblocks, uint64_t seg, bool has_chain, uint32_t (&lw)[kSegLevels]) const {
    uint32_t nlev = 0;
    for (uint32_t L = 0, w = warm; L < kSegLevels; ++L) {
        if (L > 0) {
            const uint32_t next = std::min<uint32_t>(w * 16, kSegWarmMax);
            if (next <= w || 2ull * next >= nblocks) break;  // no longer, or as long as the file
            // with a State chain to fall back on, a level whose rounds (its
            // warm-up and a segment of full callbacks) exceed 1/16 of the
            // file costs more than the chain (the State arithmetic alone over
            // every block) is likely to: not tried
            if (has_chain && 16ull * (next + seg) > nblocks) break;
            w = next;
        }
        lw[nlev++] = w;
    }
    // learnt: the first level meets the State (the later ones would only
    // return at once, a launch each of pass 1, its check and the split
    // chain): the first two levels alone -- the second one is there for
    // a render whose input keeps the first from meeting the State (it
    // unlearns this; without it such a render fell to the reruns and the
    // walk's serial chain, 465 segments of a 20 s peak follower)
    return one_level ? std::min<uint32_t>(nlev, 2) : nlev;
}

void SegLearner::launched(int slot, uint64_t K, uint64_t seg, uint32_t nlevels, bool chain, bool split) {
    pending[slot] = true;
    seq[slot] = ++calls;
    slot_gen[slot] = gen;
    slot_one[slot] = !chain && one_level;  // the levels were cut to the first two
    dsp_state_spec_info &r = info[slot];
    r = dsp_state_spec_info{};
    r.used = 1;
    r.segments = (uint32_t)K;
    r.blocks_per_segment = (uint32_t)seg;
    r.warmup_blocks = chain ? 0 : warm;  // the first level's; landed() names the one that stood
    r.levels = nlevels;                  // 0: the learnt State chain alone
    r.chain = chain ? 1 : 0;
    r.split = split ? 1 : 0;
}

void SegLearner::landed(int i, const unsigned *h) {
    pending[i] = false;
    dsp_state_spec_info &r = info[i];
    const uint32_t first_warm = r.warmup_blocks;
    const bool spec = r.levels > 0;  // a speculative render (else the learnt State chain alone)
    uint32_t stood = 0, w = first_warm;
    for (uint32_t L = 1; L < r.levels && h[DSPB_STAT_LEVEL_RAN + L]; ++L) {
        stood = L;
        w = std::min<uint32_t>(w * 16, kSegWarmMax);
    }
    if (spec) {
        r.levels = stood + 1;
        r.warmup_blocks = w;
        r.differed[0] = h[DSPB_STAT_LEVEL_DIFFERED + stood];
        r.differed[1] = h[DSPB_STAT_RERUN_DIFFERED];
        r.differed[2] = h[DSPB_STAT_RERUN_DIFFERED + 1];
    }
    r.serial_reruns = h[DSPB_STAT_WALK_RERUNS];
    r.chain = (h[DSPB_STAT_CHAINED] || !spec) ? 1 : 0;
    r.chain_mismatch = h[DSPB_STAT_CHAIN_MISMATCH];
    r.chain_records_differed = h[DSPB_STAT_CHAIN_RECORDS];
    // (split: set at launch, kept)
    if (seq[i] == calls) last = r;
    if (slot_gen[i] != gen) return;  // rendered with other Parameters: nothing to learn
    // the chain's records failed their check (the walk rendered the call
    // right): these Parameters render serially from now on
    if (r.chain && (r.chain_mismatch || r.chain_records_differed)) off = chain_bad = true;
    // learn only from renders that started with the warm-up now in force
    if (!spec || first_warm != warm || off) return;
    const uint64_t early = std::min<uint64_t>(r.segments - 1, w / r.blocks_per_segment);
    const uint64_t guessed = r.segments - 1 - early;
    const bool failed = guessed && r.differed[0] * 8ull > guessed;
    if (slot_one[i]) {  // launched with the first two levels alone
        if (failed || r.levels > 1) {
            one_level = false;  // every level again from the next call
        } else if (r.differed[0] && bumps < kSegWarmBumps) {
            // a few segments missed and took a rerun (its rounds cost more
            // than one more warm-up round for all): one block longer
            warm += 1;
            ++bumps;
        }
        return;
    }
    if (failed) {
        off = true;  // the longest warm-up it could try failed
    } else {
        warm = w;
        one_level = r.levels == 1;  // the first level sufficed
    }
}

// ---- block classes ----------------------------------------------------------
static uint32_t xorshift(uint32_t &x) {
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    return x;
}

bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

std::vector<float> make_probes(uint32_t C, uint32_t B) {
    const uint64_t n = (uint64_t)C * B;
    std::vector<float> h((size_t)(kProbes * n), 0.f);
    uint32_t seed = 0x9e3779b9u;
    for (uint64_t i = 0; i < n; ++i) {
        // (xorshift32 never yields 0, so no noise element is 0: probes 0 and
        // 1 differ in every element)
        h[n + i] = (float)((int32_t)xorshift(seed)) * (1.0f / 2147483648.0f);
        h[2 * n + i] = (float)((int32_t)xorshift(seed)) * (1000.0f / 2147483648.0f);
        h[3 * n + i] = (float)((int)(i % 13) - 6) * 0.125f;
        h[4 * n + i] = 1.0f;
    }
    for (uint32_t c = 0; c < C; ++c) h[n + (uint64_t)c * B] = 1.0f;
    h[3 * n + (B > 1 ? 1 : 0)] = -0.0f;
    return h;
}

BlockClass classify(const float *h, const float *r, uint32_t C, uint32_t B, bool may_table, bool may_gain,
                    bool may_gtab, bool have_g, float g) {
    const uint64_t n = (uint64_t)C * B;
    bool table = may_table;
    for (uint64_t i = 0; i < kProbes * n && table; ++i) table = same_bits(r[i], r[i % B]);
    bool gain = !table && may_gain && have_g && std::isfinite(g);
    for (uint64_t i = 4 * n; i < 5 * n && gain; ++i) gain = same_bits(r[i], g);  // ones -> g, every element
    for (uint64_t i = 0; i < kProbes * n && gain; ++i) gain = same_bits(r[i], h[i] * g);
    // a gain table (IR: every store x G at x's address, G free of samples,
    // each element stored at most once): G[c][s] is what the probe of ones
    // renders (fl(1 G) = G; 1 where nothing is stored), and every probe must
    // render fl(x G) element by element
    bool gtab = !table && !gain && may_gtab;
    for (uint64_t i = 0; i < kProbes * n && gtab; ++i) gtab = same_bits(r[i], h[i] * r[4 * n + i % n]);
    BlockClass c;
    if (table) c.kind = kBlockTable;
    else if (gain) c.kind = kBlockGain, c.gain = g;
    else if (gtab) c.kind = kBlockGainTable;
    return c;
}

// Is the callback's block t[0, B) an f64 ramp rounded to f32 -- t[i] =
// (float)fma(-i, s, g0), the closed form common.hpp ramp_value evaluates --
// for some (g0, s)?  IR_test.cpp (build/IR_test.cpp:47-58: `gain -= step` in
// double from float Parameters) gives one whenever its recurrence is exact.
// Candidates: g0 = t[0]; s = the float nearest the end-to-end slope and its
// neighbours (a float Parameter widened to double), then the slope itself.
// Only a candidate that reproduces all B values bit for bit is taken, so the
// closed form renders exactly the callback's block.
bool affine_ramp(const float *t, uint32_t B, double *g0, double *s) {
    const double a = t[0];
    auto fits = [&](double sc) {
        for (uint32_t i = 0; i < B; ++i)
            if (!same_bits((float)std::fma(-(double)i, sc, a), t[i])) return false;
        return true;
    };
    if (!std::isfinite(a)) return false;
    // (a subnormal value keeps the table: the device's f64 -> f32 conversion
    // is not checked against the host's there)
    for (uint32_t i = 0; i < B; ++i)
        if (t[i] != 0.f && std::fabs(t[i]) < FLT_MIN) return false;
    if (B == 1) {
        *g0 = a;
        *s = 0.0;
        return true;
    }
    const double slope = (a - (double)t[B - 1]) / (double)(B - 1);
    if (!std::isfinite(slope)) return false;
    std::vector<double> cand;
    const float sf = (float)slope;
    cand.push_back(sf);
    float up = sf, dn = sf;
    for (int k = 0; k < 8; ++k) {
        up = std::nextafter(up, INFINITY);
        dn = std::nextafter(dn, -INFINITY);
        cand.push_back(up);
        cand.push_back(dn);
    }
    cand.push_back(slope);
    for (double sc : cand)
        if (fits(sc)) {
            *g0 = a;
            *s = sc;
            return true;
        }
    return false;
}

}  // namespace dspb
