// module_policy.hpp -- the decisions of the plugin module host that need no
// device: what a speculative-segment render starts with and what its counters
// teach (SegLearner), and which block class a stateless callback's probe
// results show (make_probes / classify / affine_ramp).  Plain C++ over
// counters and float arrays, no HIP: tests/test_module_policy.py drives every
// rule on the CPU, once more under ASan + UBSan.  The module code
// (module_seg.cpp, module_spec.cpp) keeps the events, copies and launches.
#pragma once
#include <stdint.h>

#include <vector>

#include "dspbench/module.h"       // dsp_state_spec_info
#include "plugin_driver_host.hpp"  // DSPB_STAT_*, dspb_max_levels

namespace dspb {

constexpr uint32_t kSegWarm0 = 4;         // blocks of warm-up of a first render
constexpr uint32_t kSegWarmBumps = 2;     // at most this many blocks added for a few misses
constexpr uint32_t kSegWarmMax = 4096;    // the longest warm-up (blocks); past it, the chain is serial
constexpr uint32_t kSegLevels = dspb_max_levels;  // warm-up levels a render may try (x16 each)
constexpr uint32_t kSegMinBlocks = 4;     // blocks per segment at least

// What a module has learnt about the speculative renders of one (Parameters,
// C, B), and the book-keeping of the last two renders' counters: two slots,
// each filled at a launch and read when its counters have landed.  A render
// tries warm-up levels (x16 each, on the GPU) until no more than 1/8 of the
// segments it guessed started from a State that was not the true one; the
// level that stood is where the next render with these Parameters starts.
// When even the last level it could try failed (kSegWarmMax, or a warm-up
// half the file), the chain does not forget: these Parameters render from the
// State chain's records from now on, and serially once those fail their check.
struct SegLearner {
    uint32_t warm = 0;             // learned warm-up for `params` (0: not yet)
    bool off = false;              // learned: the chain does not forget its State
    bool chain_bad = false;        // learned: the State chain's records failed their check
    bool one_level = false;        // learned: the first warm-up level suffices (two levels launched)
    uint32_t bumps = 0;            // warm-up blocks added after renders whose few misses took a rerun
    uint64_t gen = 0;              // bumped when `params` change (learn only from renders with them)
    std::vector<unsigned char> params;
    uint32_t C = 0, B = 0;         // ... and the shape it was learnt with (kernels differ by shape)
    uint64_t calls = 0;
    uint64_t seq[2] = {};          // the call that filled the slot
    bool pending[2] = {};          // launched, counters not yet read
    uint64_t slot_gen[2] = {};
    bool slot_one[2] = {};         // the render in the slot was launched with the first two levels alone
    dsp_state_spec_info info[2] = {};
    dsp_state_spec_info last{};    // the newest render whose counters were read
    bool serial = false;           // the module's last State-writing render was the serial chain

    // a render with these Parameters and shape is about to be planned: new
    // Parameters, or a new shape (whether a State chain or a split State's
    // chain exists depends on it), learn again
    void begin(const void *blob, uint32_t blob_size, uint32_t C, uint32_t B);
    // segments over nblocks blocks: as many as the chip runs lanes at once,
    // kSegMinBlocks blocks at least.  false: the call does not fit (fewer than
    // two segments; block indices in 32 bits; one recorded State per block,
    // at most 8 GiB of them)
    static bool geometry(uint64_t nblocks, uint64_t lanes, uint64_t state_size, uint64_t *seg, uint64_t *K);
    // The warm-up of each level pass 1 may run: the learnt one, then 16x
    // longer ones while too many segments started wrong (each level decides on
    // the GPU whether it runs: dspb_seg_level_runs).  Returns how many.
    uint32_t levels(uint64_t nblocks, uint64_t seg, bool has_chain, uint32_t (&lw)[kSegLevels]) const;
    // the slot the next launch fills, the older one: the render two calls
    // back, whose counters have landed by now in a stream of back-to-back
    // calls.  Pending slots are read in the order slot(), 1 - slot().
    int slot() const { return seq[0] <= seq[1] ? 0 : 1; }
    // a render of K segments of `seg` blocks went into `slot`: `nlevels` from
    // levels(), or chain (the learnt State chain alone, no level)
    void launched(int slot, uint64_t K, uint64_t seg, uint32_t nlevels, bool chain, bool split);
    // the counters of the render in `slot` (dspb_stat, DSPB_STAT_PINNED
    // words): into info[slot] / last, and what they teach
    void landed(int slot, const unsigned *stats);
};

// ---- block classes (kernels.hpp ModuleSpec) ---------------------------------
constexpr int kProbes = 5;  // zeros, noise [-1, 1], noise [-1000, 1000], steps, ones
// the probe blocks, [kProbes][C][B]
std::vector<float> make_probes(uint32_t C, uint32_t B);

enum BlockKind : int { kBlockCallback = 0, kBlockTable = 1, kBlockGain = 2, kBlockGainTable = 3 };
struct BlockClass {
    BlockKind kind = kBlockCallback;
    float gain = 1.f;  // kBlockGain
};
// what the callback rendered over the probes (`results`, laid out as they
// are) shows, among the classes its IR allows (may_*); g is the gain's value
// from where the IR says the callback reads it (have_g: it could be read)
BlockClass classify(const float *probes, const float *results, uint32_t C, uint32_t B, bool may_table, bool may_gain,
                    bool may_gtab, bool have_g, float g);

bool same_bits(float a, float b);
// Is the block t[0, B) an f64 ramp rounded to f32, t[i] = (float)fma(-i, s, g0)?
bool affine_ramp(const float *t, uint32_t B, double *g0, double *s);

}  // namespace dspb
