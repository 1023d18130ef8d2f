// module_impl.hpp -- what the pieces of the plugin module host share
// (module.cpp: compile, analysis, facts; module_load.cpp: load, State,
// Parameters, the render dispatch; module_seg.cpp: speculative segments;
// module_spec.cpp: block classes): dsp_module, the kernel shape tables and
// the few helpers more than one piece calls.  Private to those files.
#pragma once
#include <hip/hip_runtime.h>

#include <iterator>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "descriptor.hpp"
#include "host_hip.hpp"
#include "ir_proof.hpp"
#include "dspbench/module.h"
#include "kernels.hpp"
#include "module_policy.hpp"  // SegLearner; the contract with the driver kernels (plugin_driver_host.hpp)

namespace dspb {

static_assert(dspb_max_channels == (unsigned)kMaxChannels, "one channel bound");

constexpr uint64_t kStagedLdsBytes = 64 * 1024;  // stateful render's LDS double-buffer limit
constexpr uint32_t kSegMaxState = 1024;          // bytes of State a lane copies (the walk keeps one in LDS)

// a kernel of the driver and the shape it is compiled for: (C, B) = 0 matches
// any value; the tables list the most specific first
struct Shape {
    const char *name;
    uint32_t C, B;
    const char *rerun;  // segments: the reruns' kernel (NULL: the same one)
    bool pf;            // segments: blocks at dspb_stride_pf, and 4 | B
};
#define DSPB_SHAPE(name, C, B) {#name, C, B, nullptr, false},
#define DSPB_SEG_PF_roles true
#define DSPB_SEG_PF_pf true
#define DSPB_SEG_PF_any false
#define DSPB_SEG_RERUN_pf(name) #name "_rerun"
#define DSPB_SEG_RERUN_same(name) nullptr
#define DSPB_SEG_SHAPE(name, C, B, P1, RR) {#name, C, B, DSPB_SEG_RERUN_##RR(name), DSPB_SEG_PF_##P1},
constexpr Shape kLdsShapes[] = {DSPB_LDS_KERNELS(DSPB_SHAPE)};
constexpr Shape kStShapes[] = {DSPB_ST_KERNELS(DSPB_SHAPE)};
constexpr Shape kSegShapes[] = {DSPB_SEG_KERNELS(DSPB_SEG_SHAPE)};
constexpr Shape kWalkShapes[] = {DSPB_WALK_KERNELS(DSPB_SHAPE)};
constexpr Shape kChainShapes[] = {DSPB_CHAIN_KERNELS(DSPB_SHAPE)};
constexpr Shape kChainIndShapes[] = {DSPB_CHAIN_IND_KERNELS(DSPB_SHAPE)};
static_assert(std::size(kChainShapes) == std::size(kChainIndShapes), "the chains of one shape list");
// the first kernel of a table that is loaded (ok(i)) and compiled for (C, B);
// a shape of any B takes B <= max_b.  -1: none
template <size_t N, class Ok>
int pick_shape(const Shape (&shapes)[N], uint32_t C, uint32_t B, Ok ok, uint32_t max_b = ~0u) {
    for (size_t i = 0; i < N; ++i) {
        const Shape &sh = shapes[i];
        if ((!sh.C || sh.C == C) && (sh.B ? sh.B == B : B <= max_b) && (!sh.pf || B % 4 == 0) && ok(i)) return (int)i;
    }
    return -1;
}

struct ArenaHost {  // mirror of dspb_arena
    char *base;
    unsigned long long capacity;
    unsigned long long used;
    float *fft_tmp;
    unsigned long long failed;
};

// a device allocation that its holder owns: freed when replaced, and with it
template <class T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    hipError_t alloc(uint64_t bytes) {
        reset();
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
};

}  // namespace dspb

struct dsp_module {
    dsp_descriptor *desc = nullptr;  // from the code object (NULL for code without one)
    int device = -1;
    hipModule_t mod = nullptr;
    hipModule_t chain_mod = nullptr;   // the State chain kernels from edited IR (dspb_chain_co), or NULL
    // the LDS-blocks kernels, as kLdsShapes (NULL for code objects compiled
    // before they existed)
    hipFunction_t f_render_lds[std::size(dspb::kLdsShapes)] = {};
    hipFunction_t f_render_st[std::size(dspb::kStShapes)] = {};  // kStShapes (NULL: dspb_render)
    // speculative segments (kSegShapes, the check, kWalkShapes; NULL in code
    // objects compiled before them: the serial chain)
    hipFunction_t f_seg[std::size(dspb::kSegShapes)] = {}, f_seg_rerun[std::size(dspb::kSegShapes)] = {},
                  f_seg_check = nullptr, f_seg_walk[std::size(dspb::kWalkShapes)] = {};
    // kChainShapes and their private memory per lane: one whose compiled
    // form kept more than a State copy there kept (part of) the block, which
    // the State then depends on -- the serial chain renders instead
    hipFunction_t f_seg_chain[std::size(dspb::kChainShapes)] = {};
    int chain_priv[std::size(dspb::kChainShapes)] = {};
    hipFunction_t f_seg_chain_ind[std::size(dspb::kChainIndShapes)] = {};  // (facts.state_split), private memory as above
    int chain_ind_priv[std::size(dspb::kChainIndShapes)] = {};
    // the device and pinned resources of the speculative renders (what the
    // renders taught: `learn`)
    struct SegWork {
        dspb::DevBuf<void> blk;           // [cap_blk] States: st_blk
        dspb::DevBuf<void> ind;           // [cap_ind] States: a split State's independent words (st_ind, kSegLevels K)
        uint64_t cap_ind = 0;
        dspb::DevBuf<void> end;           // [cap] States: st_end
        uint64_t cap_blk = 0;
        dspb::DevBuf<unsigned> list;      // [cap]
        dspb::DevBuf<unsigned char> flags;  // [cap]
        dspb::DevBuf<unsigned> words;     // [DSPB_WORDS]: the listings' counts and stats (dspb_word_slot)
        uint32_t cap = 0;
        // the counters of the last two speculative renders: pinned copies
        // [2][DSPB_STAT_PINNED], each behind an event, read back without waiting by a later
        // call (what the module learns) or waiting by dsp_module_state_spec
        unsigned *h_stats = nullptr;
        hipEvent_t ev[2] = {};
        uint64_t perturb = 0;          // dsp_module_debug: the next State chain's wrong record (block + 1)
    } seg;
    dspb::SegLearner learn;
    hipFunction_t f_sizes = nullptr, f_defaults = nullptr, f_init = nullptr, f_render = nullptr,
                  f_callback = nullptr;
    uint32_t params_size = 0, state_size = 0;
    int stateless = 0;                 // State is empty
    // blocks render independently, so in parallel: the callback's IR was
    // analysed completely (no global memory written, no unknown call) and it
    // never writes its State (facts); otherwise the blocks run in order on
    // one lane, as the reference's audio thread runs them
    int par = 0;
    bool has_facts = false;            // the code object carries dspb_callback_facts
    dspb::irp::Facts facts;            // what the callback's IR shows (ir_proof.hpp)
    int cus = 256;                     // compute units of the device (persistent grids)
    void *h_params = nullptr;          // pinned staging of the Parameters upload
    hipEvent_t upload_ev = nullptr;    // the last upload from h_params
    hipEvent_t use_ev = nullptr;       // the last render launched with d_params / d_state
    void *d_params = nullptr;          // device Parameters
    void *d_state[2] = {nullptr, nullptr};  // [0] live State, [1] compute_IR scratch State
    dspb::ArenaHost *d_arena[2] = {nullptr, nullptr};
    char *arena_mem[2] = {nullptr, nullptr};
    bool initialized = false;
    // block classes found by module_specialize, per (Parameters, C, B, sr);
    // newest last, at most kSpecCache
    // a table class's block: the calls that hold it (module_specialize hands
    // it out, module_spec_done takes it back after the call's launches), an
    // event per stream after its last use, and whether a captured graph may
    // replay it (then it lives as long as the module)
    struct SpecUse {
        float *table = nullptr;
        std::map<hipStream_t, hipEvent_t> ev;
        int inflight = 0;
        bool captured = false;
    };
    struct Spec {
        std::vector<unsigned char> params;
        uint32_t C, B;
        float sr;
        dspb::ModuleSpec r;
        std::shared_ptr<SpecUse> use;  // table classes only
    };
    std::vector<Spec> spec;
    // tables of evicted entries: freed once no call holds them and their
    // streams have passed their last use (spec_reap), or by
    // dsp_module_destroy when a captured graph may replay them
    std::vector<std::shared_ptr<SpecUse>> retired;
    std::mutex mu;
};

namespace dspb {

// host-side writers of the device Parameters / State wait for the renders
// that use them
inline int wait_uses(dsp_module *m) {
    if (m->use_ev) DSPB_HIP(hipEventSynchronize(m->use_ev));
    return DSP_OK;
}
inline bool params_fit(const dsp_module *m, const void *params, uint32_t n) {
    return n == m->params_size && (params || !n);
}

// module_load.cpp: the checks and steps every GENERIC call starts with
int check_device(const dsp_module *m);                       // called on the module's device, or refused
int refuse_generic_capture(hipStream_t s);                   // a GENERIC call cannot be captured
int check_params(const dsp_module *m, const void *params, uint32_t n);  // params_fit, or refused
int upload_params(dsp_module *m, const void *params, uint32_t n, hipStream_t s);
// the callback once (one lane) on C rows of B samples, in place, with State
// `slot`; the launch counts as a use of the device Parameters / State
int callback_on(dsp_module *m, int slot, float *const *rows, uint32_t C, uint32_t B, float sr, hipStream_t s);

// module_seg.cpp.  module_render_seg returns 1 (nothing launched) when the
// call does not fit the segments: the caller renders the serial chain
int module_render_seg(dsp_module *m, dspb_render_args &A, hipStream_t s, bool chain);
int module_seg_collect(dsp_module *m, bool wait);

}  // namespace dspb
