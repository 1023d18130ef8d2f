// module_seg.cpp -- a State-writing callback over the whole file as
// speculative segments (kSegDriver): the kernels of the shape, the
// workspaces, the warm-up levels, then the launches, and the read-back of
// each render's counters.  What a render starts with and what its counters
// teach is SegLearner's (module_policy.cpp, no HIP); this file keeps the
// buffers, events, copies and launches.
#include <algorithm>

#include "module_impl.hpp"

namespace dspb {

// The counters of the speculative renders not yet read (pinned copies, each
// behind an event), oldest first, to the learner.  wait = false reads them
// only if they have landed (a render never waits for them).
int module_seg_collect(dsp_module *m, bool wait) {
    auto &W = m->seg;
    SegLearner &T = m->learn;
    const int older = T.slot();
    for (int i : {older, 1 - older}) {
        if (!T.pending[i]) continue;
        if (wait) DSPB_HIP(hipEventSynchronize(W.ev[i]));
        else if (hipEventQuery(W.ev[i]) != hipSuccess) {
            (void)hipGetLastError();
            continue;
        }
        T.landed(i, W.h_stats + DSPB_STAT_PINNED * i);
    }
    return DSP_OK;
}

// The kernels of a speculative render of (C, B) and its geometry
struct SegKernels {
    hipFunction_t pass1 = nullptr, rerun = nullptr, walk = nullptr;
    hipFunction_t chain = nullptr;  // the State chain, if the shape has one (dspb_seg_chain)
    hipFunction_t split = nullptr;  // the chain of a split State's independent words (dspb_seg_chain_ind)
    uint64_t stride = 0, nb = 0;    // floats per block in LDS, lanes per workgroup
};
// the chain kernel of a shape, if its compiled form dropped the block (its
// private memory holds no more than a State copy)
template <size_t N>
static hipFunction_t chain_kernel(const dsp_module *m, const Shape (&shapes)[N], const hipFunction_t (&f)[N],
                                  const int (&priv)[N], uint32_t C, uint32_t B) {
    const int i = pick_shape(
        shapes, C, B, [&](size_t j) { return f[j] && (uint64_t)priv[j] <= (uint64_t)m->state_size + 64; },
        dspb_chain_max_b);
    return i < 0 ? nullptr : f[i];
}
// false: the shape does not fit the segment kernels (`chain`: nor a State chain)
static bool seg_kernels(const dsp_module *m, uint32_t C, uint32_t B, bool chain, SegKernels *k) {
    if (2ull * C * B * sizeof(float) > kStagedLdsBytes) return false;  // the walk's double buffer
    k->chain = chain_kernel(m, kChainShapes, m->f_seg_chain, m->chain_priv, C, B);
    if (chain && !k->chain) return false;
    const int fi = pick_shape(kSegShapes, C, B, [&](size_t i) {
        return m->f_seg[i] && (!kSegShapes[i].rerun || m->f_seg_rerun[i]);
    });
    const int wi = pick_shape(kWalkShapes, C, B, [&](size_t i) { return m->f_seg_walk[i] != nullptr; });
    if (fi < 0 || wi < 0 || !m->f_seg_check) return false;
    k->pass1 = m->f_seg[fi];
    k->rerun = kSegShapes[fi].rerun ? m->f_seg_rerun[fi] : k->pass1;
    k->walk = m->f_seg_walk[wi];
    k->stride = kSegShapes[fi].pf ? dspb_stride_pf(C, B) : dspb_stride(C, B);
    k->nb = dspb_seg_nb(k->stride);
    if (k->nb < 4) return false;
    // a split State: the chain of its independent words (no private block:
    // the words need no sample)
    if (!chain && m->facts.state_split)
        k->split = chain_kernel(m, kChainIndShapes, m->f_seg_chain_ind, m->chain_ind_priv, C, B);
    return true;
}
// The workspaces of K segments over nblocks blocks; 1: no room for the
// records (the serial chain renders this call).  Without room for a split
// State's records only, *split is dropped: plain speculation.
static int seg_grow(dsp_module *m, uint64_t K, uint64_t nblocks, hipFunction_t *split) {
    auto &W = m->seg;
    if (*split && kSegLevels * K > W.cap_ind) {
        if (int st = wait_uses(m)) return st;
        W.cap_ind = 0;
        const uint64_t cap = std::max<uint64_t>(kSegLevels * K, 4096);
        if (W.ind.alloc(cap * m->state_size) != hipSuccess) {
            (void)hipGetLastError();
            *split = nullptr;
        } else {
            W.cap_ind = cap;
        }
    }
    if (K > W.cap || nblocks > W.cap_blk) {
        if (int st = wait_uses(m)) return st;
        auto drop = [&] { W.blk.reset(), W.end.reset(), W.list.reset(), W.flags.reset(); };
        drop();  // (before the larger ones are made)
        W.cap = 0, W.cap_blk = 0;
        const uint32_t cap = (uint32_t)std::max<uint64_t>(K, 1024);
        const uint64_t cap_blk = std::max<uint64_t>(nblocks, 4096);
        if (W.blk.alloc(cap_blk * m->state_size) != hipSuccess ||
            W.end.alloc((uint64_t)cap * m->state_size) != hipSuccess ||
            W.list.alloc(cap * sizeof(unsigned)) != hipSuccess || W.flags.alloc(cap) != hipSuccess) {
            (void)hipGetLastError();
            drop();
            return 1;
        }
        W.cap = cap;
        W.cap_blk = cap_blk;
    }
    if (!W.words.p) {
        DSPB_HIP(W.words.alloc(DSPB_WORDS * sizeof(unsigned)));
        DSPB_HIP(hipHostMalloc(&W.h_stats, 2 * DSPB_STAT_PINNED * sizeof(unsigned), hipHostMallocDefault));
        for (hipEvent_t &e : W.ev) DSPB_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    return DSP_OK;
}
// One render's launches.  `base` holds what every launch shares (the buffers,
// the geometry, the split State's records, the test hook); each launch kind
// names the fields its kernel reads besides (directly, or through
// dspb_seg_level_runs / dspb_seg_skip); a field no kernel of the kind reads
// stays zero.
struct SegLaunch {
    const dsp_module *m;
    const SegKernels &k;
    hipStream_t s;
    dspb_seg_args base;
    unsigned *words;
    int go(hipFunction_t f, unsigned grid, unsigned block, unsigned lds, dspb_seg_args G) const {
        void *args[] = {&G};
        DSPB_HIP(hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, lds, s, args, nullptr));
        return DSP_OK;
    }
    // pass 1 (mode 0) or a rerun of the listed segments / of every segment from the chain's records
    int segments(hipFunction_t f, dspb_seg_args G) const {
        return go(f, (unsigned)((base.K + k.nb - 1) / k.nb), 256, (unsigned)(k.nb * k.stride * sizeof(float)), G);
    }
    int pass1(unsigned level, unsigned warm, unsigned prev_warm) const {
        dspb_seg_args G = base;
        G.mode = 0, G.level = level, G.warm = warm, G.prev_warm = prev_warm, G.count = words + DSPB_WORD_COUNT;
        return segments(k.pass1, G);
    }
    int rerun(unsigned exact, unsigned *count) const {
        dspb_seg_args G = base;
        G.mode = 1, G.exact = exact, G.count = count;
        return segments(k.rerun, G);
    }
    // 4 segments per 256 threads; list = true: the differing segments are listed in `count` for a rerun.
    // Pass 1's check (level != DSPB_NO_LEVEL) decides as pass 1 did whether the level runs: its prev_warm
    int check(unsigned level, unsigned prev_warm, unsigned pass, bool list, unsigned exact, unsigned *count,
              unsigned *prev_count) const {
        dspb_seg_args G = base;
        G.level = level, G.prev_warm = prev_warm, G.pass = pass, G.mode = list ? 1 : 0, G.exact = exact;
        G.count = count, G.prev_count = prev_count;
        return go(m->f_seg_check, (unsigned)((base.K + 3) / 4), 256, 0, G);
    }
    int walk(unsigned exact) const {
        dspb_seg_args G = base;
        G.exact = exact;
        return go(k.walk, 1, 256, (unsigned)(2ull * base.R.C * base.R.B * sizeof(float)), G);
    }
    // mode 2: within a speculative render, only when level `level` would run (the one before failed)
    int chain(unsigned mode, unsigned level, unsigned prev_warm) const {
        dspb_seg_args G = base;
        G.mode = mode, G.level = level, G.prev_warm = prev_warm;
        return go(k.chain, 1, 64, 0, G);
    }
    int split_chain(unsigned level, unsigned warm, unsigned prev_warm) const {
        dspb_seg_args G = base;
        G.level = level, G.warm = warm, G.prev_warm = prev_warm;
        return go(k.split, 1, 64, 0, G);
    }
    // every segment from the State chain's records, the records checked: every
    // boundary against the State the segment before ended with, then the walk
    // renders serially from the true State whatever differs and writes the
    // live State (exact 2: each returns at once unless the chain ran)
    int from_chain(unsigned exact) const {
        if (int st = rerun(exact, nullptr)) return st;
        if (int st = check(DSPB_NO_LEVEL, 0, DSPB_STAT_CHAIN_MISMATCH, false, exact, nullptr, nullptr)) return st;
        return walk(exact);
    }
};
// Returns 1 (nothing launched) when the shape does not fit the segments -- the
// caller renders the serial chain.  `chain` (a State learned not to forget):
// the chain kernel records every block's State, and the exact rerun renders
// the segments from them (dspb_seg_chain).
int module_render_seg(dsp_module *m, dspb_render_args &A, hipStream_t s, bool chain) {
    SegKernels k;
    if (!seg_kernels(m, A.C, A.B, chain, &k)) return 1;
    auto &W = m->seg;
    SegLearner &T = m->learn;
    // segments: as many as the chip runs lanes at once (two workgroups per
    // CU, nb lanes each)
    uint64_t seg = 0, K = 0;
    if (!SegLearner::geometry(A.nblocks, kLdsWgPerCu * (uint64_t)m->cus * k.nb, m->state_size, &seg, &K)) return 1;
    if (int st = seg_grow(m, K, A.nblocks, &k.split)) return st;
    const int slot = T.slot();
    if (T.pending[slot]) {
        DSPB_HIP(hipEventSynchronize(W.ev[slot]));
        if (int st = module_seg_collect(m, false)) return st;
    }
    SegLaunch q{m, k, s, {}, W.words.p};
    dspb_seg_args &G = q.base;
    G.R = A;
    G.R.lds_nb = (unsigned)k.nb;
    G.R.lds_stride = (unsigned)k.stride;
    G.st_blk = W.blk.p;
    G.st_end = W.end.p;
    G.list = W.list.p;
    G.flags = W.flags.p;
    G.stats = q.words + DSPB_WORD_STATS;
    G.seg = seg;
    G.K = (unsigned)K;
    G.perturb = chain || k.chain || k.split ? W.perturb : 0;  // (test hook: consumed by the render that may run a chain)
    if (G.perturb) W.perturb = 0;
    if (k.split) {  // pass 1 starts every warm-up from the split chain's words (the others from the live State)
        G.st_ind = W.ind.p;
        G.split = 1;
    }
    DSPB_HIP(hipMemsetAsync(q.words, 0, DSPB_WORDS * sizeof(unsigned), s));
    uint32_t levels = 0;
    if (chain) {
        if (int st = q.chain(1, 0, 0)) return st;
        if (int st = q.from_chain(1)) return st;
    } else {
        uint32_t lw[kSegLevels] = {};
        levels = T.levels(A.nblocks, seg, k.chain != nullptr, lw);
        for (uint32_t L = 0; L < levels; ++L) {
            const uint32_t prev = L ? lw[L - 1] : 0;
            // a split State: the chain of its independent words first, recording
            // them where this level's warm-ups start (it runs only where the
            // level does)
            if (k.split)
                if (int st = q.split_chain(L, lw[L], prev)) return st;
            if (int st = q.pass1(L, lw[L], prev)) return st;
            if (int st = q.check(L, prev, DSPB_STAT_LEVEL_DIFFERED + L, true, 0, q.words + DSPB_WORD_COUNT, nullptr)) return st;
        }
        // the last level failed (decided on the GPU): the State chain and the
        // exact rerun take over, the reruns and the walk below return at once
        if (k.chain)  // (levels >= 1: level 0 is always planned)
            if (int st = q.chain(2, levels, lw[levels - 1])) return st;
        // two reruns of the listed segments, each checked; the last check only flags
        unsigned *listing = q.words + DSPB_WORD_COUNT;
        for (unsigned p = 0; p < 2; ++p) {
            unsigned *next = q.words + DSPB_WORD_RERUN_COUNT + p;
            if (int st = q.rerun(0, listing)) return st;
            if (int st = q.check(DSPB_NO_LEVEL, 0, DSPB_STAT_RERUN_DIFFERED + p, p == 0, 0, next, listing)) return st;
            listing = next;
        }
        if (int st = q.walk(0)) return st;
        if (k.chain)
            if (int st = q.from_chain(2)) return st;
    }
    DSPB_HIP(hipMemcpyAsync(W.h_stats + DSPB_STAT_PINNED * slot, G.stats, DSPB_STAT_PINNED * sizeof(unsigned),
                           hipMemcpyDeviceToHost, s));
    DSPB_HIP(hipEventRecord(W.ev[slot], s));
    T.launched(slot, K, seg, levels, chain, k.split != nullptr);
    DSPB_HIP(hipEventRecord(m->use_ev, s));
    return DSP_OK;
}

}  // namespace dspb
