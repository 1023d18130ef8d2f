// plugin_driver_abi.h -- the one contract between the plugin driver's kernels
// (plugin_driver.inl, plugin_driver_seg.inl: compiled by hiprtc into every
// plugin module) and the host code that picks and launches them (module.cpp).
// Both sides read this text: module.cpp includes it, the Makefile embeds it at
// the front of kDriver.  Plain C++ with no #include (hiprtc compiles it as
// part of the driver string).  DSPB_LDS_ROUND_BYTES is defined before it on
// both sides (module.cpp hands its own value to hiprtc with -D).
#ifndef DSPB_ABI_STATE
#define DSPB_ABI_STATE void  // the host sees a State as bytes; the module's unit defines it as State
#endif
constexpr unsigned dspb_max_channels = 16;  // channels per launch
constexpr unsigned dspb_chain_max_b = 4096;  // the chain kernels of any B: their private block holds this B

// ---- the argument blocks (code objects compiled earlier still load: the
// layout is pinned by static_asserts in module.cpp) --------------------------
struct dspb_render_args {
    void *P;
    void *S;
    float *in[dspb_max_channels];
    float *out[dspb_max_channels];
    unsigned long long L;
    unsigned long long nblocks;
    unsigned long long block0;
    unsigned in_ch;
    unsigned C;
    unsigned B;
    float sr;
    unsigned lds;         // path: stateful 1 = LDS double buffer; stateless 3 = LDS blocks
    unsigned lds_nb;      // LDS blocks / segments: blocks per workgroup round
    unsigned lds_stride;  // ... and floats per block in LDS (dspb_stride / dspb_stride_pf)
    unsigned par;         // blocks render independently, in parallel
};
struct dspb_seg_args {
    dspb_render_args R;
    DSPB_ABI_STATE *st_blk;  // [nblocks] the State each block was rendered from
    DSPB_ABI_STATE *st_end;  // [K] the State each segment ended with
    unsigned *list;          // segments to rerun (check -> rerun)
    unsigned *count;         // how many
    unsigned *prev_count;    // a rerun's check: the rerun's count (0: nothing changed, skip)
    unsigned char *flags;    // the last check: 1 = differed
    unsigned *stats;         // the counters of one render (dspb_stat)
    unsigned long long seg;  // blocks per segment
    unsigned K;              // segments
    unsigned warm;           // pass 1: warm-up blocks
    unsigned prev_warm;      // pass 1 at level > 0: the warm-up of the level before
    unsigned level;          // pass 1 / its check: the warm-up level (DSPB_NO_LEVEL: a rerun's check)
    unsigned mode;           // segments: 0 = pass 1 (every segment), 1 = rerun the listed ones;
                             // check: 1 = list the differing ones for a rerun (0: flag only);
                             // chain: 2 = only when the last level tried failed
    unsigned pass;           // the check's stats slot
    unsigned exact;          // a rerun of every segment from the States the chain kernel recorded
                             // (dspb_seg_chain): no list, no early stop (2: only if the chain ran);
                             // the check and the walk after it: every segment boundary
    unsigned long long perturb;  // test hook (dsp_module_debug): the chain kernel flips a bit of the
                                 // State it recorded for block perturb - 1 (0: none)
    DSPB_ABI_STATE *st_ind;  // [levels][K] a split State's block-independent words where pass 1 at each
                             // warm-up level starts segment k's warm-up (dspb_seg_chain_ind); the
                             // other words are not written
    unsigned split;          // pass 1 starts each segment's warm-up from st_ind's words
};
constexpr unsigned DSPB_NO_LEVEL = 0xffffffffu;

// ---- the counters of a speculative render ----------------------------------
// `words` is one device allocation: the listings' counts, then `stats`
enum dspb_word_slot : unsigned {
    DSPB_WORD_COUNT = 0,        // pass 1's listing
    DSPB_WORD_RERUN_COUNT = 2,  // + p: the listing of rerun p's check
    DSPB_WORD_STATS = 8,        // dspb_seg_args.stats
    DSPB_WORDS = 32,
};
enum dspb_stat : unsigned {
    DSPB_STAT_LEVEL_DIFFERED = 0,   // + level, [0, 4): segments that differed per warm-up level
    DSPB_STAT_RERUN_DIFFERED = 4,   // + p, [4, 6): ... after rerun p
    DSPB_STAT_WALK_RERUNS = 7,      // serial reruns of the walk
    DSPB_STAT_LEVEL_RAN = 8,        // + level, [8, 12): the level ran
    DSPB_STAT_CHAINED = 12,         // the State chain took over from the levels (dspb_seg_chain)
    DSPB_STAT_CHAIN_MISMATCH = 13,  // segments whose first State (the chain's record) differed from
                                    // the State the segment before ended with
    DSPB_STAT_CHAIN_RECORDS = 14,   // blocks whose State in the exact rerun differed from the chain's record
    DSPB_STAT_PINNED = 16,          // the words above: copied to the host after every render
    // DSPB_SEG_TIMING (dsp_module_seg_timing): pass 1's clocks / 16 per phase, summed over workgroups
    DSPB_STAT_TIMING = 16,          // + phase, [16, 21)
    DSPB_STAT_TIMING_WGS = 21,      // workgroups that added theirs
    DSPB_STAT_TIMING_ROUNDS = 22,   // rounds they ran
    DSPB_STAT_WORDS = 24,
};
constexpr unsigned dspb_max_levels = 4;  // warm-up levels a render may try
static_assert(DSPB_WORD_STATS + DSPB_STAT_WORDS == DSPB_WORDS, "stats fill the rest of words");

// ---- the LDS round geometry -------------------------------------------------
// floats per block in LDS: rows at C B + 1 (the callback lanes of one ds_read
// on different banks); C B + 2 for the pipelined and role kernels (8-byte
// aligned: their copies move float2 pairs through LDS)
constexpr unsigned long long dspb_stride(unsigned long long C, unsigned long long B) { return C * B + 1u; }
constexpr unsigned long long dspb_stride_pf(unsigned long long C, unsigned long long B) { return C * B + 2u; }
// blocks per round of the LDS-blocks path at a block stride of SB floats, a
// multiple of 4 (18 blocks of stereo B = 512 instead of 16 made the
// stateless rounds 1-6% slower, profiles/r05_lds_nb_ab.txt), and lanes of
// the segment kernels: as many as the round's LDS holds (18 instead of 16:
// 15% faster)
constexpr unsigned long long dspb_seg_nb(unsigned long long SB) {
    const unsigned long long v = DSPB_LDS_ROUND_BYTES / (SB * 4u);
    return v < 64u ? v : 64u;
}
constexpr unsigned long long dspb_lds_nb(unsigned long long SB) { return dspb_seg_nb(SB) / 4u * 4u; }
// an LDS-blocks kernel of a constant shape with 4 | B runs the pipelined rounds
constexpr bool dspb_lds_pipelined(unsigned C, unsigned B) { return C > 0 && B > 0 && B % 4 == 0; }

// ---- the kernels, one list per family: X(name, C, B, ...), C / B = 0: any
// value; most specific first (the host takes the first that matches) --------
#define DSPB_LDS_KERNELS(X)            \
    X(dspb_render_lds_c2b512, 2, 512)  \
    X(dspb_render_lds_c2b256, 2, 256)  \
    X(dspb_render_lds_c2b1024, 2, 1024) \
    X(dspb_render_lds_c1b512, 1, 512)  \
    X(dspb_render_lds_c1, 1, 0)        \
    X(dspb_render_lds_c2, 2, 0)        \
    X(dspb_render_lds, 0, 0)
// the stateful LDS path's kernels: dspb_render covers every other shape
#define DSPB_ST_KERNELS(X)            \
    X(dspb_render_st_c2b512, 2, 512)  \
    X(dspb_render_st_c2b256, 2, 256)  \
    X(dspb_render_st_c1, 1, 0)        \
    X(dspb_render_st_c2, 2, 0)
// speculative segments: pass 1 `name` of kind P1 (roles / pf / any) and its
// reruns' kernel of kind RR (pf: name_rerun; same: pass 1's kernel).  roles
// and pf stride blocks by dspb_stride_pf and need 4 | B.
#define DSPB_SEG_KERNELS(X)               \
    X(dspb_seg_c2b512, 2, 512, roles, pf) \
    X(dspb_seg_c2, 2, 0, pf, pf)          \
    X(dspb_seg_c1, 1, 0, pf, pf)          \
    X(dspb_seg_c4, 4, 0, pf, pf)          \
    X(dspb_seg, 0, 0, any, same)
#define DSPB_WALK_KERNELS(X)         \
    X(dspb_seg_walk_c2b512, 2, 512)  \
    X(dspb_seg_walk_any, 0, 0)
// the chain kernels of a State that never forgets (B = 0: any B <=
// dspb_chain_max_b), and of a split State's block-independent words
#define DSPB_CHAIN_KERNELS(X)         \
    X(dspb_seg_chain_c2b512, 2, 512)  \
    X(dspb_seg_chain_c2, 2, 0)        \
    X(dspb_seg_chain_c1, 1, 0)        \
    X(dspb_seg_chain_c4, 4, 0)
#define DSPB_CHAIN_IND_KERNELS(X)         \
    X(dspb_seg_chain_ind_c2b512, 2, 512)  \
    X(dspb_seg_chain_ind_c2, 2, 0)        \
    X(dspb_seg_chain_ind_c1, 1, 0)        \
    X(dspb_seg_chain_ind_c4, 4, 0)
