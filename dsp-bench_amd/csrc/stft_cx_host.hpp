// stft_cx_host.hpp -- the host half of dsp_stft and dsp_istft (dspbench.h): both
// plans (frames, Lout, overlap, chunk, the scratch layout) and the argument
// rules that need no device.  No HIP here: plain C++ (stft_cx_host.cpp), like
// welch_host.cpp.
#pragma once
#include <cstdint>

#include "dspbench/dspbench.h"

namespace dspb {

constexpr uint32_t kStftCxN = 8192;
constexpr uint32_t kStftCxBins = kStftCxN / 2 + 1;  // 4097
constexpr uint32_t kStftCxGroup = 16;               // rows per channel group (kMaxChannels: capi_grid.cpp asserts it)
constexpr uint32_t kIstftMinHop = 512;              // at most 16 frames touch a sample
constexpr uint64_t kIstftFrameBytes = 4ull * kStftCxN;  // a windowed inverse frame in the scratch
// the frames a chunk may hold: chunk = the largest count with rows chunk 32 KiB
// <= this (rows = min(C, 16))
constexpr uint64_t kIstftChunkBytes = 64ull << 20;

struct StftCxPlan {
    uint32_t H = 0;
    int32_t window = 0;
    uint64_t frames = 0;
    uint64_t min_ld = 0;  // floats: 2 K
};

struct IstftPlan {
    uint32_t H = 0;
    int32_t window = 0;
    float floor = 0.f;       // the spec's floor rounded to float: what the kernel compares with
    uint64_t frames = 0;
    uint64_t Lout_full = 0;  // N + (F - 1) H
    uint32_t overlap = 0;    // ceil(N / H): frames that touch a sample
    uint32_t rows = 0;       // min(C, 16)
    uint32_t chunk = 0;      // frames whose samples one pair of launches finishes
    // the scratch: [rows][slots] frames of 8192 floats, w v_f.  A chunk's first
    // launch fills chunk + overlap - 1 slots at most (the frames before the
    // chunk that its samples still touch); a call of F <= chunk frames takes F.
    uint32_t slots = 0;
    uint64_t scratch_bytes = 0;
};

// the plans' bodies: 0, 1 (invalid) or 2 (unsupported) with *why set
int stft_cx_plan(uint64_t L, uint32_t C, const dsp_stft_spec *spec, StftCxPlan *plan, const char **why);
int istft_plan(uint64_t F, uint32_t C, const dsp_istft_spec *spec, IstftPlan *plan, const char **why);

// the calls' own rules (after the plan): the row stride, and Lout against the plan
int stft_cx_check_ld(bool inverse, uint64_t frames, uint64_t ld, const char **why);
int istft_check_lout(const IstftPlan &p, uint64_t Lout, const char **why);

// One chunk of the inverse: frames [f0, f0 + nf) of F own the samples [i0, i1)
// of an output row of Lout samples, and their sums need the frames [fa, fa + ns)
// in the scratch.  nf = 0: the chunk lies past Lout, nothing to do.
struct IstftChunk {
    uint64_t f0 = 0, fa = 0, i0 = 0, i1 = 0;
    uint32_t nf = 0, ns = 0;
};
IstftChunk istft_chunk(const IstftPlan &p, uint64_t f0, uint64_t Lout);

}  // namespace dspb
