// stft_pk.hip -- the 8192-point STFT dispatcher and the fused IR_test
// kernels of the headline (PER path, and the store-only launch of a cached
// spectrum row); the kernels are in stft_pk.hpp.
#include "stft_pk.hpp"
#include <hip/hip_ext.h>

namespace dspb {

// Host -> device upload of the library's small constant tables through
// kernel arguments.  The first hipMemcpy of more than a few KB in a process,
// pageable or pinned, costs 7-8 ms (copy-engine start-up,
// tools/copy_init_probe.cpp; 0.02 ms afterwards) and was most of a cold
// call; ~4 KB of kernel arguments per launch costs microseconds.  Here, in
// the headline's translation unit, so that a cold headline call loads one
// code object.
constexpr uint32_t kUploadFloats = 960;
struct UploadChunk {
    uint32_t n;
    float v[kUploadFloats];
};
__global__ void upload_kernel(float *dst, UploadChunk c) {
    for (uint32_t i = threadIdx.x; i < c.n; i += blockDim.x) dst[i] = c.v[i];
}
int launch_upload(float *dst, const float *src, uint64_t n, hipStream_t s) {
    UploadChunk c;
    for (uint64_t off = 0; off < n; off += kUploadFloats) {
        c.n = (uint32_t)(n - off < kUploadFloats ? n - off : kUploadFloats);
        for (uint32_t i = 0; i < c.n; ++i) c.v[i] = src[off + i];
        hipLaunchKernelGGL(upload_kernel, dim3(1), dim3(256), 0, s, dst + off, c);
        DSPB_HIP(hipGetLastError());
    }
    return DSP_OK;
}

// true when launch_stft8192_pk runs the PER kernel for these arguments --
// the fused path that evaluates a closed-form IR ramp itself and renders the
// tail past the last frame's hop (A.tail_end)
bool stft8192_pk_per_path(const Stft8kArgs &A, bool fused) {
    const int km = A.K == 4097u ? kKHalf : (A.K == 8192u ? kKMirror : kKPartial);
    const bool pow2 = A.map.b_mask != 0 && A.map.B >= 2;
    const bool winc = A.valid >= 8192u && A.wbase != nullptr && km == kKHalf;
    return fused && A.map.kind == MapKind::Ramp && pow2 && winc && A.map.B <= 2048u;
}

// Frame reuse.  On the PER path a frame is table[(goff + f H + n) & (B - 1)]:
// with H % B == 0 it does not depend on f, so every frame of the call has the
// same samples and the same spectrum, and a wave can compute it once for a run
// of frames and only repeat the stores.  The default run is kPkRunMax frames,
// and never more than the static split of the call over the wave slots of the
// device (kPkWaveSlots / C per channel), so that a call too short to fill them
// keeps one frame per wave (run 1), which finishes sooner than fewer, longer
// waves would.  kPkRunMax = 4 is measured (profiles/r07_frame_run_ab.txt):
// runs of 4 to 42 are equally fast on a machine that lets the launch run at
// full clock, and on one that does not the time grows with the run; 4 is the
// longest that is not behind one FFT per frame there.
constexpr uint32_t kPkWaveSlots = 256u * 4u * 2u;  // MI355X: 256 CUs x 4 SIMDs x 2 waves (amdgpu_waves_per_eu 2)
constexpr uint32_t kPkRunMax = 4;
uint32_t stft8192_pk_frame_run(const Stft8kArgs &A, bool fused, uint32_t C, uint32_t forced) {
    if (!stft8192_pk_per_path(A, fused) || A.map.B == 0 || A.H % A.map.B != 0 || A.F == 0 || C == 0) return 1;
    if (forced) return forced;
    const uint64_t slots = kPkWaveSlots / C ? kPkWaveSlots / C : 1;
    const uint64_t run = (A.F + slots - 1) / slots;
    return (uint32_t)(run < kPkRunMax ? run : kPkRunMax);
}

// A.win2: the window pre-scaled by 0.5 / sqrt(8192); the computed window
// (A.wbase, A.wa, A.wb) serves the full-frame 4097-bin shapes.
int launch_stft8192_pk(const Stft8kArgs &A_, uint32_t C, bool fused, int opt, hipStream_t stream) {
    if (A_.F == 0 || C == 0) return DSP_OK;
    Stft8kArgs A = A_;
    if (A.run == 0) A.run = 1;
    // a run of frames is one spectrum: only where stft8192_pk_frame_run allows it
    if (A.run > 1 && stft8192_pk_frame_run(A, fused, C, A.run) != A.run) return DSP_ERR_INVALID;
    A.run_waves = (A.F + A.run - 1) / A.run;
    // PER path: extra waves for the render tail [F H, tail_end)
    const uint64_t tail = A.tail_end > A.F * A.H ? (A.tail_end - A.F * A.H + A.H - 1) / A.H : 0;
    if (tail && !stft8192_pk_per_path(A, fused)) return DSP_ERR_INVALID;
    const uint64_t groups = (A.F + tail + kPkWpb - 1) / kPkWpb;  // workgroups of the default kernels
    if (groups > 0x7fffffffull) return DSP_ERR_INVALID;
    dim3 grid((uint32_t)groups, C);
    const int km = A.K == 4097u ? kKHalf : (A.K == 8192u ? kKMirror : kKPartial);
    const bool pow2 = A.map.b_mask != 0 && A.map.B >= 2;
    const bool winc = A.valid >= 8192u && A.wbase != nullptr && km == kKHalf;
    if (fused && A.map.kind == MapKind::Ramp && pow2 && winc) {
        // period of the block table in units of 128 samples
        const uint32_t per = A.map.B <= 128u ? 1u : A.map.B / 128u;
        if (per == 4 && opt) {  // A/B at the headline shape (the tools build only: stft_pk_ab.hip)
            int st = DSP_OK;
            Stft8kArgs A1 = A;  // the variants size their grids for one frame per wave
            A1.run = 1;
            A1.run_waves = A.F;
            if (stft_pk_ab_dispatch(A1, C, fused, opt, grid, stream, &st)) return st;
        }
        // (run 1: the instantiation without the reuse path, the per-frame kernel as it was)
#define DSPB_PK_PER(p)                                                                                                \
    do {                                                                                                              \
        if (A.run > 1)                                                                                                \
            hipLaunchKernelGGL((stft8192_pk_kernel<kSrcRender, kKHalf, MapKind::Ramp, true, true, p, kPkPerOpt>),    \
                               grid_per, dim3(64 * kPkPerWpb), 0, stream, A);                                         \
        else                                                                                                          \
            hipLaunchKernelGGL(                                                                                       \
                (stft8192_pk_kernel<kSrcRender, kKHalf, MapKind::Ramp, true, true, p, kPkPerOpt | kPkNoReuse>),       \
                grid_per, dim3(64 * kPkPerWpb), 0, stream, A);                                                        \
    } while (0)
        const uint64_t groups_per = (A.run_waves + tail + kPkPerWpb - 1) / kPkPerWpb;
        if (groups_per > 0x7fffffffull) return DSP_ERR_INVALID;
        const dim3 grid_per((uint32_t)groups_per, C);
        switch (per) {
        case 1: DSPB_PK_PER(1); break;
        case 2: DSPB_PK_PER(2); break;
        case 4: DSPB_PK_PER(4); break;
        case 8: DSPB_PK_PER(8); break;
        case 16: DSPB_PK_PER(16); break;
        default: DSPB_PK_PER(0); break;
        }
#undef DSPB_PK_PER
        DSPB_HIP(hipGetLastError());
        return DSP_OK;
    }
    if (opt && !fused && winc) {  // memory-source A/B variants (the tools build only)
        int st = DSP_OK;
        if (stft_pk_ab_dispatch(A, C, fused, opt, grid, stream, &st)) return st;
    }
    return launch_pk_paths(A, fused, km, pow2, winc, grid, stream);
}

// The store-only launch of a call whose spectrum row is cached (stft_pk.hpp
// stft8192_rows_kernel; in this translation unit, so that a cold headline
// call still loads one code object): A as for launch_stft8192_pk on the PER
// path with H % B == 0, A.run frames per wave, `row` the call's 4097 cached
// magnitudes.  `pace` (row_pace_valid) is the launch's pacing: an LDS pad
// beside the kernel's 16,640 B tile leaves pace.waves one-wave workgroups to a
// CU's 160 KB (the tile alone: 9), and every wave sleeps pace.nap units between
// its two bursts.  `done`, when set, is an event that completes with the launch
// (the launch's own completion signal: no packet of its own follows it).
bool row_pace_valid(uint32_t pace) {
    const uint32_t nap = pace & 0xffu, waves = (pace >> 8) & 0xffu;
    return !(pace & ~(0xffffu | kRowPaceRecord)) && nap <= kRowPaceMaxNap && waves >= kRowPaceMinWaves && waves <= 9u;
}
int launch_stft8192_rows(const Stft8kArgs &A_, uint32_t C, const float *row, uint32_t pace, hipEvent_t done,
                         hipStream_t stream) {
    if (A_.F == 0 || C == 0) return DSP_OK;
    Stft8kArgs A = A_;
    if (!row || !stft8192_pk_per_path(A, true) || A.H % A.map.B != 0 || A.H % 128u != 0 || A.H > 8192u ||
        !row_pace_valid(pace))
        return DSP_ERR_INVALID;
    const uint32_t nap = pace & 0xffu, waves = (pace >> 8) & 0xffu;
    constexpr uint32_t kLdsPerCu = 160u << 10, kTile = 64u * 65u * 4u;
    const uint32_t pad = waves >= 9u ? 0u : (kLdsPerCu / waves - kTile) & ~255u;  // (waves >= 3: within 64 KB)
    if (A.run == 0) A.run = 1;
    A.run_waves = (A.F + A.run - 1) / A.run;
    const uint64_t tail = A.tail_end > A.F * A.H ? (A.tail_end - A.F * A.H + A.H - 1) / A.H : 0;
    if (A.run_waves + tail > 0x7fffffffull) return DSP_ERR_INVALID;
    const dim3 grid((uint32_t)(A.run_waves + tail), C);
#define DSPB_PK_ROWS(p)                                                                                               \
    hipExtLaunchKernelGGL((stft8192_rows_kernel<p>), grid, dim3(64), pad, stream, nullptr, done, 0, A, row, nap)
    switch (A.map.B <= 128u ? 1u : A.map.B / 128u) {  // the block table's period in 128 samples
    case 1: DSPB_PK_ROWS(1); break;
    case 2: DSPB_PK_ROWS(2); break;
    case 4: DSPB_PK_ROWS(4); break;
    case 8: DSPB_PK_ROWS(8); break;
    case 16: DSPB_PK_ROWS(16); break;
    default: return DSP_ERR_INVALID;
    }
#undef DSPB_PK_ROWS
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

// The product library has no A/B variants: these weak definitions stand
// unless the tools build (make ab) links stft_pk_ab.hip, which defines both.
__attribute__((weak)) bool stft_pk_ab_dispatch(const Stft8kArgs &, uint32_t, bool, int, dim3, hipStream_t, int *) {
    return false;
}
__attribute__((weak)) int stft_pk_ab_options() { return 0; }

}  // namespace dspb
