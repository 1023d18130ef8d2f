// pvoc.hip -- dsp_pvoc: the phase-vocoder recurrence along the frame axis of a
// spectrogram in dsp_stft's layout (dspbench.h has the definition).
//
// A wavefront owns 64 neighbouring bins -- one 512-byte run of (re, im) pieces
// of a frame, as in stft_cx.hip -- and walks a chunk of kPvocChunk output
// frames.  Bins 0..4095 are 64 such runs; bin 4096 is a 65th run with one
// active lane.  A workgroup is four runs; the grid is (chunks, 17, rows).
//
// The phase of a bin is a 32-bit fixed-point fraction of a turn.  The argument
// of every input bin is taken once per loaded frame, in float32, and rounded to
// that format; an increment is the wrapping integer difference of two of them
// (0 where either bin is 0), and the phase is their wrapping integer sum.
// Integer addition is associative, so the sum over the output frames may be cut
// into chunks anywhere:
//   sums    chunk c < chunks - 1: the sum of its increments -> S[row][c][bin]
//   carry   one thread per (row, bin): S[row][c] <- arg Z[0] + sum_{c' < c} S[row][c']
//   frames  chunk c: the increments again, the phase carried from S[row][c],
//           Z'[t] = mag_t (cos, sin) stored once as 8-byte pieces
// and every cut gives the same bits.  No workgroup waits for another, and there
// are no atomics.  The frames launch forms the increments again and does not
// read them back: it must read Z for the magnitudes in any case, so a scratch
// of increments would add 8 bytes of traffic per output bin to save arithmetic
// the launch has to spare.
//
// Inside a chunk a lane keeps the two frames f, f + 1 it interpolates between:
// at rate <= 1 the same pair repeats or f + 1 becomes the next f, and only one
// new frame is loaded; no frame is loaded twice in a chunk.
//
// tools/pvoc_model.py pvoc32 is the float32 model of this arithmetic.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "pvoc_host.hpp"

namespace dspb {

typedef float v2f_pv __attribute__((ext_vector_type(2)));

// chunks of one launch: 2^22 blocks of 256 threads in x
constexpr uint64_t kPvocLaunchChunks = 1ull << 22;
constexpr uint32_t kPvocRuns = 65;  // 64 runs of 64 bins, and bin 4096

// atan(u) / (2 pi u) over |u| <= tan(pi / 8), in u^2 (least squares on Chebyshev nodes;
// 2.5e-9 turns with the float coefficients)
__device__ __forceinline__ float atan_turns_poly(float w) {
    float p = 0.012708066962659359f;
    p = __fmaf_rn(p, w, -0.0220451932400465f);
    p = __fmaf_rn(p, w, 0.03179024159908295f);
    p = __fmaf_rn(p, w, -0.05305079370737076f);
    return __fmaf_rn(p, w, 0.15915493667125702f);
}

// arg (re + i im) as a 32-bit fixed-point fraction of a turn; arg 0 = 0.  The
// octant's angle is a float in [0, 1/8] rounded once to the format; the folds
// into the other octants are exact integer steps, so +1/2 and -1/2 turn are the
// same word.  Only the ratio min / max of |re|, |im| enters: scaling both by a
// power of two changes nothing (underflow aside).
__device__ __forceinline__ uint32_t arg_fix(float re, float im) {
    const float ax = __builtin_fabsf(re), ay = __builtin_fabsf(im);
    const float mx = __builtin_fmaxf(ax, ay), mn = __builtin_fminf(ax, ay);
    if (mx == 0.f) return 0u;
    const float t = __fdiv_rn(mn, mx);  // [0, 1]
    const bool hi = t > 0.41421357f;    // atan t = pi / 4 + atan((t - 1) / (t + 1))
    const float u = hi ? __fdiv_rn(t - 1.f, t + 1.f) : t;
    const float r = __fmaf_rn(u, atan_turns_poly(u * u), hi ? 0.125f : 0.f);  // [0, 1/8] turns
    uint32_t a = (uint32_t)__float2int_rn(r * 4294967296.f);                   // <= 2^29
    if (ay > ax) a = 0x40000000u - a;
    if (re < 0.f) a = 0x80000000u - a;
    if (im < 0.f) a = 0u - a;
    return a;
}

// (cos, sin) of a fixed-point phase: the nearest quarter turn is taken off in
// integers, exactly; what is left, within 1/8 turn, goes through two polynomials
// in turns (sin 2 pi x / x and cos 2 pi x in x^2: 2.4e-8 and 6.7e-9 absolute)
__device__ __forceinline__ v2f_pv cos_sin_fix(uint32_t p) {
    const uint32_t q = (p + 0x20000000u) >> 30;
    const int32_t r = (int32_t)(p - (q << 30));  // [-2^29, 2^29)
    const float x = (float)r * 0x1p-32f, w = x * x;
    float s = -75.4017105102539f;
    s = __fmaf_rn(s, w, 81.59254455566406f);
    s = __fmaf_rn(s, w, -41.3416633605957f);
    s = __fmaf_rn(s, w, 6.2831854820251465f);
    s = s * x;
    float c = 59.22018814086914f;
    c = __fmaf_rn(c, w, -85.4428482055664f);
    c = __fmaf_rn(c, w, 64.93931579589844f);
    c = __fmaf_rn(c, w, -19.739208221435547f);
    c = __fmaf_rn(c, w, 1.0f);
    switch (q & 3u) {
    case 0u: return v2f_pv{c, s};
    case 1u: return v2f_pv{0.f - s, c};
    case 2u: return v2f_pv{0.f - c, 0.f - s};
    default: return v2f_pv{s, 0.f - c};
    }
}

// A/B variants (DSP_DEBUG_PVOC_VARIANT; the product is 0): DESIGN 4.5i has what each measured
constexpr uint32_t kPvProduct = 1;  // an increment is one argument of the fma-formed product, per output frame
constexpr uint32_t kPvHwTrig = 2;   // cos and sin by the hardware's turn-based instructions
constexpr uint32_t kPvStored = 4;   // the sums launch stores every increment, the frames launch reads them back

// (cos, sin) by v_cos_f32 / v_sin_f32, whose argument is in turns
__device__ __forceinline__ v2f_pv cos_sin_hw(uint32_t p) {
    const float x = (float)(int32_t)p * 0x1p-32f;  // [-1/2, 1/2]
    return v2f_pv{__builtin_amdgcn_cosf(x), __builtin_amdgcn_sinf(x)};
}

// what a lane keeps of one input bin
struct PvBin {
    uint32_t arg;
    float mag;
    uint32_t nz;   // the bin is not 0
    float re, im;  // kPvProduct only
};

template <bool MAG, bool ARG>
__device__ __forceinline__ PvBin pv_bin(v2f_pv z) {
    PvBin b;
    b.arg = ARG ? arg_fix(z.x, z.y) : 0u;
    b.mag = MAG ? __fsqrt_rn(__fmaf_rn(z.x, z.x, z.y * z.y)) : 0.f;
    b.nz = (z.x != 0.f || z.y != 0.f) ? 1u : 0u;
    b.re = z.x, b.im = z.y;
    return b;
}

// a lane's bin of the frames f, f + 1 of its row; frames at and past F are 0
template <bool MAG, bool ARG>
struct PvPair {
    const float *row;
    uint64_t ld, F, f;
    uint32_t k, active;
    PvBin b0, b1;

    __device__ __forceinline__ PvBin load(uint64_t fr) const {
        v2f_pv z{0.f, 0.f};
        if (active && fr < F) z = reinterpret_cast<const v2f_pv *>(row + fr * ld)[k];
        return pv_bin<MAG, ARG>(z);
    }
    __device__ __forceinline__ void start(uint64_t fn) {
        b0 = load(fn);
        b1 = load(fn + 1);
        f = fn;
    }
    // fn >= f, the same for every lane of the wavefront
    __device__ __forceinline__ void seek(uint64_t fn) {
        if (fn == f) return;
        b0 = fn == f + 1 ? b1 : load(fn);
        b1 = load(fn + 1);
        f = fn;
    }
    __device__ __forceinline__ uint32_t increment() const { return (b0.nz & b1.nz) ? b1.arg - b0.arg : 0u; }
    // arg(Z[f + 1] conj Z[f]) of the fma-formed product (arg 0 = 0)
    __device__ __forceinline__ uint32_t increment_of_product() const {
        const float pr = __fmaf_rn(b1.re, b0.re, b1.im * b0.im), pi = __fmaf_rn(b1.im, b0.re, 0.f - b1.re * b0.im);
        return arg_fix(pr, pi);
    }
};

// the input position of output frame t: one float64 product (pvoc_host.hpp pvoc_position)
__device__ __forceinline__ uint64_t pv_frame(uint64_t t, double rate, float *frac) {
    const double s = __dmul_rn((double)t, rate);
    const uint64_t f = (uint64_t)s;
    *frac = (float)(s - (double)f);
    return f;
}

__device__ __forceinline__ bool pv_lane(uint32_t *k, uint32_t *active) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t run = blockIdx.y * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    *k = run * 64u + lane;
    *active = *k < kStftCxBins ? 1u : 0u;
    return run < kPvocRuns;
}

// grid (chunks of this launch, 17, rows): chunk c0 + blockIdx.x < chunks - 1 (kPvStored: < chunks)
template <uint32_t OPT>
__global__ __launch_bounds__(256) void pvoc_sums_kernel(PvocArgs A) {
    uint32_t k, active;
    if (!pv_lane(&k, &active)) return;
    const uint32_t row = blockIdx.z;
    const uint64_t c = A.c0 + blockIdx.x;
    const uint64_t t0 = c * A.chunk;
    const uint64_t t1 = t0 + A.chunk < A.frames_out ? t0 + A.chunk : A.frames_out;  // (short in the last chunk only)
    PvPair<false, !(OPT & kPvProduct)> P{A.in.p[row], A.ld_in, A.F, 0, k, active, {}, {}};
    float a;
    P.start(pv_frame(t0, A.rate, &a));
    uint32_t sum = 0u;
    for (uint64_t t = t0; t < t1; ++t) {
        P.seek(pv_frame(t, A.rate, &a));
        const uint32_t inc = (OPT & kPvProduct) ? P.increment_of_product() : P.increment();
        if ((OPT & kPvStored) && active) A.inc[((uint64_t)row * A.frames_out + t) * kStftCxBins + k] = inc;
        sum += inc;
    }
    if (active) A.S[((uint64_t)row * A.chunks + c) * kStftCxBins + k] = sum;
}

// grid (17, rows): one thread per (bin, row); S[row][c] becomes the phase at chunk c's first frame
__global__ __launch_bounds__(256) void pvoc_carry_kernel(PvocArgs A) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, row = blockIdx.y;
    if (k >= kStftCxBins) return;
    const v2f_pv z0 = reinterpret_cast<const v2f_pv *>(A.in.p[row])[k];
    uint32_t run = arg_fix(z0.x, z0.y);
    uint32_t *p = A.S + (uint64_t)row * A.chunks * kStftCxBins + k;
    uint64_t c = 0;
    // eight sums in flight; the last chunk's sum is not needed and its slot is only written
    for (; c + 8 < A.chunks; c += 8) {
        uint32_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[(c + j) * kStftCxBins];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            p[(c + j) * kStftCxBins] = run;
            run += v[j];
        }
    }
    for (; c < A.chunks; ++c) {
        const uint32_t v = c + 1 < A.chunks ? p[c * kStftCxBins] : 0u;
        p[c * kStftCxBins] = run;
        run += v;
    }
}

// grid (chunks of this launch, 17, rows)
template <uint32_t OPT>
__global__ __launch_bounds__(256) void pvoc_frames_kernel(PvocArgs A) {
    uint32_t k, active;
    if (!pv_lane(&k, &active)) return;
    const uint32_t row = blockIdx.z;
    const uint64_t c = A.c0 + blockIdx.x;
    const uint64_t t0 = c * A.chunk;
    const uint64_t t1 = t0 + A.chunk < A.frames_out ? t0 + A.chunk : A.frames_out;
    PvPair<true, !(OPT & (kPvProduct | kPvStored))> P{A.in.p[row], A.ld_in, A.F, 0, k, active, {}, {}};
    uint32_t phase = active ? A.S[((uint64_t)row * A.chunks + c) * kStftCxBins + k] : 0u;
    float a;
    P.start(pv_frame(t0, A.rate, &a));
    float *o = A.out.p[row] + t0 * A.ld_out;
    for (uint64_t t = t0; t < t1; ++t, o += A.ld_out) {
        P.seek(pv_frame(t, A.rate, &a));
        const float mag = __fmaf_rn(a, P.b1.mag, (1.f - a) * P.b0.mag);
        const v2f_pv cs = (OPT & kPvHwTrig) ? cos_sin_hw(phase) : cos_sin_fix(phase);
        if (active) __builtin_nontemporal_store(v2f_pv{mag * cs.x, mag * cs.y}, reinterpret_cast<v2f_pv *>(o) + k);
        if (OPT & kPvStored) phase += active ? A.inc[((uint64_t)row * A.frames_out + t) * kStftCxBins + k] : 0u;
        else phase += (OPT & kPvProduct) ? P.increment_of_product() : P.increment();
    }
}

template <uint32_t OPT>
static int launch_pvoc_opt(const PvocArgs &A, hipStream_t s) {
    const uint32_t groups = (kPvocRuns + 3u) / 4u;
    const uint64_t nsum = (OPT & kPvStored) ? A.chunks : A.chunks - 1;  // chunks the sums launch walks
    for (uint64_t c0 = 0; c0 < nsum; c0 += kPvocLaunchChunks) {
        PvocArgs G = A;
        G.c0 = c0;
        const uint64_t n = std::min<uint64_t>(nsum - c0, kPvocLaunchChunks);
        hipLaunchKernelGGL(pvoc_sums_kernel<(OPT & (kPvProduct | kPvStored))>, dim3((uint32_t)n, groups, A.cn), dim3(256), 0,
                           s, G);
        DSPB_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(pvoc_carry_kernel, dim3((kStftCxBins + 255u) / 256u, A.cn), dim3(256), 0, s, A);
    DSPB_HIP(hipGetLastError());
    for (uint64_t c0 = 0; c0 < A.chunks; c0 += kPvocLaunchChunks) {
        PvocArgs G = A;
        G.c0 = c0;
        const uint64_t n = std::min<uint64_t>(A.chunks - c0, kPvocLaunchChunks);
        hipLaunchKernelGGL(pvoc_frames_kernel<OPT>, dim3((uint32_t)n, groups, A.cn), dim3(256), 0, s, G);
        DSPB_HIP(hipGetLastError());
    }
    return DSP_OK;
}

int launch_pvoc(const PvocArgs &A, hipStream_t s) {
    if (A.cn == 0 || A.cn > (uint32_t)kMaxChannels || A.F == 0 || A.frames_out == 0 || A.chunk == 0 ||
        A.chunks != (A.frames_out + A.chunk - 1) / A.chunk || !A.S || A.variant > 7u ||
        ((A.variant & kPvStored) && !A.inc))
        return DSP_ERR_INVALID;
    switch (A.variant) {
    case 0u: return launch_pvoc_opt<0u>(A, s);
    case 1u: return launch_pvoc_opt<1u>(A, s);
    case 2u: return launch_pvoc_opt<2u>(A, s);
    case 3u: return launch_pvoc_opt<3u>(A, s);
    case 4u: return launch_pvoc_opt<4u>(A, s);
    case 5u: return launch_pvoc_opt<5u>(A, s);
    case 6u: return launch_pvoc_opt<6u>(A, s);
    default: return launch_pvoc_opt<7u>(A, s);
    }
}

}  // namespace dspb
