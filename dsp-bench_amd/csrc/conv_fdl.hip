// conv_fdl.hip -- DSP_PLUGIN_CONV: convolution with a long impulse response
// (up to 2^20 taps) by uniform partitioned overlap-save, a frequency-domain
// delay line over 8192-point real frames.
//
// The taps are cut into partitions of kConvHop = 4096; H_p is the spectrum of
// partition p zero-padded to 8192 (host_tables.cpp conv_table).  Frame f
// covers input [4096 (f - 1), 4096 (f + 1)), zero before sample 0 and past L,
// and owns outputs [4096 f, 4096 (f + 1)): the upper half of the circular
// convolution of a frame with a 4096-tap partition is the linear one.  Three
// launches on the call's stream:
//
//   forward   one wavefront per (frame, channel): the 8192-point real FFT of
//             fir_fft.hip (ols_frame.hpp) up to the split, X_f to scratch
//   MAC       Y_f[k] = sum_{p < partitions} H_p[k] X_{f-p}[k] (f - p >= 0):
//             a complex FIR along the frame axis, independent per bin
//   inverse   one wavefront per (frame, channel): the inverse split and the
//             packed 4096-point inverse, the upper 4096 samples stored
//
// A spectrum is kConvSpec4 = 2112 float4 in the register order the split
// leaves it in -- the product is pointwise, so nothing is ever transposed to
// natural order: float4 [2 (64 ka + l) + h], ka < 16, holds the bins
// k = l + 64 ka and k + 1024 (h = 0) or M - k and M - k - 1024 (h = 1, M =
// 4096; at k = 0 that is bin 4096) as (re, re, im, im), ols_table's layout;
// then one more slice of 64 float4 whose first holds bin 2048 (the self-paired
// bin of the split) as (re, 0, im, 0), the rest zero.  The padding slice costs
// 3% of the traffic and keeps the MAC one uniform pointwise kernel.
//
// tools/conv_model.py is the float32 model of this partition arithmetic.
#include "ols_frame.hpp"

namespace dspb {

static_assert(kConvSpec4 == 2048 + 64, "a spectrum: 32 slices of the split's pairs and the bin-2048 slice");
constexpr uint32_t kConvSlices = kConvSpec4 / 64;  // 33 wave-wide float4 slices

__device__ __forceinline__ float4 *conv_spectrum(float4 *base, uint32_t ch, uint64_t F, uint64_t f) {
    return base + ((uint64_t)ch * F + f) * kConvSpec4;
}

// ---------------------------------------------------------------------------
// forward: X_f = split(FFT(frame f)) -> scratch
// ---------------------------------------------------------------------------
template <bool EDGE>
__device__ __forceinline__ void conv_forward_frame(const ConvArgs &A, uint64_t f, uint32_t ch, float *lds,
                                                   uint32_t lane) {
    const int64_t fs = (int64_t)(f * kConvHop) - (int64_t)kConvHop;  // even
    const float *x = (ch < A.in_ch) ? A.in.p[ch] : nullptr;

    cx tlo[8];
    cx2 thp[4];
    load_stage_tw(A.tw, lane, 0u, tlo, thp);
    cx2 P[32];
    ols_load_frame<EDGE>(x, fs, A.L, lane, P);
    cx zp[32], zm[32];
    fft4096_pk<false, false, false, true>(P, lds, tlo, thp, lane, zp, zm);

    const OlsLane ln = ols_lane(A.tw, lane);
    float4 *o = conv_spectrum(A.X, ch, A.F, f);
#pragma unroll
    for (int ka = 0; ka < 16; ++ka) {
        cx2 X1, X2;
        ols_split(zp, zm, ka, ln, ols_tw(ln, ka), X1, X2);
        float4 *q = o + 2u * (64u * (uint32_t)ka + lane);
        q[0] = float4{X1.r.x, X1.r.y, X1.i.x, X1.i.y};     // 2 X[k]
        q[1] = float4{X2.r.x, X2.r.y, -X2.i.x, -X2.i.y};   // 2 X[M - k]
    }
    // bin 2048: Z[2048] = zm[0] of lane 0, 2 X[2048] = 2 conj Z
    const cx Z = zm[0];
    o[2048u + lane] = ln.l0 ? float4{2.f * Z.r, 0.f, -2.f * Z.i, 0.f} : float4{0.f, 0.f, 0.f, 0.f};
}

// grid (frame groups of 4, channels); LDS: four 64 x 33 transpose tiles
__global__ __launch_bounds__(256, 2) void conv_forward_kernel(ConvArgs A) {
    __shared__ __attribute__((aligned(16))) float lds_all[4][64 * 33];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ch = blockIdx.y;
    const uint64_t f = (uint64_t)xcd_remap(blockIdx.x, gridDim.x) * 4u + wave;
    if (f >= A.F) return;
    // interior frames: [1, fe) with 4096 (f + 1) <= L (a wave-uniform branch)
    if (f == 0 || (f + 1) * kConvHop > A.L) conv_forward_frame<true>(A, f, ch, lds_all[wave], lane);
    else conv_forward_frame<false>(A, f, ch, lds_all[wave], lane);
}

// ---------------------------------------------------------------------------
// multiply-accumulate over partitions
// ---------------------------------------------------------------------------
// A wave owns one slice (a float4 per lane: 128 bins) of a run of kConvRun
// consecutive frames f0 .. f0 + R - 1 of one channel.  It keeps R complex
// accumulators and a window of R filter values in registers and walks the
// input frames j = f0 - partitions + 1 .. f0 + R - 1: at step j the window
// holds w[r] = H_{f0 + r - j} (zero outside [0, partitions)), X_j is loaded
// once and accumulated into all R outputs, then the window moves by one
// partition.  Every X and H slice loaded is used R times, so the kernel reads
// (partitions + R - 1 + partitions) / R slices per output slice instead of
// 2 partitions.  The loop is unrolled R times so that the window rotates by
// register renaming; steps past the last frame run with X = 0 rather than a
// branch, so the loads of a whole unrolled body are in flight together.
constexpr int kConvRun = 8;

__device__ __forceinline__ cx2 as_cx2(float4 q) { return cx2{v2f{q.x, q.y}, v2f{q.z, q.w}}; }

__global__ __launch_bounds__(192) void conv_fdl_kernel(ConvArgs A) {
    constexpr int R = kConvRun;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t sl = blockIdx.y * 3u + wave;  // < kConvSlices = 3 gridDim.y
    const uint32_t ch = blockIdx.z;
    // neighbouring runs of a channel read the same X frames and the same H:
    // consecutive logical indices on one XCD share its L2
    const int64_t f0 = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * R;
    const int64_t F = (int64_t)A.F, P = (int64_t)A.parts;
    const uint32_t off = 64u * sl + lane;
    const float4 *H = A.H + off;
    const float4 *X = A.X + (uint64_t)ch * A.F * kConvSpec4 + off;

    const int64_t jlo = f0 - (P - 1) > 0 ? f0 - (P - 1) : 0;
    const int64_t jhi = f0 + R - 1 < F - 1 ? f0 + R - 1 : F - 1;

    const cx2 zero = cx2{v2f{0.f, 0.f}, v2f{0.f, 0.f}};
    cx2 acc[R], w[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        acc[r] = zero;
        const int64_t p = f0 + r - jlo;  // >= 0
        const cx2 h = as_cx2(H[(uint64_t)(p < P ? p : P - 1) * kConvSpec4]);
        w[r] = p < P ? h : zero;
    }
    for (int64_t jb = jlo; jb <= jhi; jb += R) {
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int64_t j = jb + u;
            // step j (logical w[r] lives in w[(r - u) mod R]); past jhi: X = 0
            cx2 x = as_cx2(X[(uint64_t)(j <= jhi ? j : jhi) * kConvSpec4]);
            if (j > jhi) x = zero;
            // the partition entering the window for step j + 1: H_{f0 - j - 1}
            const int64_t pn = f0 - j - 1;  // <= P - 2
            cx2 hn = as_cx2(H[(uint64_t)(pn >= 0 ? pn : 0) * kConvSpec4]);
            if (pn < 0) hn = zero;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const cx2 h = w[(r - u + R) % R];
                acc[r].r = acc[r].r + h.r * x.r;
                acc[r].r = acc[r].r - h.i * x.i;
                acc[r].i = acc[r].i + h.r * x.i;
                acc[r].i = acc[r].i + h.i * x.r;
            }
            w[(R - 1 - u) % R] = hn;  // the slot of logical w[R - 1], which leaves
        }
    }
    float4 *Y = A.Y + (uint64_t)ch * A.F * kConvSpec4 + off;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (f0 + r < F) Y[(uint64_t)(f0 + r) * kConvSpec4] = float4{acc[r].r.x, acc[r].r.y, acc[r].i.x, acc[r].i.y};
}

// ---------------------------------------------------------------------------
// inverse: y[4096 f ..) = upper half of IFFT(unsplit(Y_f))
// ---------------------------------------------------------------------------
__device__ __forceinline__ void conv_inverse_frame(const ConvArgs &A, uint64_t f, uint32_t ch, float *lds,
                                                   uint32_t lane) {
    const OlsLane ln = ols_lane(A.tw, lane);
    const float4 *y = conv_spectrum(A.Y, ch, A.F, f);
    cx zk[32], zr[32];
#pragma unroll
    for (int ka = 0; ka < 16; ++ka) {
        const float4 *q = y + 2u * (64u * (uint32_t)ka + lane);
        ols_unsplit(as_cx2(q[0]), as_cx2(q[1]), ols_tw(ln, ka), ka, ln, zk, zr);
    }
    {
        const float4 q = y[2048u + lane];  // lane 0's: bin 2048
        ols_unsplit_lane0(cx{q.x, q.z}, ln, zr);
    }
    cx tlo[8];
    cx2 thp[4];
    // (packed in place: as a helper taking zk / zr by reference this loop kept
    // them in scratch memory)
    cx2 Q[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const cx u0 = 2 * j < 32 ? zk[2 * j] : zr[2 * j - 32];
        const cx u1 = 2 * j + 1 < 32 ? zk[2 * j + 1] : zr[2 * j + 1 - 32];
        Q[j] = cx2{v2f{u0.r, u1.r}, v2f{u0.i, u1.i}};
    }
    cx yp[32], ym[32];
    load_stage_tw(A.tw, lane, 0u, tlo, thp);
    fft4096_pk<true, false, false, true>(Q, lds, tlo, thp, lane, yp, ym);

    // outputs: m = l + 64 b, b >= 32 -> y[4096 f + 2l + 128 (b - 32)]
    float *o = A.out.p[ch];
    const uint64_t ob = f * kConvHop + 2u * lane;
    if (f * kConvHop + kConvHop <= A.Ly) {
#pragma unroll
        for (int b = 0; b < 32; ++b)
            __builtin_nontemporal_store(v2f{ym[b].r, ym[b].i}, reinterpret_cast<v2f *>(o + ob + 128u * (uint32_t)b));
    } else {
#pragma unroll
        for (int b = 0; b < 32; ++b) {
            const uint64_t i = ob + 128u * (uint32_t)b;
            if (i < A.Ly) o[i] = ym[b].r;
            if (i + 1 < A.Ly) o[i + 1] = ym[b].i;
        }
    }
}

__global__ __launch_bounds__(256, 2) void conv_inverse_kernel(ConvArgs A) {
    __shared__ __attribute__((aligned(16))) float lds_all[4][64 * 33];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ch = blockIdx.y;
    const uint64_t f = (uint64_t)xcd_remap(blockIdx.x, gridDim.x) * 4u + wave;
    if (f >= A.F) return;
    conv_inverse_frame(A, f, ch, lds_all[wave], lane);
}

// C <= kMaxChannels channels of one group; A.X and A.Y hold C F spectra each
int launch_conv(const ConvArgs &A, uint32_t C, hipStream_t s) {
    if (A.F == 0 || C == 0) return DSP_OK;
    const uint64_t groups = (A.F + 3) / 4, runs = (A.F + kConvRun - 1) / kConvRun;
    if (groups > 0x7fffffffull) return DSP_ERR_INVALID;
    hipLaunchKernelGGL(conv_forward_kernel, dim3((uint32_t)groups, C), dim3(256), 0, s, A);
    DSPB_HIP(hipGetLastError());
    hipLaunchKernelGGL(conv_fdl_kernel, dim3((uint32_t)runs, kConvSlices / 3, C), dim3(192), 0, s, A);
    DSPB_HIP(hipGetLastError());
    hipLaunchKernelGGL(conv_inverse_kernel, dim3((uint32_t)groups, C), dim3(256), 0, s, A);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

}  // namespace dspb
