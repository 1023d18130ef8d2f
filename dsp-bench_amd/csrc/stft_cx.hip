// stft_cx.hip -- dsp_stft and dsp_istft: the complex 8192-point STFT and its
// overlap-add inverse, assembled from the pieces of welch.hip (the forward
// frame) and conv_fdl.hip (the inverse frame).
//
//   forward   one wavefront per (frame, row): the window at load, the
//             8192-point real FFT of ols_frame.hpp up to the split.  In the
//             split's register order lane l at step ka holds the bins
//             kk = l + 64 (ka + 16 c), c = 0, 1 (X1) and 4096 - kk (X2): 64
//             lanes hold 64 neighbouring bins, so each of the four is stored as
//             one 512-byte run of (re, im) pieces straight from registers, in
//             natural bin order.  The split leaves 2 X; X is stored (the
//             halving is exact).  No scratch, no second launch.
//   inverse   per chunk of frames (stft_cx_host.hpp istft_chunk), two launches:
//     frames  one wavefront per (frame, row): the same four runs loaded, scaled
//             by 2^-13 (the inverse's 1 / 4096 and the two real-split halvings),
//             the inverse split and the packed 4096-point inverse give all 8192
//             samples of v_f; w v_f goes to the scratch, [row][slot][8192]
//     ola     one thread per output sample: num = sum w v_f and den = sum w^2
//             over the at most 16 frames that cover it, in ascending frame
//             order, then one division.  Every frame a sample needs is in the
//             chunk's slots, so no sum straddles two launches and there are no
//             atomics: the same bits on every run, whatever C is.
//
// tools/stft_model.py is the float32 model of this order.
#include "ols_frame.hpp"
#include "stft_cx_host.hpp"

namespace dspb {

constexpr float kIstftScale = 1.0f / 8192.0f;  // spec -> the inverse split's input
// frames of one forward launch: 2^22 blocks of 256 threads, 2^30 work-items in
// x (a launch's global size in one dimension must stay below 2^32)
constexpr uint64_t kLaunchFrames = 4ull << 22;

__device__ __forceinline__ void store_bin(float *o, uint32_t k, float re, float im) {
    __builtin_nontemporal_store(v2f{re, im}, reinterpret_cast<v2f *>(o) + k);
}

// grid (frame groups of 4, rows); LDS: four 64 x 33 transpose tiles
__global__ __launch_bounds__(256, 2) void stft_cx_forward_kernel(StftCxArgs A) {
    __shared__ __attribute__((aligned(16))) float lds_all[4][64 * 33];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t row = blockIdx.y;
    const uint32_t f = xcd_remap(blockIdx.x, gridDim.x) * 4u + wave;  // of this launch: nf <= kLaunchFrames
    if (f >= A.nf) return;
    const float *x = A.in.p[row] + (A.f0 + f) * (uint64_t)A.H;

    cx tlo[8];
    cx2 thp[4];
    load_stage_tw(A.tw, lane, 0u, tlo, thp);
    cx2 P[32];
    welch_load_frame(x, A.win2, lane, P);
    cx zp[32], zm[32];
    fft4096_pk<false, false, false, true>(P, lds_all[wave], tlo, thp, lane, zp, zm);

    const OlsLane ln = ols_lane(A.tw, lane);
    float *o = A.spec.p[row] + (A.f0 + f) * A.ld;
#pragma unroll
    for (int ka = 0; ka < 16; ++ka) {
        cx2 X1, X2;  // 2 X[k], conj 2 X[4096 - k] for k = kk, kk + 1024
        ols_split(zp, zm, ka, ln, ols_tw(ln, ka), X1, X2);
        const uint32_t kk = lane + 64u * (uint32_t)ka;
        // X = half of what the split leaves (exact); the M - k half is stored conjugated back
        const v2f ar = 0.5f * X1.r, ai = 0.5f * X1.i, br = 0.5f * X2.r, bi = v2f{0.f, 0.f} - 0.5f * X2.i;
        // bins 0 and 4096 (lane 0 at ka = 0) are real: +0
        const bool ends = ka == 0 && ln.l0;
        store_bin(o, kk, ar.x, ends ? 0.f : ai.x);
        store_bin(o, kk + 1024u, ar.y, ai.y);
        store_bin(o, 4096u - kk, br.x, ends ? 0.f : bi.x);
        store_bin(o, 3072u - kk, br.y, bi.y);
    }
    // bin 2048: Z[2048] = zm[0] of lane 0, X[2048] = conj Z
    if (ln.l0) store_bin(o, 2048u, zm[0].r, 0.f - zm[0].i);
}

int launch_stft_cx(const StftCxArgs &A, hipStream_t s) {
    if (A.nf == 0 || A.cn == 0 || A.cn > (uint32_t)kMaxChannels) return DSP_ERR_INVALID;
    for (uint64_t f0 = 0; f0 < A.nf; f0 += kLaunchFrames) {
        StftCxArgs G = A;
        G.f0 = A.f0 + f0;
        G.nf = A.nf - f0 < kLaunchFrames ? A.nf - f0 : kLaunchFrames;
        hipLaunchKernelGGL(stft_cx_forward_kernel, dim3((uint32_t)((G.nf + 3) / 4), A.cn), dim3(256), 0, s, G);
        DSPB_HIP(hipGetLastError());
    }
    return DSP_OK;
}

// grid (slot groups of 4, rows)
__global__ __launch_bounds__(256, 2) void istft_frame_kernel(IstftArgs A) {
    __shared__ __attribute__((aligned(16))) float lds_all[4][64 * 33];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t row = blockIdx.y;
    const uint32_t slot = xcd_remap(blockIdx.x, gridDim.x) * 4u + wave;
    if (slot >= A.ns) return;
    const v2f *p = reinterpret_cast<const v2f *>(A.spec.p[row] + (A.fa + slot) * A.ld);

    const OlsLane ln = ols_lane(A.tw, lane);
    cx zk[32], zr[32];
#pragma unroll
    for (int ka = 0; ka < 16; ++ka) {
        const uint32_t kk = lane + 64u * (uint32_t)ka;
        const v2f a0 = p[kk], a1 = p[kk + 1024u], b0 = p[4096u - kk], b1 = p[3072u - kk];
        // bins 0 and 4096 (lane 0 at ka = 0) by their real part only
        const bool ends = ka == 0 && ln.l0;
        const cx2 Yk = cx2{v2f{a0.x, a1.x} * kIstftScale, v2f{ends ? 0.f : a0.y, a1.y} * kIstftScale};
        const cx2 YMk = cx2{v2f{b0.x, b1.x} * kIstftScale, v2f{ends ? 0.f : b0.y, b1.y} * kIstftScale};
        ols_unsplit(Yk, YMk, ols_tw(ln, ka), ka, ln, zk, zr);
    }
    {
        const v2f q = p[2048u];  // every lane reads it, lane 0 uses it
        ols_unsplit_lane0(cx{q.x * kIstftScale, q.y * kIstftScale}, ln, zr);
    }
    cx tlo[8];
    cx2 thp[4];
    // (packed in place, as conv_fdl.hip's inverse does)
    cx2 Q[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const cx u0 = 2 * j < 32 ? zk[2 * j] : zr[2 * j - 32];
        const cx u1 = 2 * j + 1 < 32 ? zk[2 * j + 1] : zr[2 * j + 1 - 32];
        Q[j] = cx2{v2f{u0.r, u1.r}, v2f{u0.i, u1.i}};
    }
    cx yp[32], ym[32];
    load_stage_tw(A.tw, lane, 0u, tlo, thp);
    fft4096_pk<true, false, false, true>(Q, lds_all[wave], tlo, thp, lane, yp, ym);

    // pair m = l + 64 b holds the samples 2 m, 2 m + 1: yp for b < 32, ym for b + 32
    v2f *o = reinterpret_cast<v2f *>(A.S + ((uint64_t)row * A.slots + slot) * kStftCxN);
#pragma unroll
    for (int b = 0; b < 32; ++b) {
        const uint32_t m = lane + 64u * (uint32_t)b;
        const v2f w0 = A.win2[m], w1 = A.win2[m + 2048u];
        o[m] = v2f{yp[b].r * w0.x, yp[b].i * w0.y};
        o[m + 2048u] = v2f{ym[b].r * w1.x, ym[b].i * w1.y};
    }
}

// grid (ceil((i1 - i0) / 256), rows).  Inside a chunk everything fits 32 bits:
// t = i - fa H < (slots + 1) N, and the frames count from fa (g = f - fa, the slot)
__global__ __launch_bounds__(256) void istft_ola_kernel(IstftArgs A) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x, row = blockIdx.y;
    if (r >= A.n) return;
    const uint32_t t = A.t0 + r;
    // the frames that cover the sample: g H <= t < g H + N, and g < ns (istft_chunk:
    // the last slot is the last frame of the call a sample of the chunk touches)
    const uint32_t glo = t < kStftCxN ? 0u : (t - kStftCxN) / A.H + 1u;
    uint32_t ghi = t / A.H;
    if (ghi > A.ns - 1u) ghi = A.ns - 1u;
    const float *S = A.S + (uint64_t)row * A.slots * kStftCxN;
    float num = 0.f, den = 0.f;
    for (uint32_t g = glo; g <= ghi; ++g) {
        const uint32_t j = t - g * A.H;  // < N
        num = num + S[g * kStftCxN + j];
        const float w = A.win[j];
        den = __fmaf_rn(w, w, den);
    }
    A.out.p[row][A.i0 + r] = den < A.floor ? 0.f : __fdiv_rn(num, den);
}

int launch_istft_chunk(const IstftArgs &A, hipStream_t s) {
    if (A.cn == 0 || A.cn > (uint32_t)kMaxChannels || A.ns == 0 || A.ns > A.slots || A.i1 <= A.i0 || A.H == 0)
        return DSP_ERR_INVALID;
    // every frame a sample of [i0, i1) needs lies in the slots
    const uint64_t flo = A.i0 < kStftCxN ? 0 : (A.i0 - kStftCxN) / A.H + 1;
    const uint64_t fhi = std::min<uint64_t>((A.i1 - 1) / A.H, A.F - 1);
    if (flo < A.fa || fhi >= A.fa + A.ns || A.fa + A.ns > A.F) return DSP_ERR_INVALID;
    // ... and the chunk's samples, counted from frame fa's first, fit 32 bits
    if (A.i1 - A.fa * A.H > ((uint64_t)A.slots + 1) * kStftCxN) return DSP_ERR_INVALID;
    IstftArgs G = A;
    G.t0 = (uint32_t)(A.i0 - A.fa * A.H);
    G.n = (uint32_t)(A.i1 - A.i0);
    hipLaunchKernelGGL(istft_frame_kernel, dim3((A.ns + 3) / 4, A.cn), dim3(256), 0, s, G);
    DSPB_HIP(hipGetLastError());
    hipLaunchKernelGGL(istft_ola_kernel, dim3((G.n + 255u) / 256u, A.cn), dim3(256), 0, s, G);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

}  // namespace dspb
