// decay.hip -- dsp_decay's own launches (dspbench.h): peak and onset of the
// unfiltered rows, the band masks on a channel's spectrum, and the hop sums of
// the band-filtered rows.  The transforms between them are fft_big.hip's.
//
//   peak     integer atomic max over the bit patterns of |x| (non-negative
//            floats order as their bits), straight onto the caller's float
//   onset    thr = peak * 0.1f; integer atomic min over the indices with
//            |x[i]| >= thr, straight onto the caller's uint64 (set to ~0 first)
//   mask     one thread per (row, bin): Y_row[k] = g(k) X_ch(row)[k], g in
//            float32 with correctly rounded division and square root
//   hops     sixteen lanes per unit of at most hop samples: a hop after the
//            onset (to its entry of the energy row) or a piece before it (to
//            the scratch); lane q adds samples q, q + 16, ... in float64, the
//            sixteen are added as a xor tree (8, 4, 2, 1).  The launch reads
//            the onset on the device and zeroes the entries past the last hop
//   entry0   one wave per row: lane l adds pieces l, l + 64, ... in piece
//            order, the 64 as a xor tree (32 .. 1), into entry 0
//
// Every sum has one order, a function of hop, onset and L: no float atomics,
// the same bits on every run, and a row's bits do not depend on its neighbours.
// tools/decay_model.py is the model of this arithmetic.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace dspb {
namespace {

__device__ __forceinline__ uint64_t least(uint64_t a, uint64_t b) { return a < b ? a : b; }

// grid (blocks, channels of the group)
__global__ __launch_bounds__(256) void decay_peak_kernel(DecayArgs A) {
    const float *x = A.in.p[blockIdx.y];
    uint32_t b = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < A.L; i += (uint64_t)gridDim.x * 256u)
        b = max(b, __float_as_uint(fabsf(x[i])));
#pragma unroll
    for (int off = 32; off; off >>= 1) b = max(b, (uint32_t)__shfl_xor((int)b, off));
    if ((threadIdx.x & 63u) == 0 && b) atomicMax(reinterpret_cast<uint32_t *>(A.peak) + blockIdx.y, b);
}

__global__ __launch_bounds__(256) void decay_onset_kernel(DecayArgs A) {
    const float *x = A.in.p[blockIdx.y];
    const float thr = __fmul_rn(A.peak[blockIdx.y], 0.1f);
    unsigned long long m = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < A.L; i += (uint64_t)gridDim.x * 256u)
        if (fabsf(x[i]) >= thr) {
            m = i;
            break;
        }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long o = __shfl_xor(m, off);
        m = o < m ? o : m;
    }
    if ((threadIdx.x & 63u) == 0 && m != ~0ull) atomicMin(A.onset + blockIdx.y, m);
}

// g of bin k: u = f / fm = k fscale, v = u - 1 / u as (u - 1)(u + 1) / u (the
// difference exact near the mid frequency), g = 1 / sqrt(1 + (Qd v)^6)
__device__ __forceinline__ float decay_gain(uint32_t k, float fscale, float Qd) {
    if (k == 0) return 0.f;
    const float u = (float)k * fscale;
    const float v = __fdiv_rn((u - 1.f) * (u + 1.f), u);
    const float t = Qd * v, t2 = t * t, t6 = t2 * t2 * t2;
    return __fdiv_rn(1.f, __fsqrt_rn(1.f + t6));
}

// grid (ceil(bins / 256), rows)
__global__ __launch_bounds__(256) void decay_mask_kernel(DecayArgs A) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, r = blockIdx.y;
    if (k >= A.bins) return;
    const v2f x = A.X[(uint64_t)A.xrow[r] * A.bins + k];
    const float g = decay_gain(k, A.fscale[r], A.Qd);
    A.Y[(uint64_t)r * A.bins + k] = v2f{g * x.x, g * x.y};
}

// grid (ceil((hops + 1) / 16), rows); unit u = sixteen lanes
__global__ __launch_bounds__(256) void decay_hops_kernel(DecayArgs A) {
    const uint32_t r = blockIdx.y, q = threadIdx.x & 15u;
    const uint64_t u = (uint64_t)blockIdx.x * 16u + (threadIdx.x >> 4);
    // (a row with a NaN has no onset: its word is still ~0, and everything counts as before it)
    const uint64_t o = least(A.onset[A.chan[r]], A.L), hop = A.hop;
    const uint64_t npre = (o + hop - 1) / hop, npost = (A.L - o + hop - 1) / hop;
    const float *y = A.ir + (uint64_t)r * A.Lp;
    uint64_t i0 = 0, i1 = 0;
    double *de = nullptr, *dm = nullptr;
    if (u < npre) {
        i0 = u * hop, i1 = least(o, i0 + hop);
        de = A.pre + (uint64_t)r * 2u * A.hops + u, dm = de + A.hops;
    } else if (u - npre < npost) {
        i0 = o + (u - npre) * hop, i1 = least(A.L, i0 + hop);
        de = A.energy[r] + 1 + (u - npre), dm = A.moment[r] ? A.moment[r] + 1 + (u - npre) : nullptr;
    }
    double e = 0.0, m = 0.0;
    for (uint64_t i = i0 + q; i < i1; i += 16u) {
        const float v = y[i];
        const double sq = (double)__fmul_rn(v, v);
        e += sq;
        m += (double)((long long)i - (long long)o) * sq;
    }
#pragma unroll
    for (int off = 8; off; off >>= 1) {
        e += __shfl_xor(e, off, 16);
        m += __shfl_xor(m, off, 16);
    }
    if (q) return;
    if (de) {
        *de = e;
        if (dm) *dm = m;
    }
    if (u > npost && u < A.hops) {  // the entries past the last hop
        A.energy[r][u] = 0.0;
        if (A.moment[r]) A.moment[r][u] = 0.0;
    }
}

// grid (rows), one wave
__global__ __launch_bounds__(64) void decay_entry0_kernel(DecayArgs A) {
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const uint64_t o = least(A.onset[A.chan[r]], A.L), hop = A.hop, npre = (o + hop - 1) / hop;
    const double *pe = A.pre + (uint64_t)r * 2u * A.hops, *pm = pe + A.hops;
    double e = 0.0, m = 0.0;
    for (uint64_t p = lane; p < npre; p += 64u) e += pe[p], m += pm[p];
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        e += __shfl_xor(e, off);
        m += __shfl_xor(m, off);
    }
    if (lane) return;
    A.energy[r][0] = e;
    if (A.moment[r]) A.moment[r][0] = m;
}

}  // namespace

int launch_decay_onset(const DecayArgs &A, hipStream_t s) {
    if (A.cn == 0 || A.cn > (uint32_t)kMaxChannels || A.L == 0 || !A.peak || !A.onset) return DSP_ERR_INVALID;
    DSPB_HIP(hipMemsetAsync(A.peak, 0, sizeof(float) * A.cn, s));
    DSPB_HIP(hipMemsetAsync(A.onset, 0xFF, sizeof(unsigned long long) * A.cn, s));
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((A.L + 255) / 256, 1024);
    hipLaunchKernelGGL(decay_peak_kernel, dim3(blocks, A.cn), dim3(256), 0, s, A);
    DSPB_HIP(hipGetLastError());
    hipLaunchKernelGGL(decay_onset_kernel, dim3(blocks, A.cn), dim3(256), 0, s, A);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

int launch_decay_mask(const DecayArgs &A, hipStream_t s) {
    if (A.nrows == 0 || A.nrows > (uint32_t)kMaxChannels || A.bins == 0 || !A.X || !A.Y) return DSP_ERR_INVALID;
    hipLaunchKernelGGL(decay_mask_kernel, dim3((A.bins + 255u) / 256u, A.nrows), dim3(256), 0, s, A);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

int launch_decay_hops(const DecayArgs &A, hipStream_t s) {
    if (A.nrows == 0 || A.nrows > (uint32_t)kMaxChannels || A.hop == 0 || A.L == 0 || !A.ir || !A.pre || !A.onset ||
        A.hops != (A.L + A.hop - 1) / A.hop + 1 || A.Lp < A.L)
        return DSP_ERR_INVALID;
    for (uint32_t r = 0; r < A.nrows; ++r)
        if (!A.energy[r]) return DSP_ERR_INVALID;
    hipLaunchKernelGGL(decay_hops_kernel, dim3((uint32_t)((A.hops + 1 + 15) / 16), A.nrows), dim3(256), 0, s, A);
    DSPB_HIP(hipGetLastError());
    hipLaunchKernelGGL(decay_entry0_kernel, dim3(A.nrows), dim3(64), 0, s, A);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

}  // namespace dspb
