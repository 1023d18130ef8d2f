// welch.hip -- dsp_welch: Welch sums over 8192-point windowed frames of hop H,
// sxx = sum_f |X_f|^2, srr = sum_f |R_f|^2, sxy = sum_f conj(R_f) X_f, as
// float64 rows in natural bin order.  conv_fdl.hip's structure with a
// frame-axis reduction where that has a multiply-accumulate and an inverse.
// The frames are walked in chunks of at most A.chunk (a multiple of kWelchRun),
// three launches per chunk on the call's stream:
//
//   forward   one wavefront per (frame, row): the window at load, the
//             8192-point real FFT of ols_frame.hpp up to the split, 2 X_f to
//             scratch in the split's register order (conv_fdl.hip's spectrum:
//             kConvSpec4 float4).  Row cn is the reference.
//   reduce    a wave owns one 64-lane float4 slice of one row for one run of
//             kWelchRun consecutive frames: |X|^2 (|R|^2 for the reference row)
//             and conj(R) X accumulated in float32 registers in frame order,
//             the run's partial sums stored in the same slice order
//   combine   one thread per (row, bin): the chunk's runs added in float64 in
//             run order onto the output row, which the first chunk starts from
//             zero -- the one place the split order becomes bin order
//
// Runs never straddle a chunk (the chunk is a multiple of the run), so the
// order of every addition is a function of F alone: no atomics, the same bits
// on every run, and a channel's bits do not depend on its neighbours.
//
// The reduce's cross terms are compiled with contraction off:
// im(conj(R) X) = R.re X.im - R.im X.re is two rounded products and
// their rounded difference, which is exactly 0 when X and R hold the same bits.
// tools/welch_model.py is the float32 model of this order.
#include "ols_frame.hpp"
#include "welch_host.hpp"

namespace dspb {

static_assert(kWelchSpec4 == kConvSpec4, "the forward launch stores conv_fdl.hip's spectrum layout");
constexpr uint32_t kWelchSlices = kWelchSpec4 / 64;  // 33

// grid (frame groups of 4, rows); LDS: four 64 x 33 transpose tiles
__global__ __launch_bounds__(256, 2) void welch_forward_kernel(WelchArgs A) {
    __shared__ __attribute__((aligned(16))) float lds_all[4][64 * 33];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t row = blockIdx.y;
    const uint32_t f = xcd_remap(blockIdx.x, gridDim.x) * 4u + wave;  // of the chunk
    if (f >= A.nf) return;
    const float *x = (row < A.cn ? A.in.p[row] : A.ref) + (A.f0 + f) * (uint64_t)A.H;

    cx tlo[8];
    cx2 thp[4];
    load_stage_tw(A.tw, lane, 0u, tlo, thp);
    cx2 P[32];
    welch_load_frame(x, A.win2, lane, P);
    cx zp[32], zm[32];
    fft4096_pk<false, false, false, true>(P, lds_all[wave], tlo, thp, lane, zp, zm);

    const OlsLane ln = ols_lane(A.tw, lane);
    float4 *o = A.S + ((uint64_t)row * A.chunk + f) * kWelchSpec4;
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

// a += |x|^2 of the float4's two bins (re, re, im, im)
__device__ __forceinline__ void welch_power(v2f &a, float4 x) {
    a.x = __fmaf_rn(x.x, x.x, a.x);
    a.x = __fmaf_rn(x.z, x.z, a.x);
    a.y = __fmaf_rn(x.y, x.y, a.y);
    a.y = __fmaf_rn(x.w, x.w, a.y);
}
// one bin of a += conj(r) x: every product and sum rounded on its own (the
// pragma: HIP's __fmul_rn is a plain product, which the compiler may contract)
__device__ __forceinline__ void welch_cross(float &are, float &aim, float rr, float ri, float xr, float xi) {
#pragma clang fp contract(off)
    const float p0 = rr * xr, p1 = ri * xi, q0 = rr * xi, q1 = ri * xr;
    const float re = p0 + p1, im = q0 - q1;
    are = are + re;
    aim = aim + im;
}

// grid (runs of the chunk, 11 x 3 slices, rows); a block's three waves take
// neighbouring slices of one run
__global__ __launch_bounds__(192) void welch_reduce_kernel(WelchArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t sl = blockIdx.y * 3u + wave;  // < kWelchSlices = 3 gridDim.y
    const uint32_t row = blockIdx.z;
    const uint32_t run = xcd_remap(blockIdx.x, gridDim.x);
    const uint32_t fb = run * kWelchRun;
    const uint32_t n = A.nf - fb < kWelchRun ? A.nf - fb : kWelchRun;  // >= 1
    const uint32_t off = 64u * sl + lane;
    const float4 *X = A.S + ((uint64_t)row * A.chunk + fb) * kWelchSpec4 + off;
    const uint64_t po = ((uint64_t)row * A.runs_cap + run) * kWelchSpec4 + off;
    v2f pw = v2f{0.f, 0.f};
    if (row == A.cn || !A.has_ref) {  // the reference's |R|^2, or a channel without one
#pragma unroll 4
        for (uint32_t j = 0; j < n; ++j) welch_power(pw, X[(uint64_t)j * kWelchSpec4]);
        if (row == A.cn) A.prr[(uint64_t)run * kWelchSpec4 + off] = pw;
        else A.pxx[po] = pw;
        return;
    }
    const float4 *R = A.S + ((uint64_t)A.cn * A.chunk + fb) * kWelchSpec4 + off;
    float4 cr = float4{0.f, 0.f, 0.f, 0.f};  // (re, re, im, im)
#pragma unroll 4
    for (uint32_t j = 0; j < n; ++j) {
        const float4 x = X[(uint64_t)j * kWelchSpec4], r = R[(uint64_t)j * kWelchSpec4];
        welch_power(pw, x);
        welch_cross(cr.x, cr.z, r.x, r.z, x.x, x.z);
        welch_cross(cr.y, cr.w, r.y, r.w, x.y, x.w);
    }
    A.pxx[po] = pw;
    A.pxy[po] = cr;
}

// where bin k <= 4096 sits in a spectrum: the float index of its real part
// (the imaginary part is two floats on).  k and 4096 - k share a lane pair.
__device__ __forceinline__ uint32_t welch_bin_float(uint32_t k) {
    if (k == 2048u) return 4u * 2048u;
    const uint32_t h = k > 2048u ? 1u : 0u, kk = h ? 4096u - k : k;  // kk < 2048
    const uint32_t l = kk & 63u, q = kk >> 6, ka = q & 15u, c = q >> 4;
    return 4u * (2u * (64u * ka + l) + h) + c;
}

// grid (ceil(4097 / 256), rows)
__global__ __launch_bounds__(256) void welch_combine_kernel(WelchArgs A) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, row = blockIdx.y;
    if (k >= kWelchBins) return;
    const uint32_t runs = (A.nf + kWelchRun - 1) / kWelchRun;
    const uint32_t i = welch_bin_float(k);  // of a float4 spectrum; i / 2 + (i & 1) of a v2f one
    const uint32_t i2 = (i >> 2) * 2u + (i & 1u);
    // the spectra hold 2 X: a quarter of every sum (exact)
    if (row == A.cn) {
        if (!A.srr) return;
        const float *p = reinterpret_cast<const float *>(A.prr) + i2;
        double s = A.first ? 0.0 : A.srr[k];
        for (uint32_t r = 0; r < runs; ++r) s += 0.25 * (double)p[(uint64_t)r * (2u * kWelchSpec4)];
        A.srr[k] = s;
        return;
    }
    const uint64_t pr = (uint64_t)row * A.runs_cap;
    {
        const float *p = reinterpret_cast<const float *>(A.pxx + pr * kWelchSpec4) + i2;
        double s = A.first ? 0.0 : A.sxx[row][k];
        for (uint32_t r = 0; r < runs; ++r) s += 0.25 * (double)p[(uint64_t)r * (2u * kWelchSpec4)];
        A.sxx[row][k] = s;
    }
    if (A.has_ref) {
        const float *p = reinterpret_cast<const float *>(A.pxy + pr * kWelchSpec4) + i;
        double re = A.first ? 0.0 : A.sxy[row][2u * k], im = A.first ? 0.0 : A.sxy[row][2u * k + 1u];
        for (uint32_t r = 0; r < runs; ++r) {
            re += 0.25 * (double)p[(uint64_t)r * (4u * kWelchSpec4)];
            im += 0.25 * (double)p[(uint64_t)r * (4u * kWelchSpec4) + 2u];
        }
        A.sxy[row][2u * k] = re;
        A.sxy[row][2u * k + 1u] = im;
    }
}

// one chunk (A.nf <= A.chunk frames from A.f0) of one channel group
int launch_welch_chunk(const WelchArgs &A, hipStream_t s) {
    if (A.nf == 0 || A.cn == 0 || A.nf > A.chunk) return DSP_ERR_INVALID;
    const uint32_t rows = A.cn + (A.has_ref ? 1u : 0u);
    const uint32_t runs = (A.nf + kWelchRun - 1) / kWelchRun;
    if (runs > A.runs_cap) return DSP_ERR_INVALID;
    hipLaunchKernelGGL(welch_forward_kernel, dim3((A.nf + 3) / 4, rows), dim3(256), 0, s, A);
    DSPB_HIP(hipGetLastError());
    hipLaunchKernelGGL(welch_reduce_kernel, dim3(runs, kWelchSlices / 3, rows), dim3(192), 0, s, A);
    DSPB_HIP(hipGetLastError());
    hipLaunchKernelGGL(welch_combine_kernel, dim3((kWelchBins + 255) / 256, rows), dim3(256), 0, s, A);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

}  // namespace dspb
