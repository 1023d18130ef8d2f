// fft_big.hip -- the large real FFT of dsp_rfft / dsp_irfft and the pointwise
// kernels of dsp_deconvolve (dspbench.h), n = 2^10 .. 2^24.
//
// The real row is packed as z[j] = x[2j] + i x[2j+1]; the M = n / 2 point
// complex transform runs as 2..4 Stockham passes (host_tables.hpp rfft_plan),
// ping-pong between two work buffers.  A pass of radix R with Ns = the product
// of the radices before it: thread j < M / R
//   loads   v[t] = src[j + t M / R], t < R          (lanes: consecutive j)
//   twiddle v[t] *= W_{Ns R}^{(j mod Ns) t}         (two-level table of W_n)
//   transforms v by the register block of R (sdft8 / sdft32 / sdft64)
//   stores  dst[(j / Ns) Ns R + (j mod Ns) + k Ns] = V[k]
// so every load of a wave is 512 contiguous bytes and every store of a later
// pass a run of min(Ns, 64) complex (Ns >= 32: 256 bytes).  The first pass
// (Ns = 1) has no twiddles and its V[k] of thread j belong at j R + k: the
// workgroup's 64 R outputs are one contiguous run, transposed through a padded
// LDS tile (rows of R + 1 floats, re and im planes apart: bank (j (R + 1) + k)
// mod 32 is distinct for the 32 lanes of a half on the write, consecutive on
// the read).  The first pass also packs the real row (zero past L, never read)
// and the last pass of the inverse unpacks, scales by 1 / n and rotates.
// One workgroup is one wave: no kernel waits on another workgroup, nothing is
// accumulated across threads, so the bits are the same on every run and do not
// depend on the number of channels.
#include <hip/hip_runtime.h>

#include "fft_soa.hpp"

namespace dspb {
namespace {

template <int R> __device__ __forceinline__ constexpr int perm_of(int k) {
    return R == 64 ? perm64(k) : R == 32 ? perm32(k) : k;
}
template <int R> __device__ __forceinline__ void dft_block(cx (&v)[R]);
template <> __device__ __forceinline__ void dft_block<64>(cx (&v)[64]) { sdft64<true>(v); }
template <> __device__ __forceinline__ void dft_block<32>(cx (&v)[32]) { sdft32(v); }
template <> __device__ __forceinline__ void dft_block<8>(cx (&v)[8]) {
    sdft8(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
}

// W_n^K, K < n
__device__ __forceinline__ cx big_tw(const v2f *tw, uint32_t lo_n, uint32_t K) {
    const v2f lo = tw[K & ((1u << kBigTwShift) - 1u)], hi = tw[lo_n + (K >> kBigTwShift)];
    return mulc(cx{hi.x, hi.y}, lo.x, lo.y);
}

struct PassArgs {
    const v2f *src;   // [nch][M]
    v2f *dst;         // [nch][M]
    const v2f *tw;
    ChanIn rin;       // kLoadReal
    ChanOut rout;     // kStoreReal
    uint64_t L, Lout;
    uint32_t n, M, Mr;          // Mr = M / R
    uint32_t Ns, logNs, tmul;   // tmul = 2 M / (Ns R): K = (j mod Ns) t tmul
    uint32_t lo_n;
    uint32_t rot;
    float scale;
    uint32_t in_aligned8, out_aligned8;
};

enum { kFirstComplex = 0, kFirstReal = 1, kLaterComplex = 2, kLaterReal = 3 };

template <int R, int MODE>
__global__ __launch_bounds__(64) void big_pass_kernel(const PassArgs A) {
    const uint32_t lane = threadIdx.x, c = blockIdx.y;
    const uint32_t j = blockIdx.x * 64u + lane;
    const bool active = j < A.Mr;
    const uint64_t row = (uint64_t)c * A.M;
    cx v[R];
    if (active) {
        if (MODE == kFirstReal) {
            const float *x = A.rin.p[c];
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const uint64_t s0 = 2ull * (j + (uint32_t)t * A.Mr);
                if (A.in_aligned8 && s0 + 1 < A.L) {
                    const v2f p = *reinterpret_cast<const v2f *>(x + s0);
                    v[t] = cx{p.x, p.y};
                } else {
                    v[t].r = s0 < A.L ? x[s0] : 0.f;
                    v[t].i = s0 + 1 < A.L ? x[s0 + 1] : 0.f;
                }
            }
        } else {
            const v2f *z = A.src + row;
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const v2f p = z[j + (uint32_t)t * A.Mr];
                v[t] = cx{p.x, p.y};
            }
            if (MODE >= kLaterComplex) {
                const uint32_t k1 = (j & (A.Ns - 1u)) * A.tmul;
#pragma unroll
                for (int t = 1; t < R; ++t) v[t] = mulc(v[t], big_tw(A.tw, A.lo_n, k1 * (uint32_t)t));
            }
        }
        dft_block<R>(v);
    }
    if (MODE <= kFirstReal) {
        // the workgroup's outputs [blockIdx.x 64 R, + rows R) through the padded tile
        __shared__ float tre[64 * (R + 1)], tim[64 * (R + 1)];
        if (active) {
#pragma unroll
            for (int k = 0; k < R; ++k) {
                tre[lane * (R + 1) + k] = v[perm_of<R>(k)].r;
                tim[lane * (R + 1) + k] = v[perm_of<R>(k)].i;
            }
        }
        __syncthreads();
        const uint32_t rows = min(64u, A.Mr - blockIdx.x * 64u);  // (Mr is a power of two: below 64, or a multiple)
        v2f *z = A.dst + row + (uint64_t)blockIdx.x * 64u * R;
        for (uint32_t o = lane; o < rows * R; o += 64u) {
            const uint32_t a = o + o / R;
            z[o] = v2f{tre[a], tim[a]};
        }
    } else if (active) {
        const uint32_t base = ((j >> A.logNs) << A.logNs) * R + (j & (A.Ns - 1u));
        if (MODE == kLaterComplex) {
            v2f *z = A.dst + row;
#pragma unroll
            for (int k = 0; k < R; ++k) z[base + (uint32_t)k * A.Ns] = v2f{v[perm_of<R>(k)].r, v[perm_of<R>(k)].i};
        } else {
            // w = conj(FFT(conj Z)): x[2i] = Re w[i] / n, x[2i + 1] = -Im w[i] / n, at (2i + rot) mod n
            float *y = A.rout.p[c];
            const bool pairs = A.out_aligned8 && !(A.rot & 1u);
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const uint32_t i0 = (2u * (base + (uint32_t)k * A.Ns) + A.rot) & (A.n - 1u);
                const uint32_t i1 = (i0 + 1u) & (A.n - 1u);
                const float a = v[perm_of<R>(k)].r * A.scale, b = -v[perm_of<R>(k)].i * A.scale;
                if (pairs && (uint64_t)i0 + 1 < A.Lout) {  // (rot even: i1 = i0 + 1)
                    *reinterpret_cast<v2f *>(y + i0) = v2f{a, b};
                } else {
                    if (i0 < A.Lout) y[i0] = a;
                    if (i1 < A.Lout) y[i1] = b;
                }
            }
        }
    }
}

struct SplitArgs {
    const v2f *z;   // forward: [nch][M] the packed transform
    v2f *zout;      // inverse: [nch][M] conj of the packed spectrum
    const v2f *tw;
    ChanIn sin;     // inverse: spectra
    ChanOut sout;   // forward: spectra
    uint32_t n, M, lo_n;
    uint32_t aligned8;
};

// X[k] = E[k] + W_n^k O[k], E = (Z[k] + conj Z[M - k]) / 2, O = (Z[k] - conj Z[M - k]) / 2i, k <= M
__global__ __launch_bounds__(256) void big_split_kernel(const SplitArgs A) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, c = blockIdx.y;
    if (k > A.M) return;
    const v2f *z = A.z + (uint64_t)c * A.M;
    const v2f a = z[k & (A.M - 1u)], b = z[(A.M - k) & (A.M - 1u)];
    v2f X;
    if (k == 0) X = v2f{a.x + a.y, 0.f};
    else if (k == A.M) X = v2f{a.x - a.y, 0.f};
    else {
        const cx e = cx{0.5f * (a.x + b.x), 0.5f * (a.y - b.y)};
        const cx d = cx{a.x - b.x, a.y + b.y};         // Z[k] - conj Z[M - k]
        const cx o = cx{0.5f * d.i, -0.5f * d.r};       // d / 2i
        const cx t = mulc(o, big_tw(A.tw, A.lo_n, k));
        X = v2f{e.r + t.r, e.i + t.i};
    }
    float *out = A.sout.p[c] + 2ull * k;
    if (A.aligned8) *reinterpret_cast<v2f *>(out) = X;
    else out[0] = X.x, out[1] = X.y;
}

// conj Z[k], Z[k] = (X[k] + conj X[M - k]) + i conj(W_n^k) (X[k] - conj X[M - k]), k < M
// (twice E + i O: the 1 / 2 is in the last pass's 1 / n)
__global__ __launch_bounds__(256) void big_unsplit_kernel(const SplitArgs A) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, c = blockIdx.y;
    if (k >= A.M) return;
    const float *X = A.sin.p[c];
    v2f a, b;
    if (A.aligned8) {
        a = *reinterpret_cast<const v2f *>(X + 2ull * k);
        b = *reinterpret_cast<const v2f *>(X + 2ull * (A.M - k));
    } else {
        a = v2f{X[2ull * k], X[2ull * k + 1]};
        b = v2f{X[2ull * (A.M - k)], X[2ull * (A.M - k) + 1]};
    }
    if (k == 0) a.y = 0.f, b.y = 0.f;  // bins 0 and n / 2: the real part only
    const cx s = cx{a.x + b.x, a.y - b.y};
    const cx d = cx{a.x - b.x, a.y + b.y};
    const cx w = big_tw(A.tw, A.lo_n, k);
    const cx t = mulc(d, w.r, -w.i);             // conj(W) d
    const cx Z = cx{s.r - t.i, s.i + t.r};       // s + i t
    A.zout[(uint64_t)c * A.M + k] = v2f{Z.r, -Z.i};
}

__device__ __forceinline__ float power_of(v2f s) { return __builtin_fmaf(s.x, s.x, s.y * s.y); }

__global__ __launch_bounds__(256) void deconv_max_kernel(const v2f *S, uint32_t bins, uint32_t *word) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    // |S|^2 >= 0 (a NaN's bits would win: the caller's rows are finite by contract)
    uint32_t b = k < bins ? __float_as_uint(power_of(S[k])) : 0u;
#pragma unroll
    for (int off = 32; off; off >>= 1) b = max(b, (uint32_t)__shfl_xor((int)b, off));
    if ((threadIdx.x & 63u) == 0 && b) atomicMax(word, b);
}

__global__ __launch_bounds__(256) void deconv_divide_kernel(v2f *Y, const v2f *S, uint32_t bins, float eps,
                                                            const uint32_t *word) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= bins) return;
    const float lambda = eps * __uint_as_float(*word);
    const v2f s = S[k];
    v2f *row = Y + (uint64_t)blockIdx.y * bins;
    const v2f y = row[k];
    const float den = power_of(s) + lambda;
    const float re = __builtin_fmaf(y.x, s.x, y.y * s.y), im = __builtin_fmaf(y.y, s.x, -(y.x * s.y));
    row[k] = den > 0.f ? v2f{re / den, im / den} : v2f{0.f, 0.f};
}

int args_ok(const BigFftArgs &A) {
    uint32_t passes = 0, radix[4];
    if (!rfft_plan(A.n, &passes, radix)) return DSP_ERR_INVALID;
    if (A.passes != passes || A.nch == 0 || A.nch > (uint32_t)kMaxChannels) return DSP_ERR_INVALID;
    for (uint32_t i = 0; i < 4; ++i)
        if (A.radix[i] != radix[i]) return DSP_ERR_INVALID;
    if (!A.tw || !A.buf0 || !A.buf1 || A.L > A.n || A.Lout > A.n || A.rot >= A.n) return DSP_ERR_INVALID;
    for (uint32_t j = 0; j < A.nch; ++j)
        if (!A.in.p[j] || !A.out.p[j]) return DSP_ERR_INVALID;
    return DSP_OK;
}

template <int MODE>
int launch_pass(const PassArgs &P, uint32_t R, uint32_t nch, hipStream_t s) {
    const dim3 grid((P.Mr + 63u) / 64u, nch);
    if (R == 64) hipLaunchKernelGGL((big_pass_kernel<64, MODE>), grid, dim3(64), 0, s, P);
    else if (R == 32) hipLaunchKernelGGL((big_pass_kernel<32, MODE>), grid, dim3(64), 0, s, P);
    else if (R == 8) hipLaunchKernelGGL((big_pass_kernel<8, MODE>), grid, dim3(64), 0, s, P);
    else return DSP_ERR_INVALID;
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

// the passes of the plan: the first from `first_src` (or the real rows), the
// last into `*result` (or the real rows)
int run_passes(const BigFftArgs &A, bool load_real, bool store_real, const v2f *first_src, const v2f **result,
               hipStream_t s) {
    const uint32_t M = A.n / 2;
    PassArgs P{};
    P.tw = A.tw;
    P.rin = A.in;
    P.rout = A.out;
    P.L = A.L;
    P.Lout = A.Lout;
    P.n = A.n;
    P.M = M;
    P.lo_n = rfft_twiddle_lo(A.n);
    P.rot = A.rot;
    P.scale = 1.f / (float)A.n;
    P.in_aligned8 = A.in_aligned8;
    P.out_aligned8 = A.out_aligned8;
    const v2f *src = first_src;
    // (the inverse's split wrote buf0: its first pass goes to buf1)
    v2f *dst = first_src == A.buf0 ? A.buf1 : A.buf0;
    uint32_t Ns = 1, logNs = 0;
    for (uint32_t i = 0; i < A.passes; ++i) {
        const uint32_t R = A.radix[i];
        P.src = src;
        P.dst = dst;
        P.Mr = M / R;
        P.Ns = Ns;
        P.logNs = logNs;
        P.tmul = 2u * (M / (Ns * R));
        int st;
        if (i == 0) st = load_real ? launch_pass<kFirstReal>(P, R, A.nch, s) : launch_pass<kFirstComplex>(P, R, A.nch, s);
        else if (i + 1 == A.passes && store_real) st = launch_pass<kLaterReal>(P, R, A.nch, s);
        else st = launch_pass<kLaterComplex>(P, R, A.nch, s);
        if (st) return st;
        src = dst;
        dst = dst == A.buf0 ? A.buf1 : A.buf0;
        Ns *= R;
        while ((1u << logNs) < Ns) ++logNs;
    }
    if (result) *result = src;
    return DSP_OK;
}

}  // namespace

int launch_big_rfft(const BigFftArgs &A, hipStream_t s) {
    if (int st = args_ok(A)) return st;
    const v2f *Z = nullptr;
    if (int st = run_passes(A, true, false, nullptr, &Z, s)) return st;
    SplitArgs S{};
    S.z = Z;
    S.tw = A.tw;
    S.sout = A.out;
    S.n = A.n;
    S.M = A.n / 2;
    S.lo_n = rfft_twiddle_lo(A.n);
    S.aligned8 = A.out_aligned8;
    hipLaunchKernelGGL(big_split_kernel, dim3(S.M / 256u + 1u, A.nch), dim3(256), 0, s, S);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

int launch_big_irfft(const BigFftArgs &A, hipStream_t s) {
    if (int st = args_ok(A)) return st;
    SplitArgs S{};
    S.zout = A.buf0;
    S.tw = A.tw;
    S.sin = A.in;
    S.n = A.n;
    S.M = A.n / 2;
    S.lo_n = rfft_twiddle_lo(A.n);
    S.aligned8 = A.in_aligned8;
    hipLaunchKernelGGL(big_unsplit_kernel, dim3(S.M / 256u, A.nch), dim3(256), 0, s, S);
    DSPB_HIP(hipGetLastError());
    return run_passes(A, false, true, A.buf0, nullptr, s);
}

int launch_deconv_max(const v2f *S, uint32_t bins, uint32_t *word, hipStream_t s) {
    if (!S || !word || bins == 0) return DSP_ERR_INVALID;
    hipLaunchKernelGGL(deconv_max_kernel, dim3((bins + 255u) / 256u), dim3(256), 0, s, S, bins, word);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

int launch_deconv_divide(v2f *Y, const v2f *S, uint32_t bins, uint32_t nch, float eps, const uint32_t *word,
                         hipStream_t s) {
    if (!Y || !S || !word || bins == 0 || nch == 0 || nch > (uint32_t)kMaxChannels) return DSP_ERR_INVALID;
    hipLaunchKernelGGL(deconv_divide_kernel, dim3((bins + 255u) / 256u, nch), dim3(256), 0, s, Y, S, bins, eps, word);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

}  // namespace dspb
