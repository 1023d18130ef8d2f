// iir_scan.hpp -- the lane types, the cascade and the state-transition product
// of the block-parallel biquad scan, shared by DSP_PLUGIN_BIQUAD (iir.hip) and
// the K-weighting meter (loudness.hip).  See iir.hip for the scheme.
#pragma once
#include "kernels.hpp"

namespace dspb {

constexpr int kIirT = 32;             // samples per lane
constexpr int kIirTile = 64 * kIirT;  // samples per wavefront (tile)
constexpr int kIirWaves = 4;          // wavefronts per workgroup
constexpr int kIirLdsStride = kIirT + 1;  // floats per lane chunk in LDS (conflict-free column reads)
typedef float f4 __attribute__((ext_vector_type(4)));

// a lane's values for NCH channels at once: float (one channel per wave) or
// a VGPR pair (a channel pair per wave: every section step one v_pk_fma_f32)
template <int NCH> struct Lanes;
template <> struct Lanes<1> {
    typedef float V;
    static __device__ __forceinline__ V splat(float x) { return x; }
    static __device__ __forceinline__ V fma(V a, V b, V c) { return __builtin_fmaf(a, b, c); }
    static __device__ __forceinline__ float get(V v, int) { return v; }
    static __device__ __forceinline__ void set(V &v, int, float x) { v = x; }
    static __device__ __forceinline__ V shfl_up(V v, uint32_t d) { return __shfl_up(v, d); }
    static __device__ __forceinline__ V shfl(V v, int l) { return __shfl(v, l); }
    static __device__ __forceinline__ V shfl_xor(V v, int m) { return __shfl_xor(v, m); }
};
template <> struct Lanes<2> {
    typedef v2f V;
    static __device__ __forceinline__ V splat(float x) { return V{x, x}; }
    static __device__ __forceinline__ V fma(V a, V b, V c) { return __builtin_elementwise_fma(a, b, c); }
    static __device__ __forceinline__ float get(V v, int k) { return k ? v.y : v.x; }
    static __device__ __forceinline__ void set(V &v, int k, float x) {
        if (k) v.y = x;
        else v.x = x;
    }
    static __device__ __forceinline__ V shfl_up(V v, uint32_t d) { return V{__shfl_up(v.x, d), __shfl_up(v.y, d)}; }
    static __device__ __forceinline__ V shfl(V v, int l) { return V{__shfl(v.x, l), __shfl(v.y, l)}; }
    static __device__ __forceinline__ V shfl_xor(V v, int m) { return V{__shfl_xor(v.x, m), __shfl_xor(v.y, m)}; }
};

template <int S, int NCH>
struct Cascade {
    static constexpr int D = 2 * S;
    typedef Lanes<NCH> LN;
    typedef typename LN::V V;
    V b0[S], b1[S], b2[S], na1[S], na2[S];

    __device__ explicit Cascade(const float *cf) {
#pragma unroll
        for (int k = 0; k < S; ++k) {
            b0[k] = LN::splat(cf[5 * k]);
            b1[k] = LN::splat(cf[5 * k + 1]);
            b2[k] = LN::splat(cf[5 * k + 2]);
            na1[k] = LN::splat(-cf[5 * k + 3]);
            na2[k] = LN::splat(-cf[5 * k + 4]);
        }
    }

    // runs the cascade over x[0..T) from state st (y1, y2 per section; the x
    // history of section k > 0 is section k - 1's (y1, y2)); section 1's x
    // history is (xh1, xh2).  st ends as the state after x[T-1].  kWrite:
    // x[n] becomes the last section's output.
    template <bool kWrite>
    __device__ __forceinline__ void run(V (&x)[kIirT], V xh1, V xh2, V (&st)[D]) const {
        V X1[S], X2[S], Y1[S], Y2[S];
#pragma unroll
        for (int k = 0; k < S; ++k) {
            Y1[k] = st[2 * k];
            Y2[k] = st[2 * k + 1];
            X1[k] = k ? st[2 * k - 2] : xh1;
            X2[k] = k ? st[2 * k - 1] : xh2;
        }
#pragma unroll
        for (int n = 0; n < kIirT; ++n) {
            V v = x[n];
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const V acc = LN::fma(b2[k], X2[k], LN::fma(b1[k], X1[k], b0[k] * v));
                const V y = LN::fma(na1[k], Y1[k], LN::fma(na2[k], Y2[k], acc));
                X2[k] = X1[k];
                X1[k] = v;
                Y2[k] = Y1[k];
                Y1[k] = y;
                v = y;
            }
            if (kWrite) x[n] = v;
        }
#pragma unroll
        for (int k = 0; k < S; ++k) {
            st[2 * k] = Y1[k];
            st[2 * k + 1] = Y2[k];
        }
    }
};

// r = m v for a D x D row-major matrix in memory
template <int D, int NCH>
__device__ __forceinline__ void matvec(const float *m, const typename Lanes<NCH>::V (&v)[D],
                                       typename Lanes<NCH>::V (&r)[D]) {
    typedef Lanes<NCH> LN;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        typename LN::V a = LN::splat(0.f);
#pragma unroll
        for (int j = 0; j < D; ++j) a = LN::fma(LN::splat(m[i * D + j]), v[j], a);
        r[i] = a;
    }
}

}  // namespace dspb
