// loudness.hip -- dsp_loudness (dspbench.h): the K-weighted hop energies and the
// sample peak in one read of the input, and the true peak, with no signal
// written back to HBM.
//
// loudness_kweight_kernel<NCH>: the two-section tile scan of iir.hip (one wave
// per 2048-sample tile, lane l the 32 samples [32 l, 32 l + 32), channel pairs
// on packed FMAs), with the store of pass 2 replaced by a reduction.  The
// K-weighting cascade decays: the state a tile is entered with depends, above
// 2^-48, only on the `window` tiles before it (dsp_biquad_plan; 1 at 8 kHz,
// 5 at 48 kHz, 18 at 192 kHz).  So no tile waits for another: a wave owns a
// run of `run` consecutive tiles of a channel unit, enters `window` tiles
// before its run with a zero state (pass 1 and the lane scan only: the
// warm-up), and carries the state from tile to tile in registers,
// S' = agg + M^(2048) S.  The scan and the carry run in the coordinates
// (y1, y1 - y2) for stage 2 (loudness_host.hpp loudness_tables): the slope of
// a state, which the near-double pole at z = 1 amplifies, keeps its own
// rounding.  Inside its run it adds pass 2 and the epilogue:
//   each lane squares its 32 outputs and splits the sum at the hop boundary
//   where one falls inside its run (at most one: hop >= 800);
//   the wave reduces each hop the tile touches (at most 4) by a butterfly;
//   lane 0 writes the tile's partials part[row][tile][0..4), first hop first.
// Every partial is a fixed function of (input, rate): the same bits every run,
// and no floating-point atomics.  The sample peak is max |x| over the staged
// tiles (integer atomicMax on the bits: |x| >= 0).
//
// loudness_finish_kernel: z[row][j] = the partials of hop j, added in tile
// order in double.
//
// loudness_truepeak_kernel<OVS>: dsp_resample's y for sr -> OVS sr, phase by
// phase over 1024 inputs staged once in LDS with their halo; every output's
// products run in the definition's order i = 0 .. Tp - 1 (zero products
// after), so an impulse gives table entries exactly; only max |y| is kept.
#include "iir_scan.hpp"
#include "loudness_host.hpp"

namespace dspb {

static_assert(kIirTile == (int)kLoudTile, "the meter's tiles are the scan's");

__device__ __forceinline__ float lanes_absmax(float m, float v) { return __builtin_fmaxf(m, __builtin_fabsf(v)); }
__device__ __forceinline__ v2f lanes_absmax(v2f m, v2f v) {
    return __builtin_elementwise_max(m, __builtin_elementwise_abs(v));
}
__device__ __forceinline__ float lanes_sel(bool c, float a, float b) { return c ? a : b; }
__device__ __forceinline__ v2f lanes_sel(bool c, v2f a, v2f b) { return c ? a : b; }

__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int NCH>
__global__ __launch_bounds__(256) void loudness_kweight_kernel(LoudnessArgs A) {
    constexpr int S = 2, D = 2 * S;
    typedef Lanes<NCH> LN;
    typedef typename LN::V V;
    __shared__ float lds[kIirWaves][64 * kIirLdsStride];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    float *buf = lds[wave];

    const uint32_t U = A.count / NCH;  // channel units (pairs) of the launch
    const uint64_t runs = (A.tiles + A.run - 1) / A.run;
    const uint64_t g = (uint64_t)blockIdx.x * kIirWaves + wave;
    if (g >= (uint64_t)U * runs) return;
    const uint32_t u = (uint32_t)(g % U);
    const uint64_t t_first = (g / U) * A.run;
    const uint64_t t_end = t_first + A.run < A.tiles ? t_first + A.run : A.tiles;
    const uint64_t t_warm = t_first > A.window ? t_first - A.window : 0;
    const uint32_t row0 = A.first + u * NCH;

    const Cascade<S, NCH> cs(A.coef);
    const uint32_t hop = A.hop;
    uint32_t rem = (uint32_t)((t_warm * (uint64_t)kIirTile) % hop);  // the tile's first sample inside its hop
    V Sin[D], pk = LN::splat(0.f);
#pragma unroll
    for (int q = 0; q < D; ++q) Sin[q] = LN::splat(0.f);

    for (uint64_t ti = t_warm; ti < t_end; ++ti) {
        const uint64_t base = ti * kIirTile;
        // stage each channel of the unit through LDS (iir.hip, step 1)
        V xr[kIirT], h1 = LN::splat(0.f), h2 = LN::splat(0.f);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const float *x = A.in.p[row0 + (uint32_t)ch];
            const uint64_t lim = A.L - base;  // > 0: ti < tiles
            if (lim >= (uint64_t)kIirTile && A.in_aligned16) {
                const f4 *x4 = reinterpret_cast<const f4 *>(x + base);
                f4 v[kIirTile / 256];
#pragma unroll
                for (int k = 0; k < kIirTile / 256; ++k) v[k] = __builtin_nontemporal_load(x4 + k * 64 + lane);
#pragma unroll
                for (int k = 0; k < kIirTile / 256; ++k) {
                    const uint32_t e = k * 256 + lane * 4;
                    float *d = buf + (e / kIirT) * kIirLdsStride + e % kIirT;
                    d[0] = v[k].x, d[1] = v[k].y, d[2] = v[k].z, d[3] = v[k].w;
                }
            } else {
                for (uint32_t e = lane; e < (uint32_t)kIirTile; e += 64)
                    buf[(e / kIirT) * kIirLdsStride + e % kIirT] = e < lim ? x[base + e] : 0.f;
            }
            float a1 = 0.f, a2 = 0.f;  // section 1's x history at the tile start
            if (lane == 0) {
                if (base >= 1) a1 = x[base - 1];
                if (base >= 2) a2 = x[base - 2];
            }
            wave_sync_lds();
#pragma unroll
            for (int n = 0; n < kIirT; ++n) LN::set(xr[n], ch, buf[lane * kIirLdsStride + n]);
            if (lane > 0) {
                a1 = buf[(lane - 1) * kIirLdsStride + kIirT - 1];
                a2 = buf[(lane - 1) * kIirLdsStride + kIirT - 2];
            }
            LN::set(h1, ch, a1);
            LN::set(h2, ch, a2);
            wave_sync_lds();
        }
#pragma unroll
        for (int n = 0; n < kIirT; ++n) pk = lanes_absmax(pk, xr[n]);

        // pass 1 from state 0, then the scan over the lanes (iir.hip, steps 1-2)
        V E[D];
#pragma unroll
        for (int r = 0; r < D; ++r) E[r] = LN::splat(0.f);
        cs.template run<false>(xr, h1, h2, E);
        E[3] = E[2] - E[3];  // the scan's coordinates: stage 2 as (y1, y1 - y2) (loudness_host.hpp)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const uint32_t d = 1u << j;
            V t[D], r[D];
#pragma unroll
            for (int q = 0; q < D; ++q) t[q] = LN::shfl_up(E[q], d);
            matvec<D, NCH>(A.Q + (size_t)d * D * D, t, r);
            if (lane >= d) {
#pragma unroll
                for (int q = 0; q < D; ++q) E[q] += r[q];
            }
        }

        if (ti >= t_first) {
            // pass 2: lane l from E_(l-1) + M^(T l) S_in
            V s0[D];
            {
                V r[D];
                matvec<D, NCH>(A.Q + (size_t)lane * D * D, Sin, r);
#pragma unroll
                for (int q = 0; q < D; ++q) {
                    const V prev = LN::shfl_up(E[q], 1);
                    s0[q] = (lane ? prev : LN::splat(0.f)) + r[q];
                }
                s0[3] = s0[2] - s0[3];  // back to (y1, y2)
            }
            cs.template run<true>(xr, h1, h2, s0);

            // the lane's run [pos, pos + 32) inside the tile's first hop's frame
            const uint32_t pos = rem + lane * kIirT;  // < hop + 2048
            const uint32_t k = (pos >= hop) + (pos >= 2 * hop) + (pos >= 3 * hop);
            const uint32_t nxt = (k + 1) * hop - pos;  // samples of the run before the next hop starts (>= 1)
            V sa = LN::splat(0.f), sb = LN::splat(0.f);
#pragma unroll
            for (int n = 0; n < kIirT; ++n) sa = LN::fma(xr[n], xr[n], sa);
            if (nxt < (uint32_t)kIirT) {  // a boundary inside the run: the same sums, split
                sa = LN::splat(0.f);
#pragma unroll
                for (int n = 0; n < kIirT; ++n) {
                    const bool before = (uint32_t)n < nxt;
                    const V ya = lanes_sel(before, xr[n], LN::splat(0.f));
                    const V yb = lanes_sel(before, LN::splat(0.f), xr[n]);
                    sa = LN::fma(ya, ya, sa);
                    sb = LN::fma(yb, yb, sb);
                }
            }
            const uint32_t last = rem + (uint32_t)kIirTile - 1;
            const uint32_t nh = 1u + (last >= hop) + (last >= 2 * hop) + (last >= 3 * hop);  // hops the tile touches
            for (uint32_t q = 0; q < nh; ++q) {
                V a = lanes_sel(k == q, sa, LN::splat(0.f)) + lanes_sel(k + 1 == q, sb, LN::splat(0.f));
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) a += LN::shfl_xor(a, o);
                if (lane == 0) {
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch)
                        A.part[((size_t)(row0 + (uint32_t)ch) * A.tiles + ti) * kLoudSlots + q] = LN::get(a, ch);
                }
            }
        }

        // the state entering the next tile: agg + M^(64 T) S_in
        {
            V r[D];
            matvec<D, NCH>(A.P + (size_t)D * D, Sin, r);
#pragma unroll
            for (int q = 0; q < D; ++q) Sin[q] = LN::shfl(E[q], 63) + r[q];
        }
        rem += (uint32_t)kIirTile;
        while (rem >= hop) rem -= hop;
    }

#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) pk = lanes_absmax(pk, LN::shfl_xor(pk, o));
    if (lane == 0) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) atomicMax(A.peaks + row0 + (uint32_t)ch, __float_as_uint(LN::get(pk, ch)));
    }
}

// one thread per (row, hop): the hop's partials in tile order, in double
__global__ __launch_bounds__(256) void loudness_finish_kernel(LoudnessArgs A) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t row = blockIdx.y;
    if (j >= A.hops) return;
    const uint64_t n0 = j * A.hop, n1 = n0 + A.hop - 1;  // the hop's first and last sample (n1 < L)
    double s = 0.0;
    for (uint64_t t = n0 / kLoudTile; t <= n1 / kLoudTile; ++t) {
        const uint64_t q = j - (t * kLoudTile) / A.hop;  // 0..3: the tile's first hop is (t 2048) / hop <= j
        s += (double)A.part[((size_t)row * A.tiles + t) * kLoudSlots + q];
    }
    A.z[(size_t)row * A.hops + j] = s;
}

constexpr uint32_t kTpInputs = 1024;  // inputs per workgroup
constexpr uint32_t kTpSteps = 256;    // the most steps: Tp = 2 ceil(64 / 0.5)

template <int OVS>
__global__ __launch_bounds__(256) void loudness_truepeak_kernel(const float *__restrict__ const table, uint32_t steps,
                                                               uint32_t half, LoudnessArgs A) {
    __shared__ float xs[kTpInputs + kTpSteps];
    const uint32_t t = threadIdx.x, row = blockIdx.y;
    const float *__restrict__ x = A.in.p[row];
    const uint64_t nbase = (uint64_t)blockIdx.x * kTpInputs;
    // xs[e] = x[nbase - (half - 1) + e], zero outside [0, L)
    const int64_t n_lo = (int64_t)nbase - (int64_t)(half - 1);
    for (uint32_t e = t; e < kTpInputs + steps; e += 256) {
        const int64_t n = n_lo + (int64_t)e;
        xs[e] = (n >= 0 && (uint64_t)n < A.L) ? x[n] : 0.f;
    }
    __syncthreads();
    // input nbase + t + 256 k, k < 4; its OVS outputs sum table[phi][i] xs[t + 256 k + i] over i in order
    float acc[4][OVS];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int p = 0; p < OVS; ++p) acc[k][p] = 0.f;
    const float *tg = (const float *)__builtin_assume_aligned(table, 16);
    for (uint32_t i = 0; i < steps; i += 4) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float xv = xs[t + 256u * k + i + v];
#pragma unroll
                for (int p = 0; p < OVS; ++p) acc[k][p] = __builtin_fmaf(tg[(i + v) * OVS + p], xv, acc[k][p]);
            }
        }
    }
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (nbase + t + 256u * k < A.L) {
#pragma unroll
            for (int p = 0; p < OVS; ++p) m = __builtin_fmaxf(m, __builtin_fabsf(acc[k][p]));
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, o));
    // (every wave of a row meets at one word: only a wave that raises it pays for the atomic)
    uint32_t *word = A.peaks + kLoudGroup + row;
    if ((t & 63u) == 0 && __float_as_uint(m) > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(word, __float_as_uint(m));
}

int launch_loudness_kweight(const LoudnessArgs &A, uint32_t nch, hipStream_t s) {
    if (nch != 1 && nch != 2) return DSP_ERR_INVALID;
    if (A.count == 0 || A.count % nch || A.first + A.count > (uint32_t)kMaxChannels) return DSP_ERR_INVALID;
    if (A.tiles == 0) return DSP_OK;
    if (A.run == 0 || A.window == 0 || A.hop < 800) return DSP_ERR_INVALID;  // (a tile touches <= 4 hops)
    const uint64_t waves = (uint64_t)(A.count / nch) * ((A.tiles + A.run - 1) / A.run);
    const uint64_t groups = (waves + kIirWaves - 1) / kIirWaves;
    if (groups > 0x7fffffffull) return DSP_ERR_INVALID;
    if (nch == 2) hipLaunchKernelGGL(loudness_kweight_kernel<2>, dim3((uint32_t)groups), dim3(256), 0, s, A);
    else hipLaunchKernelGGL(loudness_kweight_kernel<1>, dim3((uint32_t)groups), dim3(256), 0, s, A);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

int launch_loudness_finish(const LoudnessArgs &A, uint32_t rows, hipStream_t s) {
    if (rows == 0 || rows > (uint32_t)kMaxChannels) return DSP_ERR_INVALID;
    if (A.hops == 0) return DSP_OK;
    const uint64_t groups = (A.hops + 255) / 256;
    if (groups > 0x7fffffffull) return DSP_ERR_INVALID;
    hipLaunchKernelGGL(loudness_finish_kernel, dim3((uint32_t)groups, rows), dim3(256), 0, s, A);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

int launch_loudness_truepeak(const LoudnessArgs &A, uint32_t rows, uint32_t ovs, const float *table, uint32_t steps,
                             uint32_t half, hipStream_t s) {
    if (rows == 0 || rows > (uint32_t)kMaxChannels) return DSP_ERR_INVALID;
    if (A.L == 0) return DSP_OK;
    if (steps == 0 || steps > kTpSteps || steps % 4 || half == 0 || 2 * half > steps) return DSP_ERR_INVALID;
    const uint64_t groups = (A.L + kTpInputs - 1) / kTpInputs;
    if (groups > 0x7fffffffull) {
        set_last_error("dsp_loudness: more than 2^31 true-peak tiles");
        return DSP_ERR_UNSUPPORTED;
    }
    const dim3 grid((uint32_t)groups, rows);
    if (ovs == 4) hipLaunchKernelGGL(loudness_truepeak_kernel<4>, grid, dim3(256), 0, s, table, steps, half, A);
    else if (ovs == 2) hipLaunchKernelGGL(loudness_truepeak_kernel<2>, grid, dim3(256), 0, s, table, steps, half, A);
    else return DSP_ERR_INVALID;
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

}  // namespace dspb
