// limiter.hip -- dsp_limiter (dspbench.h): a look-ahead peak limiter in three
// launches, none of which waits for another workgroup.
//
// A tile is 2048 samples of a link group, one workgroup of 256 threads; the
// tile grid is anchored at sample 0.
//
// limiter_detect_kernel<OVS> (pass 1): the detector p over the tile and A
// samples to its right, channel after channel (sample mode: |x| from global
// memory; OVS > 1: the row staged in LDS with the oversampler's halo and the
// polyphase sums of loudness_truepeak_kernel, taps by scalar loads, products
// in the definition's order, the maximum kept per input sample), the needed
// attenuation a, the forward sliding maximum h over A + 1 samples by log-step
// doubling in LDS (max is exact: any order gives the same bits), h to the
// group's scratch row, p to the detector row, and the tile's aggregate E =
// e at the tile's end from a zero start (tile_scan).
//
// limiter_carry_kernel (pass 2): one wave per group walks the tiles in order,
// 64 aggregates per load: carry[t + 1] = max(E[t], rho^2048 carry[t]).
//
// limiter_apply_kernel (pass 3): e over the tile from its carry and, for the
// A samples before it, over the previous tile from that tile's carry (the
// same tile_scan, so an e has one value wherever it is computed); e in LDS,
// the smoothing sum s over k = 0..A in order, 8 consecutive outputs per
// thread from a sliding register window, w by scalar loads (a tile whose e are
// all zero skips the sum: it is +0 either way); g = 1 - s, y = clamp(x g) for
// every channel of the group, the gain row, and per wave the minimum of g and
// the count of g < 1 (integer atomics, issued only where they change the
// word).
//
// tile_scan: thread t owns samples [8 t, 8 t + 8) of the tile.  It runs the
// recurrence serially from zero, the wave scans the lanes' ends with the
// decays rho^(8 2^i), the four waves' ends are folded in order with rho^512,
// and the value entering a lane reaches sample i through rho^(i + 1).  Every
// power is float64 rounded once (limiter_host.hpp limiter_table); rho = 0
// makes every decayed term +0 and A = 0 makes the sum 1 e: no special path.
#include "kernels.hpp"
#include "limiter_host.hpp"

namespace dspb {

constexpr uint32_t kLimSpan = kLimTile + kLimMaxLookahead;  // pass 1: the tile and its look-ahead
constexpr uint32_t kLimSteps = 256;                         // the oversampler's most steps (loudness.hip)
constexpr uint32_t kLimFront = kLimMaxLookahead + 8;        // pass 3: e before the tile, and one window refill

__device__ __forceinline__ float lim_max(float a, float b) { return __builtin_fmaxf(a, b); }

// e[0..8) of the thread's samples from h[0..8) and the carry entering the tile;
// returns e at the tile's end.  Every thread of the workgroup calls it.
__device__ __forceinline__ float tile_scan(const float (&h)[kLimLane], float (&e)[kLimLane], float carry,
                                           const float *__restrict__ tab, float *wagg) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float rho = tab[1];
    e[0] = h[0];
#pragma unroll
    for (int i = 1; i < (int)kLimLane; ++i) e[i] = lim_max(h[i], rho * e[i - 1]);
    float v = e[kLimLane - 1];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const uint32_t d = 1u << j;
        const float u = __shfl_up(v, d);
        const float pw = tab[kLimTabLane + d];
        if (lane >= d) v = lim_max(v, pw * u);
    }
    if (lane == 63u) wagg[wave] = v;
    __syncthreads();
    const float pwave = tab[kLimTabWave];
    float winc = carry, end = carry;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        end = lim_max(wagg[w], pwave * end);
        if (w + 1 == wave) winc = end;
    }
    const float prev = __shfl_up(v, 1);
    const float inc = lim_max(lane ? prev : 0.f, tab[kLimTabLane + lane] * winc);
#pragma unroll
    for (int i = 0; i < (int)kLimLane; ++i) e[i] = lim_max(e[i], tab[i + 1] * inc);
    __syncthreads();  // (wagg is free again)
    return end;
}

template <int OVS>
__global__ __launch_bounds__(256) void limiter_detect_kernel(LimiterArgs A) {
    __shared__ __attribute__((aligned(16))) float ab[kLimSpan];
    __shared__ float xs[OVS > 1 ? kLimSpan + kLimSteps : 1];
    __shared__ float wagg[4];
    const uint32_t t = threadIdx.x, grp = blockIdx.y;
    const uint64_t tile = blockIdx.x, start = tile * kLimTile, rowlen = A.tiles * kLimTile;
    const uint32_t n_in = A.pmode ? kLimTile : kLimTile + A.A;  // detector samples of this workgroup
    constexpr int NK = kLimSpan / 256;
    float p[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) p[k] = 0.f;

    for (uint32_t ch = 0; ch < A.nch; ++ch) {
        const float *__restrict__ x = A.in.p[grp * A.nch + ch];
        if constexpr (OVS > 1) {
            // xs[e] = x[start - (half - 1) + e], zero outside [0, L)
            const uint32_t chunks = (n_in + 1023u) / 1024u;
            const uint32_t fill = chunks * 1024u + A.steps;
            const int64_t n_lo = (int64_t)start - (int64_t)(A.half - 1);
            if (n_lo >= 0 && (uint64_t)n_lo + fill <= A.L) {  // an interior tile: no checks
                for (uint32_t e = t; e < fill; e += 256) xs[e] = x[n_lo + e];
            } else {
                for (uint32_t e = t; e < fill; e += 256) {
                    const int64_t n = n_lo + (int64_t)e;
                    xs[e] = (n >= 0 && (uint64_t)n < A.L) ? x[n] : 0.f;
                }
            }
            __syncthreads();
            const float *tg = (const float *)__builtin_assume_aligned(A.tp, 16);
#pragma unroll
            for (int kk = 0; kk < NK / 4; ++kk) {
                if ((uint32_t)kk * 1024u < n_in) {
                    // input kk 1024 + t + 256 k, k < 4: its OVS outputs, products over i in order
                    float acc[4][OVS];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int q = 0; q < OVS; ++q) acc[k][q] = 0.f;
                    const float *xk = xs + kk * 1024 + t;
                    for (uint32_t i = 0; i < A.steps; i += 4) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const float xv = xk[256u * k + i + v];
#pragma unroll
                                for (int q = 0; q < OVS; ++q)
                                    acc[k][q] = __builtin_fmaf(tg[(i + v) * OVS + q], xv, acc[k][q]);
                            }
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float m = __builtin_fabsf(xk[256u * k + A.half - 1]);
#pragma unroll
                        for (int q = 0; q < OVS; ++q) m = lim_max(m, __builtin_fabsf(acc[k][q]));
                        p[kk * 4 + k] = lim_max(p[kk * 4 + k], m);
                    }
                }
            }
            __syncthreads();  // (xs is staged again for the next channel)
        } else {
            if (start + n_in <= A.L) {  // an interior tile: no checks against L
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const uint32_t e = t + 256u * k;
                    if (e < n_in) p[k] = lim_max(p[k], __builtin_fabsf(x[start + e]));
                }
            } else {
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const uint32_t e = t + 256u * k;
                    if (e < n_in && start + e < A.L) p[k] = lim_max(p[k], __builtin_fabsf(x[start + e]));
                }
            }
        }
    }

    // a linked group of more than 16 channels: p over the earlier launches' rows
    if (A.pmode == 2 || A.use_pmax) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const uint32_t e = t + 256u * k;
            if (e < n_in && start + e < A.L) p[k] = lim_max(p[k], A.pmax[start + e]);
        }
    }
    if (A.pmode) {
#pragma unroll
        for (int k = 0; k < (int)(kLimTile / 256); ++k) {
            const uint32_t e = t + 256u * k;
            if (start + e < A.L) A.pmax[start + e] = p[k];
        }
        return;
    }

    float *det = A.det.p[grp];
    if (det) {
#pragma unroll
        for (int k = 0; k < (int)(kLimTile / 256); ++k) {
            const uint32_t e = t + 256u * k;
            if (start + e < A.L) det[start + e] = p[k];
        }
    }
    // the needed attenuation (IEEE division; 0 past the rows' end)
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const uint32_t e = t + 256u * k;
        if (e < n_in) ab[e] = (start + e < A.L && p[k] > A.c) ? 1.f - A.c / p[k] : 0.f;
    }
    __syncthreads();
    // h[e] = max ab[e .. e + A]: windows of 1, 2, 4, .. cw <= A + 1, then two of them
    const uint32_t W = A.A + 1;
    uint32_t cw = 1;
    while (cw < W) {
        const uint32_t d = 2 * cw <= W ? cw : W - cw;
        float r[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const uint32_t e = t + 256u * k;
            r[k] = e + d < n_in ? ab[e + d] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const uint32_t e = t + 256u * k;
            if (e < n_in) ab[e] = lim_max(ab[e], r[k]);
        }
        __syncthreads();
        cw += d;
    }
    float *hrow = A.h + (uint64_t)grp * rowlen + start;  // (the row holds whole tiles)
#pragma unroll
    for (int k = 0; k < (int)(kLimTile / 256); ++k) hrow[t + 256u * k] = ab[t + 256u * k];
    float hv[kLimLane], ev[kLimLane];
    {
        const float4 *a4 = reinterpret_cast<const float4 *>(ab + kLimLane * t);
        const float4 u = a4[0], v = a4[1];
        hv[0] = u.x, hv[1] = u.y, hv[2] = u.z, hv[3] = u.w, hv[4] = v.x, hv[5] = v.y, hv[6] = v.z, hv[7] = v.w;
    }
    const float end = tile_scan(hv, ev, 0.f, A.tab, wagg);
    if (t == 0) A.E[(uint64_t)grp * A.tiles + tile] = end;
}

__global__ __launch_bounds__(64) void limiter_carry_kernel(LimiterArgs A) {
    const uint32_t lane = threadIdx.x, grp = blockIdx.x;
    const float ptile = A.tab[kLimTabTile];
    const float *__restrict__ E = A.E + (uint64_t)grp * A.tiles;
    float *cy = A.carry + (uint64_t)grp * A.tiles;
    float c = 0.f;
    float nxt = lane < A.tiles ? E[lane] : 0.f;
    for (uint64_t base = 0; base < A.tiles; base += 64) {
        const float cur = nxt;
        const uint64_t nb = base + 64 + lane;
        nxt = nb < A.tiles ? E[nb] : 0.f;  // the next 64, on its way during this walk
        float mine = 0.f;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            if (lane == (uint32_t)j) mine = c;
            c = lim_max(__shfl(cur, j), ptile * c);
        }
        if (base + lane < A.tiles) cy[base + lane] = mine;
    }
}

__global__ __launch_bounds__(256) void limiter_apply_kernel(LimiterArgs A) {
    __shared__ __attribute__((aligned(16))) float eb[kLimFront + kLimTile];  // eb[kLimFront + i] = e[start + i]
    __shared__ float wagg[4];
    const uint32_t t = threadIdx.x, grp = blockIdx.y, lane = t & 63u;
    const uint64_t tile = blockIdx.x, start = tile * kLimTile, rowlen = A.tiles * kLimTile;
    const float *__restrict__ hrow = A.h + (uint64_t)grp * rowlen;
    const float *__restrict__ cy = A.carry + (uint64_t)grp * A.tiles;

    for (uint32_t e = t; e < kLimFront; e += 256) eb[e] = 0.f;  // e[j < 0] = 0, and the window's padding
    __syncthreads();
    float hv[kLimLane], ev[kLimLane];
    auto load_h = [&](uint64_t at) {
        const float4 *h4 = reinterpret_cast<const float4 *>(hrow + at + kLimLane * t);
        const float4 u = h4[0], v = h4[1];
        hv[0] = u.x, hv[1] = u.y, hv[2] = u.z, hv[3] = u.w, hv[4] = v.x, hv[5] = v.y, hv[6] = v.z, hv[7] = v.w;
    };
    auto store_e = [&](uint32_t at) {
        float4 *e4 = reinterpret_cast<float4 *>(eb + at);
        e4[0] = float4{ev[0], ev[1], ev[2], ev[3]};
        e4[1] = float4{ev[4], ev[5], ev[6], ev[7]};
    };
    int any = 0;
    if (A.A > 0 && tile > 0) {  // the previous tile again, for its last 1024 e
        load_h(start - kLimTile);
        (void)tile_scan(hv, ev, cy[tile - 1], A.tab, wagg);
        if (kLimLane * t >= kLimTile - kLimMaxLookahead) {
            store_e(kLimFront - kLimTile + kLimLane * t);
#pragma unroll
            for (int i = 0; i < (int)kLimLane; ++i) any |= ev[i] != 0.f;
        }
    }
    load_h(start);
    (void)tile_scan(hv, ev, cy[tile], A.tab, wagg);
    store_e(kLimFront + kLimLane * t);
#pragma unroll
    for (int i = 0; i < (int)kLimLane; ++i) any |= ev[i] != 0.f;
    any = __syncthreads_or(any);

    float s[kLimLane];
#pragma unroll
    for (int i = 0; i < (int)kLimLane; ++i) s[i] = 0.f;
    if (any) {  // (all e zero: every product is +0, and so is the sum)
        const float *__restrict__ w = A.tab + kLimTabWindow;
        const uint32_t base = kLimFront + kLimLane * t;
        float win[16];  // win[j] = eb[base - kb - 8 + j]
        {
            const float4 *e4 = reinterpret_cast<const float4 *>(eb + base);
            const float4 u = e4[0], v = e4[1];
            win[0] = u.x, win[1] = u.y, win[2] = u.z, win[3] = u.w, win[4] = v.x, win[5] = v.y, win[6] = v.z, win[7] = v.w;
        }
        for (uint32_t kb = 0; kb < A.wpad; kb += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) win[8 + j] = win[j];
            const float4 *e4 = reinterpret_cast<const float4 *>(eb + base - kb - 8);
            const float4 u = e4[0], v = e4[1];
            win[0] = u.x, win[1] = u.y, win[2] = u.z, win[3] = u.w, win[4] = v.x, win[5] = v.y, win[6] = v.z, win[7] = v.w;
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const float wk = w[kb + kk];
#pragma unroll
                for (int i = 0; i < (int)kLimLane; ++i) s[i] = __builtin_fmaf(wk, win[8 + i - kk], s[i]);
            }
        }
    }

    const uint64_t n0 = start + kLimLane * t;
    float g[kLimLane], gmin = 1.f;
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < (int)kLimLane; ++i) {
        g[i] = 1.f - s[i];
        if (n0 + i < A.L) {
            gmin = __builtin_fminf(gmin, g[i]);
            cnt += g[i] < 1.f;
        }
    }
    const bool whole = start + kLimTile <= A.L;  // the workgroup's branch: a full tile takes no checks
    const float c = A.c;
    for (uint32_t ch = 0; ch < A.nch; ++ch) {
        const float *x = A.in.p[grp * A.nch + ch];  // (may be the output row: no __restrict__)
        float *y = A.out.p[grp * A.nch + ch];
        if (whole && A.in_aligned16 && A.out_aligned16) {
            const float4 *x4 = reinterpret_cast<const float4 *>(x + n0);
            float4 *y4 = reinterpret_cast<float4 *>(y + n0);
            const float4 u = x4[0], v = x4[1];
            const float xv[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
            float yv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) yv[i] = __builtin_fminf(lim_max(xv[i] * g[i], -c), c);
            y4[0] = float4{yv[0], yv[1], yv[2], yv[3]};
            y4[1] = float4{yv[4], yv[5], yv[6], yv[7]};
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (n0 + i < A.L) y[n0 + i] = __builtin_fminf(lim_max(x[n0 + i] * g[i], -c), c);
        }
    }
    float *grow = A.gain.p[grp];
    if (grow) {
        if (whole && A.gain_aligned16) {
            float4 *g4 = reinterpret_cast<float4 *>(grow + n0);
            g4[0] = float4{g[0], g[1], g[2], g[3]};
            g4[1] = float4{g[4], g[5], g[6], g[7]};
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (n0 + i < A.L) grow[n0 + i] = g[i];
        }
    }
    if (A.words) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            gmin = __builtin_fminf(gmin, __shfl_xor(gmin, o));
            cnt += __shfl_xor(cnt, o);
        }
        if (lane == 0) {
            // floats in their order as unsigned keys (g may round below zero)
            const uint32_t b = __float_as_uint(gmin), key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
            // (only a wave that lowers the word pays for the atomic)
            if (key < __hip_atomic_load(A.words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(A.words, key);
            if (cnt) atomicAdd(reinterpret_cast<unsigned long long *>(A.words + 2), (unsigned long long)cnt);
        }
    }
}

static int limiter_args_ok(const LimiterArgs &A) {
    if (A.ngroups == 0 || A.nch == 0 || A.ngroups * A.nch > (uint32_t)kMaxChannels) return DSP_ERR_INVALID;
    if (A.A > kLimMaxLookahead || A.wpad != ((A.A + 8) & ~7u) || !A.tab || !A.h || !A.E || !A.carry)
        return DSP_ERR_INVALID;
    if (A.tiles != A.L / kLimTile + (A.L % kLimTile ? 1 : 0)) return DSP_ERR_INVALID;
    if (A.tiles > 0x7fffffffull) {
        set_last_error("dsp_limiter: more than 2^31 tiles");
        return DSP_ERR_UNSUPPORTED;
    }
    return DSP_OK;
}

int launch_limiter_detect(const LimiterArgs &A, uint32_t ovs, hipStream_t s) {
    if (int st = limiter_args_ok(A)) return st;
    if (A.tiles == 0) return DSP_OK;
    if ((A.pmode || A.use_pmax) && !A.pmax) return DSP_ERR_INVALID;
    if (A.pmode > 2 || (A.pmode && A.ngroups != 1)) return DSP_ERR_INVALID;
    const dim3 grid((uint32_t)A.tiles, A.ngroups);
    if (ovs == 1) {
        hipLaunchKernelGGL(limiter_detect_kernel<1>, grid, dim3(256), 0, s, A);
    } else {
        if (!A.tp || A.steps == 0 || A.steps > kLimSteps || A.steps % 4 || A.half == 0 || 2 * A.half > A.steps)
            return DSP_ERR_INVALID;
        if (ovs == 4) hipLaunchKernelGGL(limiter_detect_kernel<4>, grid, dim3(256), 0, s, A);
        else if (ovs == 2) hipLaunchKernelGGL(limiter_detect_kernel<2>, grid, dim3(256), 0, s, A);
        else return DSP_ERR_INVALID;
    }
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

int launch_limiter_carry(const LimiterArgs &A, hipStream_t s) {
    if (int st = limiter_args_ok(A)) return st;
    if (A.tiles == 0) return DSP_OK;
    hipLaunchKernelGGL(limiter_carry_kernel, dim3(A.ngroups), dim3(64), 0, s, A);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

int launch_limiter_apply(const LimiterArgs &A, hipStream_t s) {
    if (int st = limiter_args_ok(A)) return st;
    if (A.tiles == 0) return DSP_OK;
    hipLaunchKernelGGL(limiter_apply_kernel, dim3((uint32_t)A.tiles, A.ngroups), dim3(256), 0, s, A);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

}  // namespace dspb
