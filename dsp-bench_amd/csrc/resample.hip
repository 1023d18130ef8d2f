// resample.hip -- dsp_resample: rational sample-rate conversion by a polyphase
// Kaiser-windowed sinc (dspbench.h, host_tables.cpp resample_plan / _table).
//
//   y[m] = sum_{i < Tp} table[phi][i] x[n0 - half + 1 + i],
//   q = m down, n0 = q / up, phi = q % up, x = 0 outside [0, L)
//
// Outputs of one phase, m = r + j up, read inputs n0(r) + j down: a wave that
// owns one phase over 64 consecutive j has wave-uniform taps.
//
// resample_phase_kernel<R> (the fast path, wherever its tile fits in LDS): a
// workgroup of 4 waves owns J = 64 JC periods -- J down inputs, J up outputs
// -- and stages the inputs plus the filter's halo once in LDS.  A wave takes
// tasks (group g of R consecutive phases, chunk jc of 64 periods); lane l is
// period j = 64 jc + l.  The R phases of a group read windows that start
// d_k = n0(g R + k) - n0(g R) samples apart, so the wave sweeps the union
// window once: per step s one LDS read of x and R FMAs with the R taps of
// that step, which the scalar unit loads as one aligned vector from the
// device table gt[g][s][k] = table[phi_k][s - d_k] (zero where s - d_k is
// outside [0, Tp), and for the phases past `up` of the last group: y's sum is
// the definition's products in the order i = 0 .. Tp - 1, with zero products
// before and after).  Results
// go through an LDS image of the tile's outputs, then out as contiguous
// dwordx4 stores.
//
// LDS banks: lanes read x `down` apart.  Odd down: every lane of a half-wave
// on its own bank.  down = o 2^a: the staged span is stored as 2^a regions,
// sample e in region e mod 2^a at e >> a, so that the lanes of one read (all
// the same e mod 2^a) sit o apart -- odd again.  The output image pads one
// slot every 32 (lanes write `up` apart).
//
// resample_direct_kernel (every other accepted plan: a tile that does not fit
// in LDS, i.e. a large up or down): one output per lane, x and taps straight
// from global memory through the caches (the device table is then the plain
// table[phi][i]), every bound checked.  Correct for every plan; slow.
//
// Index arithmetic: a tile's first input tile J down - half + 1 (phase
// kernel) or its n0 = (m0 down) / up (direct kernel) is computed once in 64
// bits; everything past it is 32-bit.
#include <algorithm>

#include "kernels.hpp"

namespace dspb {

constexpr uint32_t kRsLdsMax = 160u * 1024u;  // one workgroup may use the CU's whole LDS
constexpr uint32_t kRsLdsTwo = 80u * 1024u;   // two workgroups per CU

__device__ __forceinline__ uint32_t rs_yslot(uint32_t e) { return e + (e >> 5); }

template <int R>
__global__ __launch_bounds__(256) void resample_phase_kernel(const ResampleArgs A) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    float *xs = rs_lds;
    float *ys = rs_lds + A.xfloats;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t tile = blockIdx.x;
    const uint32_t J = 64u * A.JC;
    const float *__restrict__ x = A.in.p[blockIdx.y];
    float *__restrict__ y = A.out.p[blockIdx.y];

    // stage inputs [nbase, nbase + xspan): sample e at region e & amask, slot e >> a
    const int64_t nbase = (int64_t)((uint64_t)tile * J * A.down) - (int64_t)(A.half - 1);
    const uint32_t a = A.a, amask = (1u << a) - 1u, hreg = A.hreg;
    if (nbase >= 0 && (uint64_t)nbase + A.xspan <= A.L) {  // interior tile: no checks
        const float *xb = x + nbase;
        for (uint32_t e = t; e < A.xspan; e += 256) xs[(e >> a) + (e & amask) * hreg] = xb[e];
    } else {  // an edge of the file: zeros outside [0, L)
        for (uint32_t e = t; e < A.xspan; e += 256) {
            const int64_t n = nbase + (int64_t)e;
            xs[(e >> a) + (e & amask) * hreg] = (n >= 0 && (uint64_t)n < A.L) ? x[n] : 0.f;
        }
    }
    __syncthreads();

    const uint32_t ngroups = (A.up + R - 1) / R, ntasks = ngroups * A.JC;
    const uint32_t lane_x = lane * (A.down >> a);  // lane's offset inside a region
    for (uint32_t task = wave; task < ntasks; task += 4) {
        const uint32_t g = task % ngroups, jc = task / ngroups;
        const uint32_t n0g = (g * R * A.down) / A.up;
        // the group's taps, [s][k]: 16-byte aligned (S % 4 == 0)
        const float *tg = (const float *)__builtin_assume_aligned(A.table + (size_t)g * A.S * R, 16);
        float acc[R];
#pragma unroll
        for (int k = 0; k < R; ++k) acc[k] = 0.f;
        const uint32_t cu = n0g + jc * 64u * A.down;  // uniform: first sample of lane 0's union window
        if (a == 0) {
            const float *xp = xs + cu + lane_x;
            for (uint32_t s = 0; s < A.S; s += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float xv = xp[s + u];
#pragma unroll
                    for (int k = 0; k < R; ++k) acc[k] = __builtin_fmaf(tg[(s + u) * R + k], xv, acc[k]);
                }
            }
        } else {
            const float *xp = xs + lane_x;
            for (uint32_t s = 0; s < A.S; s += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t e = cu + s + u;  // uniform
                    const float xv = xp[(e >> a) + (e & amask) * hreg];
#pragma unroll
                    for (int k = 0; k < R; ++k) acc[k] = __builtin_fmaf(tg[(s + u) * R + k], xv, acc[k]);
                }
            }
        }
        const uint32_t j = jc * 64u + lane;
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (g * R + k < A.up) ys[rs_yslot(g * R + k + j * A.up)] = acc[k];
    }
    __syncthreads();

    // the tile's J up outputs, contiguous from m0
    const uint32_t nout = J * A.up;  // a multiple of 64
    const uint64_t m0 = (uint64_t)tile * nout;
    if (A.out_aligned16 && m0 + nout <= A.Lout) {
        float4 *y4 = reinterpret_cast<float4 *>(y + m0);
        for (uint32_t e = 4 * t; e < nout; e += 1024) {
            const float *p = ys + rs_yslot(e);  // e % 4 == 0: the four share a 32-block
            y4[e >> 2] = float4{p[0], p[1], p[2], p[3]};
        }
    } else {
        const uint64_t left = A.Lout - m0;  // the grid has no tile past Lout
        const uint32_t n = left < nout ? (uint32_t)left : nout;
        float *yb = y + m0;
        for (uint32_t e = t; e < n; e += 256) yb[e] = ys[rs_yslot(e)];
    }
}

// one output per lane; tiles of 256 consecutive outputs
__global__ __launch_bounds__(256) void resample_direct_kernel(const ResampleArgs A) {
    const float *__restrict__ x = A.in.p[blockIdx.y];
    float *__restrict__ y = A.out.p[blockIdx.y];
    const uint64_t m0 = (uint64_t)blockIdx.x * 256u;
    const uint64_t q0 = m0 * A.down;  // < 2^63 + (host: L up < 2^63, m0 < Lout)
    const uint64_t nb = q0 / A.up;
    const uint32_t phib = (uint32_t)(q0 % A.up);
    const uint32_t t = threadIdx.x;
    if (m0 + t >= A.Lout) return;
    const uint32_t ql = phib + t * A.down;  // < 4096 + 256 * 2^22 (host)
    const uint32_t nl = ql / A.up, phi = ql % A.up;
    // first input of the window, relative to the file
    const int64_t w0 = (int64_t)nb + (int64_t)nl - (int64_t)(A.half - 1);
    const uint32_t lo = w0 < 0 ? (uint32_t)(-w0 < (int64_t)A.Tp ? -w0 : (int64_t)A.Tp) : 0u;
    const int64_t room = (int64_t)A.L - w0;  // taps that stay below L
    const uint32_t hi = room <= 0 ? 0u : (room < (int64_t)A.Tp ? (uint32_t)room : A.Tp);
    const float *tp = A.table + (size_t)phi * A.Tp;
    const float *xw = x + w0;
    float acc = 0.f;
    for (uint32_t i = lo; i < hi; ++i) acc = __builtin_fmaf(tp[i], xw[i], acc);
    y[m0 + t] = acc;
}

// phases per group of the phase kernel
static uint32_t rs_group(uint32_t up) { return up >= 3 ? 4u : up; }

// the largest window offset d_k inside a group of R phases
static uint32_t rs_pad(uint32_t up, uint32_t down, uint32_t R) {
    uint32_t pad = 0;
    for (uint32_t g = 0; g * R < up; ++g) {
        const uint32_t last = std::min(g * R + R - 1, up - 1);
        pad = std::max(pad, (uint32_t)(((uint64_t)last * down) / up - ((uint64_t)g * R * down) / up));
    }
    return pad;
}

// The kernel and blocking of a plan (up, down, Tp set in *A): the phase
// kernel's R, S, JC and LDS layout when a tile of 64 periods fits in LDS,
// else the direct kernel.  A function of (up, down, Tp) alone.
void resample_blocking(ResampleArgs *A) {
    const uint32_t up = A->up, down = A->down;
    A->phase = 0;
    A->R = A->S = A->JC = A->a = A->hreg = A->xspan = A->xfloats = A->lds_bytes = 0;
    if (up > 4096u || down > 4096u) return;  // (keeps every product of the phase kernel below 32 bits)
    const uint32_t R = rs_group(up);
    const uint32_t S = (A->Tp + rs_pad(up, down, R) + 3) & ~3u;
    uint32_t a = 0;
    while (!((down >> a) & 1u)) ++a;
    const uint32_t ngroups = (up + R - 1) / R;
    auto lds_of = [&](uint32_t JC, uint32_t *xspan, uint32_t *hreg, uint32_t *xfloats) {
        const uint64_t J = 64ull * JC;
        const uint64_t span = J * down + S;
        const uint64_t hr = (span + (1u << a) - 1) >> a;
        const uint64_t xf = ((hr << a) + 3) & ~3ull;
        const uint64_t yf = J * up + (J * up >> 5) + 4;
        *xspan = (uint32_t)span;
        *hreg = (uint32_t)hr;
        *xfloats = (uint32_t)xf;
        return (xf + yf) * 4;
    };
    uint32_t JC = 1, xspan, hreg, xfloats;
    uint64_t bytes = lds_of(1, &xspan, &hreg, &xfloats);
    if (bytes > kRsLdsMax) return;
    // few phases: more periods per tile, until every wave has two tasks
    while (ngroups * JC < 8 && JC < 16) {
        uint32_t xs2, hr2, xf2;
        const uint64_t b2 = lds_of(JC * 2, &xs2, &hr2, &xf2);
        if (b2 > kRsLdsTwo) break;
        JC *= 2, xspan = xs2, hreg = hr2, xfloats = xf2, bytes = b2;
    }
    A->phase = 1;
    A->R = R;
    A->S = S;
    A->JC = JC;
    A->a = a;
    A->hreg = hreg;
    A->xspan = xspan;
    A->xfloats = xfloats;
    A->lds_bytes = (uint32_t)bytes;
}

uint64_t resample_device_floats(const ResampleArgs &A) {
    if (!A.phase) return (uint64_t)A.up * A.Tp;
    return (uint64_t)((A.up + A.R - 1) / A.R) * A.S * A.R;
}

// the device table of a blocking from the plain table[phi][i]
void resample_device_table(const ResampleArgs &A, const float *plain, float *out) {
    const uint64_t n = resample_device_floats(A);
    if (!A.phase) {
        std::copy(plain, plain + n, out);
        return;
    }
    std::fill(out, out + n, 0.f);
    const uint32_t R = A.R;
    for (uint32_t r = 0; r < A.up; ++r) {
        const uint32_t g = r / R, k = r % R;
        const uint64_t q = (uint64_t)r * A.down;
        const uint32_t phi = (uint32_t)(q % A.up);
        const uint32_t d = (uint32_t)(q / A.up - ((uint64_t)g * R * A.down) / A.up);
        for (uint32_t i = 0; i < A.Tp; ++i)
            out[((uint64_t)g * A.S + d + i) * R + k] = plain[(uint64_t)phi * A.Tp + i];
    }
}

template <int R>
static int launch_phase(const ResampleArgs &A, dim3 grid, hipStream_t s) {
    if (A.lds_bytes > 64u * 1024u)  // (per device: set on every such launch, a host-side call)
        DSPB_HIP(hipFuncSetAttribute((const void *)resample_phase_kernel<R>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRsLdsMax));
    hipLaunchKernelGGL(resample_phase_kernel<R>, grid, dim3(256), A.lds_bytes, s, A);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

int launch_resample(const ResampleArgs &A, uint32_t C, hipStream_t s) {
    if (A.Lout == 0 || C == 0) return DSP_OK;
    if (C > (uint32_t)kMaxChannels) return DSP_ERR_INVALID;
    if (A.phase) {
        const uint64_t per = 64ull * A.JC * A.up;
        const uint64_t tiles = (A.Lout + per - 1) / per;
        if (tiles > 0x7fffffffull) {
            set_last_error("dsp_resample: more than 2^31 tiles");
            return DSP_ERR_UNSUPPORTED;
        }
        const dim3 grid((uint32_t)tiles, C);
        switch (A.R) {
        case 1: return launch_phase<1>(A, grid, s);
        case 2: return launch_phase<2>(A, grid, s);
        default: return launch_phase<4>(A, grid, s);
        }
    }
    const uint64_t tiles = (A.Lout + 255) / 256;
    if (tiles > 0x7fffffffull) {
        set_last_error("dsp_resample: more than 2^31 tiles");
        return DSP_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(resample_direct_kernel, dim3((uint32_t)tiles, C), dim3(256), 0, s, A);
    DSPB_HIP(hipGetLastError());
    return DSP_OK;
}

}  // namespace dspb
