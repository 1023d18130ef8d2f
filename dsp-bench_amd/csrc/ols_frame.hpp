// ols_frame.hpp -- the parts of an 8192-point real overlap-save frame shared by
// the FIR (fir_fft.hip, forward + H + inverse in one wave) and the partitioned
// convolution (conv_fdl.hip, forward and inverse as separate stages): the
// stage twiddles, the frame load with its bounds-checked EDGE variant, and the
// paired real split in both directions.  See fir_fft.hip for the index math.
#pragma once
#include "fft_pk.hpp"

namespace dspb {

// twiddles for the 4096-point passes; `salt` is an opaque zero so that the
// second load (for the inverse) is not merged with the first and the
// compiler does not keep 30 VGPRs of twiddles live across the whole frame
__device__ __forceinline__ void load_stage_tw(const v2f *tw, uint32_t lane, uint32_t salt, cx (&tlo)[8],
                                              cx2 (&thp)[4]) {
    const v2f *t = tw + salt;
#pragma unroll
    for (int j = 1; j < 8; ++j) {
        const v2f a = (t + 8192u + 64u * (uint32_t)(j - 1))[lane];
        tlo[j] = cx{a.x, a.y};
    }
    const float4 *tp4 = reinterpret_cast<const float4 *>(t + 8192u + 896u);
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const float4 q = tp4[64u * (uint32_t)h + lane];
        thp[h] = cx2{v2f{q.x, q.y}, v2f{q.z, q.w}};
    }
}

// the frame starting at sample fs (even) of x (L samples, nullptr: a channel
// the file does not have): v[b] = (x[fs + 2l + 128b], x[fs + 2l + 128b + 1]),
// zero outside [0, L), packed as the transform's input pairs.
// EDGE: frames that reach before sample 0 or past L (bounds-checked loads)
template <bool EDGE>
__device__ __forceinline__ void ols_load_frame(const float *x, int64_t fs, uint64_t L, uint32_t lane,
                                               cx2 (&P)[32]) {
    cx v[64];
    if constexpr (!EDGE) {
        if (x != nullptr) {
#pragma unroll
            for (int b = 0; b < 64; ++b) {
                const v2f t = reinterpret_cast<const v2f *>(x + fs + 128 * b)[lane];
                v[b] = cx{t.x, t.y};
            }
        } else {  // a channel the file does not have: silence
#pragma unroll
            for (int b = 0; b < 64; ++b) v[b] = cx{0.f, 0.f};
        }
    } else {
#pragma unroll
        for (int b = 0; b < 64; ++b) {
            const int64_t s = fs + 2 * (int64_t)lane + 128 * b;
            v[b] = cx{(x && s >= 0 && (uint64_t)s < L) ? x[s] : 0.f,
                      (x && s + 1 >= 0 && (uint64_t)(s + 1) < L) ? x[s + 1] : 0.f};
        }
    }
#pragma unroll
    for (int j = 0; j < 32; ++j)
        P[j] = cx2{v2f{v[2 * j].r, v[2 * j + 1].r}, v2f{v[2 * j].i, v[2 * j + 1].i}};
}

// ols_load_frame for a frame that lies wholly inside its row and starts at any
// sample (an odd hop, a row 4 bytes past a boundary): 4-byte-aligned 8-byte
// loads, and the window w2[m] = (w[2m], w[2m+1]) applied to the pairs (welch.hip,
// stft_cx.hip)
typedef v2f v2f_a4 __attribute__((aligned(4)));
__device__ __forceinline__ void welch_load_frame(const float *x, const v2f *w2, uint32_t lane, cx2 (&P)[32]) {
    cx v[64];
#pragma unroll
    for (int b = 0; b < 64; ++b) {
        const v2f t = reinterpret_cast<const v2f_a4 *>(x + 128 * b)[lane];
        const v2f w = w2[64 * b + lane];
        v[b] = cx{t.x * w.x, t.y * w.y};
    }
#pragma unroll
    for (int j = 0; j < 32; ++j)
        P[j] = cx2{v2f{v[2 * j].r, v[2 * j + 1].r}, v2f{v[2 * j].i, v[2 * j + 1].i}};
}

// per-lane constants of the split: the partner lane 64 - l (as a ds_bpermute
// byte address) and W8192^l
struct OlsLane {
    uint32_t src;
    bool l0;
    cx wl;
};
__device__ __forceinline__ OlsLane ols_lane(const v2f *tw, uint32_t lane) {
    const v2f wl2 = tw[lane];
    return OlsLane{((64u - lane) & 63u) * 4u, lane == 0, cx{wl2.x, wl2.y}};
}

// W8192^k for the pair k = l + 64 ka, k + 1024
__device__ __forceinline__ cx2 ols_tw(const OlsLane &ln, int ka) {
    return cmulb(ln.wl, cx2{v2f{kW128_re[ka], kW128_re[ka + 16]}, v2f{kW128_im[ka], kW128_im[ka + 16]}});
}

// forward split of the pair (ka, ka + 16), ka < 16, from the packed transform
// Z = (zp, zm): X1 = 2 X[k], X2 = conj 2 X[M - k] for k = l + 64 ka and
// k + 1024, the M - k half fetched from lane 64 - l (lane 0 pairs with itself,
// shifted by one register; at ka = 0 its M - k is bin 4096)
__device__ __forceinline__ void ols_split(const cx (&zp)[32], const cx (&zm)[32], int ka, const OlsLane &ln,
                                          cx2 tw, cx2 &X1, cx2 &X2) {
    const cx a0 = ka == 0 ? zp[0] : zm[32 - ka], b0 = zm[31 - ka];
    const cx a1 = zm[16 - ka], b1 = zm[15 - ka];
    const cx s0 = cx{ln.l0 ? a0.r : b0.r, ln.l0 ? a0.i : b0.i};
    const cx s1 = cx{ln.l0 ? a1.r : b1.r, ln.l0 ? a1.i : b1.i};
    const cx2 Pp = cx2{v2f{bperm(ln.src, s0.r), bperm(ln.src, s1.r)}, v2f{bperm(ln.src, s0.i), bperm(ln.src, s1.i)}};
    const cx2 Z = cx2{v2f{zp[ka].r, zp[ka + 16].r}, v2f{zp[ka].i, zp[ka + 16].i}};
    const cx2 E = cx2{Z.r + Pp.r, Z.i - Pp.i};
    const cx2 D = cx2{Z.r - Pp.r, Z.i + Pp.i};
    const cx2 T = cmul2(negi(D), tw);
    X1 = E + T;  // 2 X[k]
    X2 = E - T;  // conj 2 X[M - k]
}

// the split run backwards on the same lane pairs: from Y[k] and Y[M - k],
// Z'[k] = E + i O into zk and Z'[M - k] = conj E + i conj O sent back to its
// owner lane into zr, with E = Y[k] + conj Y[M-k], O = (Y[k] - conj Y[M-k]) W^-k.
// Lane 0's zr is off by one register until ols_unsplit_lane0.
__device__ __forceinline__ void ols_unsplit(cx2 Yk, cx2 YMk, cx2 tw, int ka, const OlsLane &ln, cx (&zk)[32],
                                            cx (&zr)[32]) {
    const cx2 E2 = cx2{Yk.r + YMk.r, Yk.i - YMk.i};                           // Y[k] + conj Y[M-k]
    const cx2 O2 = cmul2(cx2{Yk.r - YMk.r, Yk.i + YMk.i}, cx2{tw.r, -tw.i});  // (..) W^-k
    const cx2 Zk = cx2{E2.r - O2.i, E2.i + O2.r};                            // E + i O
    const cx2 ZMk = cx2{E2.r + O2.i, O2.r - E2.i};                           // conj E + i conj O
    zk[ka] = cx{Zk.r.x, Zk.i.x};
    zk[ka + 16] = cx{Zk.r.y, Zk.i.y};
    zr[31 - ka] = cx{bperm(ln.src, ZMk.r.x), bperm(ln.src, ZMk.i.x)};
    zr[15 - ka] = cx{bperm(ln.src, ZMk.r.y), bperm(ln.src, ZMk.i.y)};
}

// lane 0 received its own Z'[M - k] of ka = 31 - q at q; it needs the one of
// ka = 32 - q, i.e. what landed at q - 1, and at q = 0 the self-paired bin
// k = 2048: Z'[2048] = 2 conj Y, Y = 2 X[2048] H[2048]
__device__ __forceinline__ void ols_unsplit_lane0(cx Y, const OlsLane &ln, cx (&zr)[32]) {
#pragma unroll
    for (int q = 31; q >= 1; --q) zr[q] = cx{ln.l0 ? zr[q - 1].r : zr[q].r, ln.l0 ? zr[q - 1].i : zr[q].i};
    zr[0] = cx{ln.l0 ? 2.f * Y.r : zr[0].r, ln.l0 ? -2.f * Y.i : zr[0].i};
}

}  // namespace dspb
