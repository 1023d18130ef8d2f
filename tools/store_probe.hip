// tools/store_probe.hip -- HBM write-pattern probe for the headline kernel's
// stores, without its FFT.  Every "frame wave" writes what stft8192_pk_kernel
// writes for one frame: 4096 render floats (16 KB, contiguous) and one
// 4097-float magnitude row at mag + f * ld.  Variants change the store width,
// the row layout (ld), the magnitude lane order and a compute delay between
// the two bursts (s_sleep, standing in for the FFT), at the kernel's own
// occupancy (66.5 KB LDS per 4-wave block -> 2 waves per SIMD).
//
//
// `store_probe rows [passes]` is the store-only launch instead
// (stft_pk.hpp stft8192_rows_kernel: one-wave workgroups, the XCD remap, the
// cached row loaded from a 16 KB buffer, store_row_pieces' LDS staging at ld
// 4097, 32 non-temporal dwordx2 per hop) at its shape, 42,186 frames x 2
// channels, with the pacing knobs of profiles/r10_rows_pacing_probe.txt:
// resident waves per CU (an LDS pad), an s_sleep between the hop burst and the
// row burst, between the two halves of the row burst or as a stagger at wave
// start, and the order of the two bursts.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/store_probe.hip -o build/store_probe
//   ./build/store_probe            (prints one line per variant, GB/s of 8 TB/s)
//   ./build/store_probe rows 3     (the pacing sweep, three passes)
//   ./build/store_probe rows 3 fine   (3 to 6 waves, sleeps of 0 to 6 x 64 between the bursts)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#define CK(x)                                                                          \
    do {                                                                               \
        hipError_t e = (x);                                                            \
        if (e != hipSuccess) {                                                         \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));                    \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t xcd_remap(uint32_t bid, uint32_t nwg) {
    const uint32_t xcd = bid & 7u, q = nwg >> 3, r = nwg & 7u;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

struct Args {
    float *out[2];
    float *mag[2];
    uint64_t F;
    uint32_t ld;
    uint32_t delay;  // s_sleep 64 iterations (each ~64 x 64 cycles)
};

// RW: 2 = dwordx2 render stores (the kernel), 4 = dwordx4
// MAG: 0 = the kernel's dword pieces (forward + reversed), 1 = LDS-staged
//      16-byte pieces, 2 = dwordx4 straight (row must be 16 B aligned: ld % 4 == 0)
// NT: render stores non-temporal
template <int RW, int MAG, bool NT>
__global__ __launch_bounds__(256, 2) void probe(Args A) {
    __shared__ __attribute__((aligned(16))) float lds_all[4][64 * 65];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ch = blockIdx.y;
    const uint64_t f = (uint64_t)xcd_remap(blockIdx.x, gridDim.x) * 4u + wave;
    if (f >= A.F) return;
    float *lds = lds_all[wave];
    const float v = (float)lane * 0.25f + (float)f;
    float *o = A.out[ch] + f * 4096u;
    if constexpr (RW == 2) {
#pragma unroll
        for (int b = 0; b < 32; ++b) {
            v2f t = v2f{v + b, v - b};
            if constexpr (NT) __builtin_nontemporal_store(t, reinterpret_cast<v2f *>(o + 128u * b) + lane);
            else reinterpret_cast<v2f *>(o + 128u * b)[lane] = t;
        }
    } else {
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            v4f t = v4f{v + b, v - b, v * b, v + 2 * b};
            if constexpr (NT) __builtin_nontemporal_store(t, reinterpret_cast<v4f *>(o + 256u * b) + lane);
            else reinterpret_cast<v4f *>(o + 256u * b)[lane] = t;
        }
    }
    for (uint32_t i = 0; i < A.delay; ++i) __builtin_amdgcn_s_sleep(64);
    float *mrow = A.mag[ch] + f * A.ld;
    if constexpr (MAG == 0) {
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) {
            mrow[64u * kk + lane] = v + kk;
            mrow[4096u - 64u * kk - lane] = v - kk;
        }
        if (lane == 0) mrow[2048] = v;
    } else if constexpr (MAG == 1) {
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) {
            lds[64u * kk + lane] = v + kk;
            lds[4096u - 64u * kk - lane] = v - kk;
        }
        if (lane == 0) lds[2048] = v;
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float4 q = reinterpret_cast<const float4 *>(lds)[64 * i + lane];
            *reinterpret_cast<f4u *>(mrow + 256u * i + 4u * lane) = f4u{q.x, q.y, q.z, q.w};
        }
        if (lane == 0) mrow[4096] = lds[4096];
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            reinterpret_cast<float4 *>(mrow + 256u * i)[lane] = float4{v + i, v - i, v, v * i};
        if (lane == 0) mrow[4096] = v;
    }
}

// ---------------------------------------------------------------------------
// the store-only launch (stft8192_rows_kernel) and its pacing knobs
// ---------------------------------------------------------------------------
struct RowsArgs {
    float *out[2];
    float *mag[2];
    const float *row;  // 4100 floats
    uint64_t F;
    uint32_t ld;
    uint32_t mode;  // 0 none, 1 sleep between the bursts, 2 between the halves of the row burst, 3 stagger at wave start
    uint32_t n;     // s_sleep(64) count
    uint32_t k;     // mode 3: (wave index mod k) * n sleeps
};

__device__ __forceinline__ void nap(uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(64);
}

// store_row_pieces of stft_pk.hpp, with the mode 2 sleep after 8 of its 16 pieces
__device__ __forceinline__ void rows_pieces(const float (&M)[66], float *mrow, uint32_t lane, float *lds, uint32_t mid) {
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(mrow) >> 2) & 3u;
    float *sl = lds + a;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        (sl + lane)[64 * q] = M[4 * q];
        (sl + 2048u + lane)[64 * q] = M[4 * q + 1];
        (sl + 4096u - lane)[-64 * q] = M[4 * q + 2];
        (sl + 2048u - lane)[-64 * q] = M[4 * q + 3];
    }
    if (lane == 0) {
        sl[1024] = M[64];
        sl[3072] = M[65];
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    const uint32_t j0 = a ? 1u : 0u, j1 = (4093u + a) >> 2;
    float *gb = mrow - a;  // 16-byte aligned
    float4 p[16];
#pragma unroll
    for (int it = 0; it < 16; ++it) p[it] = reinterpret_cast<const float4 *>(lds)[j0 + 64u * (uint32_t)it + lane];
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        if (it == 8) nap(mid);
        const uint32_t j = j0 + 64u * (uint32_t)it + lane;
        if (it < 15 || j <= j1) *reinterpret_cast<v4f *>(gb + 4u * j) = v4f{p[it].x, p[it].y, p[it].z, p[it].w};
    }
    const uint32_t head = 4u * j0 - a, tail0 = 4u * j1 + 4u - a;
    if (lane < head) mrow[lane] = M[0];
    if (4096u - lane >= tail0) (mrow + 4096u - lane)[0] = M[2];
}

template <bool ROW_FIRST>
__global__ __launch_bounds__(64) void rows_probe(RowsArgs A) {
    __shared__ __attribute__((aligned(16))) float lds[64 * 65];
    const uint32_t lane = threadIdx.x;
    const uint32_t ch = blockIdx.y;
    const uint64_t f = xcd_remap(blockIdx.x, gridDim.x);
    if (f >= A.F) return;
    // (blockIdx.x >> 3: the order of the waves one XCD is given)
    if (A.mode == 3) nap(((blockIdx.x >> 3) % A.k) * A.n);
    const float v = (float)lane * 0.25f + (float)(f & 511u);
    const v2f st[4] = {v2f{v, v + 1.f}, v2f{v + 2.f, v + 3.f}, v2f{v + 4.f, v + 5.f}, v2f{v + 6.f, v + 7.f}};
    float *o = A.out[ch] + f * 4096u;
    auto hop = [&] {
#pragma unroll
        for (int b = 0; b < 32; ++b) __builtin_nontemporal_store(st[b % 4], reinterpret_cast<v2f *>(o + 128u * b) + lane);
    };
    auto rowburst = [&] {
        const float *row = A.row;
        float M[66];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            M[4 * q] = (row + lane)[64 * q];
            M[4 * q + 1] = (row + 2048u + lane)[64 * q];
            M[4 * q + 2] = (row + 4096u - lane)[-64 * q];
            M[4 * q + 3] = (row + 2048u - lane)[-64 * q];
        }
        M[64] = row[1024];
        M[65] = row[3072];
        rows_pieces(M, A.mag[ch] + f * A.ld, lane, lds, A.mode == 2 ? A.n : 0u);
    };
    if (ROW_FIRST) rowburst(); else hop();
    if (A.mode == 1) nap(A.n);
    if (ROW_FIRST) hop(); else rowburst();
}

__global__ void fill4(float4 *p, uint64_t n4) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * blockDim.x)
        p[i] = float4{1.f, 2.f, 3.f, 4.f};
}

template <typename K>
static float timeit(K launch, int reps = 20) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    for (int i = 0; i < 5; ++i) launch();
    std::vector<float> ts;
    for (int i = 0; i < reps; ++i) {
        CK(hipEventRecord(a));
        launch();
        CK(hipEventRecord(b));
        CK(hipEventSynchronize(b));
        float ms;
        CK(hipEventElapsedTime(&ms, a, b));
        ts.push_back(ms);
    }
    std::sort(ts.begin(), ts.end());
    return ts[ts.size() / 2];
}

// The sweep: every setting `passes` times, the unpaced launch (9 waves, no
// sleep, hop first) at the start, the middle and the end of every pass as the
// session's spread.
// fine: around the coarse sweep's best corner instead (few waves, hop first, a short sleep between the bursts)
static int rows_sweep(int passes, bool fine) {
    const uint64_t F = 42186, L = F * 4096u;
    const uint32_t ld = 4097;
    float *out, *row;
    CK(hipMalloc(&out, (2 * L + 2 * F * ld + 4) * 4));
    CK(hipMalloc(&row, 4100 * 4));
    {
        std::vector<float> h(4100);
        for (int i = 0; i < 4100; ++i) h[i] = 0.001f * (float)i;
        CK(hipMemcpy(row, h.data(), 4100 * 4, hipMemcpyHostToDevice));
    }
    RowsArgs A;
    A.out[0] = out; A.out[1] = out + L;
    A.mag[0] = out + 2 * L; A.mag[1] = A.mag[0] + F * ld;
    A.row = row; A.F = F; A.ld = ld;
    const double bytes = 2.0 * F * (4096 + 4097) * 4;
    const dim3 grid((uint32_t)F, 2);
    // static LDS 16,640 B of the 160 KB: the pad that leaves `waves` workgroups per CU
    auto pad_for = [](uint32_t waves) { return waves >= 9 ? 0u : (163840u / waves - 16640u) & ~255u; };
    auto run = [&](uint32_t waves, bool row_first, uint32_t mode, uint32_t n, uint32_t k) {
        A.mode = mode; A.n = n; A.k = k ? k : 1;
        const uint32_t pad = pad_for(waves);
        const float ms = timeit([&] {
            if (row_first) rows_probe<true><<<grid, 64, pad>>>(A);
            else rows_probe<false><<<grid, 64, pad>>>(A);
        }, 15);
        CK(hipGetLastError());
        printf("waves %2u order %s mode %u n %u k %u  %8.4f ms  %7.1f GB/s\n", waves, row_first ? "row-hop" : "hop-row", mode,
               n, k, ms, bytes / ms / 1e6);
        fflush(stdout);
    };
    for (int pass = 0; pass < passes; ++pass) {
        printf("-- pass %d\n", pass);
        run(9, false, 0, 0, 0);
        if (fine) {
            for (uint32_t waves : {6u, 5u, 4u, 3u})
                for (uint32_t n : {0u, 1u, 2u, 3u, 4u, 6u}) run(waves, false, n ? 1 : 0, n, 0);
            run(9, false, 0, 0, 0);
            continue;
        }
        for (uint32_t waves : {9u, 8u, 6u, 4u}) {
            if (waves == 6) run(9, false, 0, 0, 0);
            for (int rf = 0; rf < 2; ++rf) {
                if (waves != 9 || rf) run(waves, rf, 0, 0, 0);
                for (uint32_t mode : {1u, 2u})
                    for (uint32_t n : {1u, 2u, 4u, 8u}) run(waves, rf, mode, n, 0);
                for (uint32_t k : {2u, 4u})
                    for (uint32_t n : {1u, 2u, 4u, 8u}) run(waves, rf, 3, n, k);
            }
        }
        run(9, false, 0, 0, 0);
    }
    CK(hipDeviceSynchronize());
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "rows")) return rows_sweep(argc > 2 ? atoi(argv[2]) : 3, argc > 3 && !strcmp(argv[3], "fine"));
    const uint64_t F = 84372, L = F * 4096u;
    const uint32_t ldmax = 4224;
    // one allocation: the render rows, then the magnitude rows (the fill
    // probe below writes the same byte count from the start of it)
    const uint64_t total = 2 * L + 2 * F * (uint64_t)ldmax;  // floats
    float *out;
    CK(hipMalloc(&out, total * 4));
    float *mag = out + 2 * L;
    Args A;
    A.out[0] = out; A.out[1] = out + L;
    A.mag[0] = mag; A.mag[1] = mag + F * ldmax;
    A.F = F;
    const double bytes = 2.0 * F * (4096 + 4097) * 4;
    dim3 grid((uint32_t)((F + 3) / 4), 2);
    auto line = [&](const char *name, float ms) {
        printf("%-44s %8.4f ms  %7.1f GB/s  %5.1f%%\n", name, ms, bytes / ms / 1e6, bytes / ms / 1e6 / 80.0);
        fflush(stdout);
    };
    {
        const uint64_t n4 = (uint64_t)(bytes / 16);
        if (n4 * 4 > total) { fprintf(stderr, "fill exceeds the buffer\n"); return 1; }
        line("fill float4 grid-stride (same bytes)", timeit([&] { fill4<<<4096, 256>>>((float4 *)out, n4); }));
    }
    struct V { const char *name; int rw, mag; bool nt; uint32_t ld; };
    const V vs[] = {
        {"kernel: x2 NT render, dword mag, ld 4097", 2, 0, true, 4097},
        {"x2 cached render, dword mag, ld 4097", 2, 0, false, 4097},
        {"x4 NT render, dword mag, ld 4097", 4, 0, true, 4097},
        {"x4 cached render, dword mag, ld 4097", 4, 0, false, 4097},
        {"x2 NT render, LDS x4 mag, ld 4097", 2, 1, true, 4097},
        {"x4 NT render, LDS x4 mag, ld 4097", 4, 1, true, 4097},
        {"x2 NT render, dword mag, ld 4100", 2, 0, true, 4100},
        {"x4 NT render, x4 mag, ld 4100", 4, 2, true, 4100},
        {"x4 NT render, x4 mag, ld 4128", 4, 2, true, 4128},
        {"x4 cached render, x4 mag, ld 4128", 4, 2, false, 4128},
        {"x2 NT render, dword mag, ld 4128", 2, 0, true, 4128},
    };
    for (uint32_t delay : {0u, 4u}) {
        A.delay = delay;
        printf("-- compute delay %u x s_sleep(64)\n", delay);
        for (const V &v : vs) {
            A.ld = v.ld;
            float ms = 0;
#define P(rw, m, nt) ms = timeit([&] { probe<rw, m, nt><<<grid, 256>>>(A); })
            if (v.rw == 2 && v.mag == 0 && v.nt) P(2, 0, true);
            else if (v.rw == 2 && v.mag == 0) P(2, 0, false);
            else if (v.rw == 4 && v.mag == 0 && v.nt) P(4, 0, true);
            else if (v.rw == 4 && v.mag == 0) P(4, 0, false);
            else if (v.rw == 2 && v.mag == 1) P(2, 1, true);
            else if (v.rw == 4 && v.mag == 1) P(4, 1, true);
            else if (v.rw == 4 && v.mag == 2 && v.nt) P(4, 2, true);
            else P(4, 2, false);
#undef P
            CK(hipGetLastError());
            line(v.name, ms);
        }
    }
    CK(hipDeviceSynchronize());
    return 0;
}
