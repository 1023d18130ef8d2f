// What dspbench_render holds on the device, each thing owned by an object: a
// return from any depth, an error among them, releases it.  (The RCCL
// communicator is not owned this way: destroying one is a collective, and it
// happens on the success paths only.)
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <utility>
#include <vector>

#include "dspbench/dspbench.h"
#include "dspbench/module.h"

inline int fail(const char *what, int st) {
    std::fprintf(stderr, "dspbench_render: %s: %s (%s)\n", what, dsp_status_string(st), dsp_last_error());
    return 1;
}

#define HIPCK(x)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            std::fprintf(stderr, "dspbench_render: %s: %s\n", #x, hipGetErrorString(e_)); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

// a handle and what destroys it; move-only
template <class T, auto Destroy> struct Owned {
    T h{};
    Owned() = default;
    Owned(Owned &&o) noexcept : h(o.h) { o.h = T{}; }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) reset(o.h), o.h = T{};
        return *this;
    }
    ~Owned() { reset(T{}); }
    void reset(T to) {
        if (h) (void)Destroy(h);
        h = to;
    }
};
using DevBuf = Owned<void *, hipFree>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Module = Owned<dsp_module *, dsp_module_destroy>;

// C rows of n floats; ptr is the table the ABI takes.  n is taken as given: rows
// of no floats are null (hipMalloc of 0 bytes), and the ABI refuses them
struct Rows {
    std::vector<DevBuf> own;
    std::vector<float *> ptr;
    hipError_t alloc(uint32_t C, uint64_t n) {
        own.resize(C), ptr.resize(C);
        for (uint32_t c = 0; c < C; ++c) {
            if (hipError_t e = hipMalloc(&own[c].h, n * sizeof(float))) return e;
            ptr[c] = (float *)own[c].h;
        }
        return hipSuccess;
    }
    void replace(uint32_t c, DevBuf &&with) { own[c] = std::move(with), ptr[c] = (float *)own[c].h; }
};

// the device, its stream and the clock of "end to end": all from the first open()
struct Device {
    const int device;
    Stream stream;
    dsp_exec ex{};
    std::chrono::steady_clock::time_point t0;
    explicit Device(int ordinal) : device(ordinal) {}
    int open() {
        if (stream.h) return 0;
        HIPCK(hipSetDevice(device));
        HIPCK(hipStreamCreate(&stream.h));
        ex.device = device, ex.stream = stream.h;
        t0 = std::chrono::steady_clock::now();
        return 0;
    }
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
