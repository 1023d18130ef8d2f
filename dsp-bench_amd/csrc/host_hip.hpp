// host_hip.hpp -- host-side idioms shared by the C ABI (capi.cpp) and the
// plugin module host (module*.cpp): the device guard, the capture predicate
// and the row-overlap test.
#pragma once
#include "common.hpp"

namespace dspb {

// RAII: make a device current for the call (a negative index: stay), restore
// the caller's afterwards -- on every return.
struct DeviceGuard {
    int prev = -1;
    int dev = -1;
    int status = DSP_OK;
    explicit DeviceGuard(int device) {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) { status = hip_fail(e, "hipGetDevice"); return; }
        dev = prev;
        if (device >= 0 && device != prev) {
            e = hipSetDevice(device);
            if (e != hipSuccess) { status = hip_fail(e, "hipSetDevice"); return; }
            dev = device;
        }
    }
    explicit DeviceGuard(const dsp_exec *ex) : DeviceGuard(ex ? ex->device : -1) {}
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
    ~DeviceGuard() {
        if (prev >= 0 && dev != prev) (void)hipSetDevice(prev);
    }
};

// the stream is being captured into a graph
inline bool capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// whether any input row [in[c], in[c] + L) overlaps any output row [out[c'], out[c'] + Lr)
inline bool rows_overlap(const float *const *in, uint32_t in_ch, uint64_t L, const float *const *out, uint32_t C,
                         uint64_t Lr) {
    for (uint32_t a = 0; a < in_ch; ++a)
        for (uint32_t b = 0; b < C; ++b) {
            const uintptr_t i0 = reinterpret_cast<uintptr_t>(in[a]), o0 = reinterpret_cast<uintptr_t>(out[b]);
            if (L && Lr && i0 < o0 + 4 * Lr && o0 < i0 + 4 * L) return true;
        }
    return false;
}

}  // namespace dspb
