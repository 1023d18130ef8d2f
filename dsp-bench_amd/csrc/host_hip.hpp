// host_hip.hpp -- host-side idioms shared by the C ABI (capi.cpp,
// capi_render.cpp, capi_rate.cpp, capi_bigfft.cpp, capi_grid.cpp) and the
// plugin module host (module*.cpp): the device guard, the capture predicate,
// the row-overlap predicates and a row call's layout rule.
#pragma once
#include "common.hpp"

#include <initializer_list>

#pragma GCC visibility push(hidden)
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

// `count` rows of `floats` floats each: [rows[c], rows[c] + floats).  A set of
// empty rows overlaps nothing, and its table is not looked at.
struct Rows {
    const float *const *rows;
    uint32_t count;
    uint64_t floats;
};

inline bool row_pair_overlaps(const float *p, uint64_t np, const float *q, uint64_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + 4 * nq && b < a + 4 * np;
}

// whether any row of a overlaps any row of b; with `same_ok`, a[c] == b[c]
// (channel c in place) does not count
inline bool rows_overlap(const Rows &a, const Rows &b, bool same_ok = false) {
    if (!a.floats || !b.floats) return false;
    for (uint32_t i = 0; i < a.count; ++i)
        for (uint32_t j = 0; j < b.count; ++j) {
            if (same_ok && i == j && a.rows[i] == b.rows[j]) continue;
            if (row_pair_overlaps(a.rows[i], a.floats, b.rows[j], b.floats)) return true;
        }
    return false;
}

// whether any two rows of a overlap each other
inline bool rows_overlap_each_other(const Rows &a) {
    if (!a.floats) return false;
    for (uint32_t i = 0; i < a.count; ++i)
        for (uint32_t j = i + 1; j < a.count; ++j)
            if (row_pair_overlaps(a.rows[i], a.floats, a.rows[j], a.floats)) return true;
    return false;
}

// The layout rule of a row call, asked once per call: whether a row of an
// output set overlaps a row of an input set, of another output set or of its
// own set (input sets may share memory: they are only read).  Its exceptions:
enum : uint32_t {
    kInPlaceOk = 1,        // outs[0][c] == ins[0][c] (channel c in place) does not count
    kOutputsUnchecked = 2  // the output sets are checked against the input sets only
};
inline bool output_rows_overlap(std::initializer_list<Rows> ins, std::initializer_list<Rows> outs, uint32_t except = 0) {
    for (const Rows *o = outs.begin(); o != outs.end(); ++o) {
        for (const Rows *i = ins.begin(); i != ins.end(); ++i)
            if (rows_overlap(*i, *o, (except & kInPlaceOk) && i == ins.begin() && o == outs.begin())) return true;
        if (except & kOutputsUnchecked) continue;
        for (const Rows *p = outs.begin(); p != o; ++p)
            if (rows_overlap(*p, *o)) return true;
        if (rows_overlap_each_other(*o)) return true;
    }
    return false;
}

}  // namespace dspb
#pragma GCC visibility pop
