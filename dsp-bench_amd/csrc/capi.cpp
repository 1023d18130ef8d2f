// capi.cpp -- the extern "C" boundary of libdspbench (include/dspbench/dspbench.h).
//
// Validates arguments, owns the per-device constant tables (twiddles,
// windows: the analogue of the IPP FFT spec / plan cache of dsp.cpp:84-95 and
// IPP_FFT_Context, structs.h:170-178), maps a dsp_plugin onto a kernel and
// launches on the caller's stream.  Fails loudly (negative status) on
// anything it cannot run on the GPU -- there is no CPU path here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "host_hip.hpp"
#include "host_tables.hpp"
#include "kernels.hpp"
#include "limiter_host.hpp"
#include "loudness_host.hpp"
#include "sweep_host.hpp"
#include "dspbench/wav.h"

namespace dspb {

static thread_local char g_last_error[512] = "";

void set_last_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof g_last_error, fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char *what) {
    set_last_error("%s: %s", what, hipGetErrorString(e));
    if (e == hipErrorOutOfMemory) return DSP_ERR_NOMEM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return DSP_ERR_NO_DEVICE;
    return DSP_ERR_HIP;
}

static int invalid(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof g_last_error, fmt, ap);
    va_end(ap);
    return DSP_ERR_INVALID;
}

// ---------------------------------------------------------------------------
// per-device resources
// ---------------------------------------------------------------------------
// A cached device table (FIR taps and spectra, BIQUAD transition powers):
// each call that maps it holds it until its launches are enqueued; the table
// is freed when the cache has evicted it and no call holds it, after the
// device has finished the work already enqueued
typedef std::shared_ptr<float> DevTable;
static DevTable dev_table(float *p, int dev) {
    return DevTable(p, [dev](float *q) {
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(dev);
        (void)hipDeviceSynchronize();
        (void)hipFree(q);
        if (prev >= 0) (void)hipSetDevice(prev);
    });
}


// One entry of a keyed cache of device tables (cached_table): a FIR filter's
// taps + overlap-save spectra, keyed by the taps, or a biquad cascade's
// coefficients + state-transition powers (biquad_tables), keyed by the
// coefficients
struct CachedTable {
    std::vector<float> key;
    DevTable dev;
    float h2048r = 0.f, h2048i = 0.f;  // FIR: H[2048] of the 8192-point spectrum
    uint32_t window = 0;               // BIQUAD: biquad_tables' W
    size_t bytes = 0;                  // of the device table
};
typedef std::vector<CachedTable> TableCache;  // oldest first

// the look-back workspace of biquad_scan_kernel, one per (device, stream):
// calls on one stream run in order, so a launch only meets words tagged with
// its own epoch (zeroed at allocation; epochs run 1 .. 2^32 - 1)
struct IirWork {
    uint64_t *aggw = nullptr, *inclw = nullptr;  // cap * 16 words each, one allocation, then the error word
    uint64_t cap = 0;
    uint64_t epoch = 0;
};

struct DeviceRes {
    v2f *tw8192 = nullptr;  // exp(-2 pi i k / 8192), then 896 lane-major stage twiddles
    float4 *wbase = nullptr;  // (cos, sin)(theta 2l), (cos, sin)(theta (2l+1)), theta = 2 pi / 8191
    std::map<std::tuple<int, uint32_t, uint32_t, float>, float *> windows;  // (kind, N, valid, scale)
    std::map<std::pair<void *, int>, std::pair<float *, size_t>> scratch;  // per (stream, slot)
    TableCache fir;                                            // FIR filters seen (plugin_map)
    TableCache iir;                                            // biquad cascades seen (plugin_map)
    TableCache conv;                                           // CONV impulse responses seen (plugin_map)
    TableCache resample;                                       // dsp_resample conversions seen (up, down, spec)
    TableCache limiter;                                        // dsp_limiter tables seen (rho, lookahead)
    TableCache rfft;                                           // dsp_rfft twiddle tables seen (n)
    std::map<void *, IirWork> iir_work;                        // per stream
    uint32_t *iir_fb_host = nullptr, *iir_fb_dev = nullptr;  // host-mapped counter of repaired launches
    float *delta = nullptr;  // 2048 floats: 1, 0, 0, ... (compute_IR's impulse, read-only)
};

static std::mutex g_mu;
// (never destroyed: its tables must not be freed after the HIP runtime's own
// teardown at process exit)
static std::map<int, DeviceRes> &g_res = *new std::map<int, DeviceRes>;

static int current_device(int *dev) {
    DSPB_HIP(hipGetDevice(dev));
    return DSP_OK;
}

// A call on a stream that is being captured into a graph cannot make a
// first-use table or scratch allocation (an allocation, a legacy-stream
// launch and a sync would invalidate the capture): it is refused instead, and
// one eager call of the same shape beforehand creates what it needs.
static int refuse_capture(hipStream_t s, const char *what) {
    if (capturing(s)) {
        set_last_error("stream capture: %s is created on first use; make one eager call of this shape on the "
                       "capturing stream first", what);
        return DSP_ERR_INVALID;
    }
    return DSP_OK;
}

// Synchronous upload of a constant table (launch_upload: kernel arguments,
// not a copy -- see render.hip); the tables are shared by every stream of the
// device, so the upload completes before the first use.  (Callers check the
// caller's stream for capture first: refuse_capture.)
static int upload_table(void *dst, const void *src, size_t bytes) {
    if (int st = launch_upload((float *)dst, (const float *)src, bytes / sizeof(float), nullptr)) return st;
    DSPB_HIP(hipStreamSynchronize(nullptr));
    return DSP_OK;
}

// A constant device table made on first use, with g_mu held: `slot` if it is
// set already; else the host values from build(), uploaded to a fresh
// allocation.  `what` names the table in the capture refusal.
template <class T, class Build>
static int first_use_table(T *&slot, hipStream_t s, const char *what, Build build) {
    if (slot) return DSP_OK;
    if (int st = refuse_capture(s, what)) return st;
    const std::vector<T> h = build();
    T *d = nullptr;
    DSPB_HIP(hipMalloc(&d, sizeof(T) * h.size()));
    if (int st = upload_table(d, h.data(), sizeof(T) * h.size())) {
        (void)hipFree(d);
        return st;
    }
    slot = d;
    return DSP_OK;
}

static std::vector<v2f> twiddle_table() {
    std::vector<v2f> h(8192);
    for (int k = 0; k < 8192; ++k) {
        const double a = -2.0 * M_PI * (double)k / 8192.0;
        h[k] = v2f{(float)std::cos(a), (float)std::sin(a)};
    }
    // exact zeros / ones at the quarter turns
    h[0] = v2f{1.f, 0.f}; h[2048] = v2f{0.f, -1.f};
    h[4096] = v2f{-1.f, 0.f}; h[6144] = v2f{0.f, 1.f};
    // lane-major stage twiddles of the 64 x 64 step (stft_pk.hpp, fft_pk.hpp):
    // [8192 + 64 (j-1) + l] = T[2 l j], [8192 + 448 + 64 (j-1) + l] = T[16 l j]
    for (int j = 1; j < 8; ++j)
        for (int l = 0; l < 64; ++l) h.push_back(h[(2 * l * j) & 8191]);
    for (int j = 1; j < 8; ++j)
        for (int l = 0; l < 64; ++l) h.push_back(h[(16 * l * j) & 8191]);
    // stft_pk.hip pairs, one float4 per (hi, lane), hi < 4:
    // (re T[16 l hi], re T[16 l (hi + 4)], im T[16 l hi], im T[16 l (hi + 4)])
    for (int hi = 0; hi < 4; ++hi)
        for (int l = 0; l < 64; ++l) {
            const v2f a = h[(16 * l * hi) & 8191], b = h[(16 * l * (hi + 4)) & 8191];
            h.push_back(v2f{a.x, b.x});
            h.push_back(v2f{a.y, b.y});
        }
    return h;
}

static int get_tw(int dev, hipStream_t s, const v2f **out) {
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceRes &r = g_res[dev];
    if (int st = first_use_table(r.tw8192, s, "the FFT twiddle table", twiddle_table)) return st;
    *out = r.tw8192;
    return DSP_OK;
}

// compute_IR's impulse (plugin.cpp:27-34) as a read-only device buffer: the
// IR render of a map plugin reads it as its file, so no impulse launch
constexpr uint32_t kDeltaLen = 2048;  // the largest ir_len (4 ir_len <= 8192)
static int get_delta(int dev, hipStream_t s, const float **out) {
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceRes &r = g_res[dev];
    const int st = first_use_table(r.delta, s, "the impulse buffer", [] {
        std::vector<float> h(kDeltaLen, 0.0f);
        h[0] = 1.0f;
        return h;
    });
    *out = r.delta;
    return st;
}

// the cosine windows w[n] = a - b cos(2 pi n / (valid - 1))
static void window_coefficients(int kind, double *a, double *b) {
    *a = 0.54, *b = 0.46;
    if (kind == DSP_WIN_HANN) *a = 0.5, *b = 0.5;
    else if (kind == DSP_WIN_RECT) *a = 1.0, *b = 0.0;
}

// Window of length `valid` (symmetric, ref ippsWinHamming_32f convention)
// zero-padded to N.  Computed in double, rounded once to float.
static int get_window(int dev, hipStream_t s, int kind, uint32_t N, uint32_t valid, const float **out,
                      double scale = 1.0) {
    std::lock_guard<std::mutex> lk(g_mu);
    float *&slot = g_res[dev].windows[std::make_tuple(kind, N, valid, (float)scale)];
    const int st = first_use_table(slot, s, "a window table", [&] {
        double a, b;
        window_coefficients(kind, &a, &b);
        std::vector<float> h(N, 0.f);
        for (uint32_t n = 0; n < valid; ++n)
            h[n] = valid == 1 ? (float)scale
                              : (float)(scale * (a - b * std::cos(2.0 * M_PI * (double)n / (double)(valid - 1))));
        return h;
    });
    *out = slot;
    return st;
}

// stft8192_pk_kernel folds DIV_BY_SQRTN and the 1/2 of the real split into
// the window: 0.5 / sqrt(N)
static float window_prescale(uint32_t N) { return (float)(0.5 / std::sqrt((double)N)); }
// DIV_BY_SQRTN (dsp.cpp:74-132): every transform scales by 1 / sqrt(n)
static float fft_scale(uint32_t n) { return (float)(1.0 / std::sqrt((double)n)); }

// Inputs of the computed-window kernels (stft_pk.hpp kOptWinComp): per-lane
// base angles and the (pre-scaled) cosine-window coefficients.
static int set_wincomp(int dev, hipStream_t s, int kind, Stft8kArgs *A) {
    {
        std::lock_guard<std::mutex> lk(g_mu);
        DeviceRes &r = g_res[dev];
        const int st = first_use_table(r.wbase, s, "the window base angles", [] {
            std::vector<float4> h(64);
            const double th = 2.0 * M_PI / 8191.0;
            for (int l = 0; l < 64; ++l)
                h[l] = float4{(float)std::cos(th * 2 * l), (float)std::sin(th * 2 * l),
                              (float)std::cos(th * (2 * l + 1)), (float)std::sin(th * (2 * l + 1))};
            return h;
        });
        if (st) return st;
        A->wbase = r.wbase;
    }
    double a, b;
    window_coefficients(kind, &a, &b);
    const double sc = window_prescale(8192);
    A->wa = (float)(a * sc);
    A->wb = (float)(b * sc);
    return DSP_OK;
}

// Stream-ordered scratch: calls on one stream are serialised by the stream,
// so one buffer per (device, stream, slot) is enough.  Slots: 0 the IR_test
// block table, 1 loop mode's wrapped file, 2 a CONV channel group's spectra,
// 3 a dsp_loudness channel group's partial sums, hop energies and peaks,
// 4 a dsp_limiter call's hold rows, tile aggregates, carries and result words,
// 5 a dsp_rfft / dsp_irfft / dsp_deconvolve channel group's work buffers and spectra.
static int get_scratch(int dev, hipStream_t s, size_t bytes, float **out, int slot_id = 0) {
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceRes &r = g_res[dev];
    auto &slot = r.scratch[std::make_pair((void *)s, slot_id)];
    if (slot.second < bytes) {
        // a stream being captured into a graph cannot allocate or wait: its
        // scratch must exist from an eager call of the same shape first
        if (int st = refuse_capture(s, "the stream's scratch buffer")) return st;
        if (slot.first) {
            DSPB_HIP(hipStreamSynchronize(s));
            DSPB_HIP(hipFree(slot.first));
        }
        slot.first = nullptr;
        slot.second = 0;
        DSPB_HIP(hipMalloc(&slot.first, bytes));
        slot.second = bytes;
    }
    *out = slot.first;
    return DSP_OK;
}

// ---------------------------------------------------------------------------
// optional per-launch timing of the dominant kernel (HIP events on the
// launch stream), read back by dsp_kernel_timing(); used by bench.py
// ---------------------------------------------------------------------------
struct TimedLaunch {
    hipEvent_t start, stop;
    uint64_t bytes;
    int dev;
};
static bool g_timing = false;
// recycled timing events per device (g_mu): a hipEventCreate pair per timed
// launch cost more than the records themselves
static std::map<int, std::vector<hipEvent_t>> g_event_pool;

// A/B and ablation options of stft8192_pk_kernel: 0 in the product library
// (the tools build's stft_pk_ab.hip sets them per thread)
static int pk_options() { return stft_pk_ab_options(); }

// a closed-form IR ramp (plugin_map) leaves the block table unbuilt; every
// fused path but stft_pk's PER path reads it
static int ensure_ramp_table(const SampleMap &m, hipStream_t s) {
    if (m.kind != MapKind::Ramp || m.closed != 1) return DSP_OK;  // 2: the table holds it already
    return launch_ramp_table(const_cast<float *>(m.table), m.B, (float)m.rg0, (float)m.rs, s);
}

// DSP_DEBUG_FRAME_RUN: frames per wave of the fused IR_test launch's frame
// reuse (0: the launch's own choice, stft8192_pk_frame_run)
static std::atomic<uint32_t> g_frame_run{0};

static int launch_stft(const Stft8kArgs &A, uint32_t C, bool fused, hipStream_t s) {
    if (fused && !(A.map.closed && stft8192_pk_per_path(A, fused))) {
        const int st = ensure_ramp_table(A.map, s);
        if (st) return st;
    }
    return launch_stft8192_pk(A, C, fused, pk_options(), s);
}

static std::vector<TimedLaunch> g_timed;

// set while a call times its launches as one region (the pipelined GENERIC
// render + STFT): the launches inside record nothing of their own
static thread_local bool tl_timing_outer = false;

static int timing_begin(hipStream_t s, TimedLaunch *t) {
    t->start = t->stop = nullptr;
    if (!g_timing || tl_timing_outer) return DSP_OK;
    DSPB_HIP(hipGetDevice(&t->dev));
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto &pool = g_event_pool[t->dev];
        if (pool.size() >= 2) {
            t->start = pool.back();
            pool.pop_back();
            t->stop = pool.back();
            pool.pop_back();
        }
    }
    if (!t->start) {
        DSPB_HIP(hipEventCreate(&t->start));
        DSPB_HIP(hipEventCreate(&t->stop));
    }
    DSPB_HIP(hipEventRecord(t->start, s));
    return DSP_OK;
}

static int timing_end(hipStream_t s, TimedLaunch *t, uint64_t bytes) {
    if (!t->start) return DSP_OK;
    DSPB_HIP(hipEventRecord(t->stop, s));
    t->bytes = bytes;
    std::lock_guard<std::mutex> lk(g_mu);
    g_timed.push_back(*t);
    return DSP_OK;
}

static bool is_pow2(uint64_t n) { return n && !(n & (n - 1)); }
static uint32_t ilog2(uint64_t n) { uint32_t l = 0; while ((1ull << l) < n) ++l; return l; }
static bool aligned(const void *p, size_t a) { return ((uintptr_t)p % a) == 0; }

// ---------------------------------------------------------------------------
// plugin -> sample map
// ---------------------------------------------------------------------------
// sleeps a BIQUAD look-back waits for a predecessor's words before it gives
// up (a legitimate wait is a few rounds: a tile waits only for waves
// dispatched before it); the launch is then rendered again serially
// (iir.hip biquad_repair_kernel, on the same stream)
constexpr uint32_t kIirSpinLimit = 1u << 16;
static std::atomic<uint32_t> g_iir_spin_limit{kIirSpinLimit};

// takes the stream's workspace for one launch (a fresh epoch) and launches,
// under one lock: launches on a stream are enqueued in epoch order
static int iir_launch(int dev, hipStream_t s, BiquadArgs *A, uint32_t sections, uint32_t nch) {
    const uint64_t tiles = (uint64_t)(A->C / nch) * A->ntiles_ch;
    if (capturing(s)) {  // every launch takes a fresh epoch: a graph replay would reuse it
        set_last_error("stream capture: a BIQUAD render cannot be captured (its look-back state is per launch)");
        return DSP_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceRes &r = g_res[dev];
    if (!r.iir_fb_host) {
        if (int st = refuse_capture(s, "the BIQUAD repair counter")) return st;
        void *p = nullptr;
        DSPB_HIP(hipHostMalloc(&p, 64, hipHostMallocMapped));
        r.iir_fb_host = (uint32_t *)p;
        *r.iir_fb_host = 0;
        void *d = nullptr;
        DSPB_HIP(hipHostGetDevicePointer(&d, p, 0));
        r.iir_fb_dev = (uint32_t *)d;
    }
    IirWork &w = r.iir_work[(void *)s];
    if (w.cap < tiles) {
        if (int st = refuse_capture(s, "the BIQUAD look-back workspace")) return st;
        if (w.aggw) {
            DSPB_HIP(hipStreamSynchronize(s));
            DSPB_HIP(hipFree(w.aggw));
            w = IirWork{};
        }
        const uint64_t cap = std::max<uint64_t>(tiles, 1024);
        const size_t bytes = (2 * cap * 16 + 1) * sizeof(uint64_t);  // 16 words: a channel pair's 2 x 8
        void *p = nullptr;
        DSPB_HIP(hipMalloc(&p, bytes));
        DSPB_HIP(hipMemsetAsync(p, 0, bytes, s));
        w.aggw = (uint64_t *)p;
        w.inclw = w.aggw + cap * 16;
        w.cap = cap;
    }
    A->aggw = w.aggw;
    A->inclw = w.inclw;
    A->err = (uint32_t *)(w.inclw + w.cap * 16);
    A->repairs = r.iir_fb_dev;
    A->spin_limit = g_iir_spin_limit.load(std::memory_order_relaxed);
    w.epoch = w.epoch % 0xffffffffull + 1;
    A->epoch = w.epoch;
    if (int st = launch_biquad(*A, sections, nch, s)) return st;
    return DSP_OK;
}

// device bytes of CONV tables a device keeps cached beside the newest one (a
// 2^20-tap table is 8.25 MiB)
constexpr size_t kConvCacheBytes = 64u << 20;

// The entry of `key` in a cache of at most 8 device tables -- and, with
// max_bytes set, of at most that many bytes of them beside the newest, the
// oldest leaving first -- with g_mu held.
// On a miss build(h, entry) fills the host table and the entry's payload; the
// table is uploaded once per key, not once per render.  The caller copies
// what it needs out of *out (the DevTable as its hold) before it unlocks.
template <class Build>
static int cached_table(TableCache &cache, const std::vector<float> &key, int dev, hipStream_t s, const char *what,
                        Build build, const CachedTable **out, size_t max_bytes = 0) {
    for (auto &e : cache)
        if (e.key == key) { *out = &e; return DSP_OK; }
    CachedTable e;
    e.key = key;
    float *d = nullptr;
    const int st = first_use_table(d, s, what, [&] {
        std::vector<float> h;
        build(h, e);
        e.bytes = h.size() * sizeof(float);
        return h;
    });
    if (st) return st;
    e.dev = dev_table(d, dev);
    // the one eviction: the oldest entry leaves, and its table is freed here
    // unless a call still holds it -- dev_table's deleter waits for the device
    // with g_mu held (ADVICE.md's open finding)
    if (cache.size() >= 8) cache.erase(cache.begin());
    if (max_bytes) {
        size_t held = e.bytes;
        for (auto &c : cache) held += c.bytes;
        while (!cache.empty() && held > max_bytes) {
            held -= cache.front().bytes;
            cache.erase(cache.begin());
        }
    }
    cache.push_back(std::move(e));
    *out = &cache.back();
    return DSP_OK;
}

// *table: a hold on the call's cached device table (FIR / BIQUAD), kept by
// the caller until the call's launches are enqueued
static int plugin_map(const dsp_plugin *p, uint32_t B, int dev, hipStream_t s, SampleMap *m, float sr,
                      uint32_t flags, DevTable *table) {
    m->kind = MapKind::Noop;
    m->fir_direct = (flags & DSP_EXEC_FIR_DIRECT) ? 1u : 0u;
    m->a = 1.f;
    m->table = nullptr;
    m->B = B;
    m->b_mask = is_pow2(B) ? B - 1 : 0;
    m->taps = nullptr;
    m->ntaps8 = 0;
    m->convH = nullptr;
    m->conv_parts = 0;
    m->iir_tab = nullptr;
    m->sections = 0;
    m->iir_window = 0;
    m->module = nullptr;
    m->gparams = nullptr;
    m->gparams_size = 0;
    m->sr = sr;
    m->closed = 0;
    m->rg0 = m->rs = 0.0;
    if (!p) return DSP_OK;  // no plugin loaded: the file plays through (audio.cpp:144)
    float v0 = 0.f, v1 = 0.f;
    switch (p->kind) {
    case DSP_PLUGIN_NOOP:
        return DSP_OK;
    case DSP_PLUGIN_GAIN:  // build/gain_test.cpp: Parameters{float gain}
        if (!p->params || p->params_size < 4) return invalid("GAIN plugin needs a 4-byte params blob");
        std::memcpy(&v0, p->params, 4);
        m->kind = MapKind::Gain;
        m->a = v0;
        return DSP_OK;
    case DSP_PLUGIN_STATIC_GAIN:  // test/static_gain_plugin.cpp: State{float gain}
        if (!p->state || p->state_size < 4) return invalid("STATIC_GAIN plugin needs a 4-byte state blob");
        std::memcpy(&v0, p->state, 4);
        m->kind = MapKind::Gain;
        m->a = v0;
        return DSP_OK;
    case DSP_PLUGIN_IR_RAMP: {  // build/IR_test.cpp: Parameters{float gain; float step}
        if (!p->params || p->params_size < 8) return invalid("IR_RAMP plugin needs an 8-byte params blob");
        std::memcpy(&v0, p->params, 4);
        std::memcpy(&v1, (const char *)p->params + 4, 4);
        float *table = nullptr;
        int st = get_scratch(dev, s, sizeof(float) * B, &table);
        if (st) return st;
        m->kind = MapKind::Ramp;
        m->table = table;
        m->rg0 = (double)v0;
        m->rs = (double)v1;
        m->closed = ramp_closed_form(v0, v1, B) ? 1u : 0u;
        // closed form: the table is built only by ensure_ramp_table, for the
        // kernels that read it
        if (!m->closed) return launch_ramp_table(table, B, v0, v1, s);
        return DSP_OK;
    }
    case DSP_PLUGIN_FIR: {  // build-defined cfg 3b: Parameters{float taps[T]}
        const uint32_t T = p->params_size / 4;
        if (!p->params || T == 0 || p->params_size % 4 || T > 2048)
            return invalid("FIR plugin needs 1..2048 float taps as its params blob");
        const uint32_t T8 = (T + 15) & ~15u;  // zero-padded to 16 (fir.hip)
        // device copy: [taps, T8 floats][overlap-save H table, 8192 + 2 floats],
        // cached per device by the taps' bytes (the host FFT and the upload
        // happen once per filter, not once per render)
        std::vector<float> key((const float *)p->params, (const float *)p->params + T);
        float h2048[2] = {0.f, 0.f};
        {
            std::lock_guard<std::mutex> lk(g_mu);
            const CachedTable *ft = nullptr;
            const int st = cached_table(g_res[dev].fir, key, dev, s, "a FIR filter's device taps",
                                        [&](std::vector<float> &h, CachedTable &e) {
                // [taps, T8][8192-point table, 8194 (+ 2 pad)][4096-point pair table, 8192]
                h.assign(T8 + 8196 + 8192, 0.f);
                std::memcpy(h.data(), key.data(), 4 * (size_t)T);
                if (T <= 1025) {
                    ols_table(h.data(), T, h.data() + T8);
                    pair_table(h.data(), T, h.data() + T8 + 8196);
                }
                e.h2048r = h[T8 + 8192];
                e.h2048i = h[T8 + 8193];
            }, &ft);
            if (st) return st;
            *table = ft->dev;  // held by the call (copied under the lock)
            h2048[0] = ft->h2048r;
            h2048[1] = ft->h2048i;
        }
        float *tp = table->get();
        m->kind = MapKind::Fir;
        m->taps = tp;
        m->ntaps8 = T8;
        m->ntaps = T;
        m->olsH = tp + T8;
        m->pairH = tp + T8 + 8196;  // 16-byte aligned: T8 and 8196 are multiples of 4
        m->olsH2048[0] = h2048[0];
        m->olsH2048[1] = h2048[1];
        return DSP_OK;
    }
    case DSP_PLUGIN_CONV: {  // build-defined: Parameters{float taps[T]}, a long impulse response
        const uint32_t T = p->params_size / 4;
        if (!p->params || T == 0 || p->params_size % 4 || T > kConvMaxTaps)
            return invalid("CONV plugin needs 1..%u float taps as its params blob", kConvMaxTaps);
        std::vector<float> key((const float *)p->params, (const float *)p->params + T);
        for (float v : key)
            if (!std::isfinite(v)) return invalid("CONV taps must be finite");
        uint32_t parts = 0;
        if (conv_plan(T, 0, 1, 1, &parts, nullptr, nullptr)) return invalid("CONV plugin: bad tap count");
        {
            std::lock_guard<std::mutex> lk(g_mu);
            const CachedTable *ct = nullptr;
            const int st = cached_table(g_res[dev].conv, key, dev, s, "a CONV impulse response's partition spectra",
                                        [&](std::vector<float> &h, CachedTable &) {
                h.assign((size_t)parts * 4 * kConvSpec4, 0.f);
                conv_table(key.data(), T, h.data());
            }, &ct, kConvCacheBytes);
            if (st) return st;
            *table = ct->dev;  // held by the call (copied under the lock)
        }
        m->kind = MapKind::Conv;
        m->convH = table->get();
        m->conv_parts = parts;
        m->ntaps = T;
        return DSP_OK;
    }
    case DSP_PLUGIN_BIQUAD: {  // build-defined: Parameters{float coef[5 S]}, S = 1..4 sections
        const uint32_t S = p->params_size / 20;
        if (!p->params || S == 0 || S > 4 || p->params_size % 20)
            return invalid("BIQUAD plugin needs 1..4 sections of 5 floats (b0 b1 b2 a1 a2) as its params blob");
        std::vector<float> key((const float *)p->params, (const float *)p->params + 5 * S);
        for (float v : key)
            if (!std::isfinite(v)) return invalid("BIQUAD coefficients must be finite");
        uint32_t window = 0;
        {
            std::lock_guard<std::mutex> lk(g_mu);
            const CachedTable *it = nullptr;
            const int st = cached_table(g_res[dev].iir, key, dev, s, "a BIQUAD cascade's state-transition tables",
                                        [&](std::vector<float> &h, CachedTable &e) {
                e.window = biquad_tables(key.data(), S, biquad_lane_samples(), h);
            }, &it);
            if (st) return st;
            *table = it->dev;  // held by the call (copied under the lock)
            window = it->window;
        }
        m->kind = MapKind::Biquad;
        m->iir_tab = table->get();
        m->sections = S;
        m->iir_window = window;
        return DSP_OK;
    }
    case DSP_PLUGIN_GENERIC:  // the plugin's own audio_callback, compiled for gfx950 (module.h)
        if (!p->module) return invalid("GENERIC plugin needs a loaded dsp_module");
        m->kind = MapKind::Generic;
        m->module = const_cast<void *>(p->module);
        m->gparams = p->params;
        m->gparams_size = p->params_size;
        m->gflags = flags;
        return DSP_OK;
    default:
        return invalid("unknown plugin kind %d", p->kind);
    }
}

// A GENERIC plugin with a known block class (module.h dsp_module_block_class)
// runs as that map: its own callback's block as a table, or its gain.
// in_place: the call renders over its own input; with DSP_EXEC_VERIFY_CLASS
// the callback then runs on every block, since the check needs the input
// after the render (and a re-render would need it whole)
// a table class's block held by a call: released (an event after the call's
// launches on its stream) when the call returns, so an evicted table is freed
// only after every launch that reads it
struct SpecHold {
    ::dsp_module *m = nullptr;
    void *use = nullptr;
    hipStream_t s = nullptr;
    DevTable table;  // the call's FIR / BIQUAD table (plugin_map)
    ~SpecHold() {
        if (use) (void)module_spec_done(m, use, s);
    }
};

static int specialize_generic(SampleMap *m, uint32_t C, uint32_t B, hipStream_t s, const dsp_exec *ex,
                              bool in_place, SpecHold *hold) {
    if (m->kind != MapKind::Generic || (ex && (ex->flags & DSP_EXEC_NO_SPECIALIZE))) return DSP_OK;
    if (in_place && ex && (ex->flags & DSP_EXEC_VERIFY_CLASS)) return DSP_OK;
    ModuleSpec sp;
    int st = module_specialize((::dsp_module *)m->module, m->gparams, m->gparams_size, C, B, m->sr, s, &sp);
    if (st) return st;
    hold->m = (::dsp_module *)m->module;
    hold->use = sp.use;
    hold->s = s;
    if (sp.kind == kSpecTable) {
        m->kind = MapKind::Ramp;  // value = table[(global sample) mod B]
        m->table = sp.table;
        m->closed = 0;
        if (sp.affine) {  // ... = (float)fma(-i, rs, rg0), checked against every table value
            m->closed = 2;  // (the table is the callback's own block: nothing to build)
            m->rg0 = sp.rg0;
            m->rs = sp.rs;
        }
    } else if (sp.kind == kSpecGain) {
        m->kind = MapKind::Gain;
        m->a = sp.gain;
    } else if (sp.kind == kSpecGainTable) {
        m->kind = MapKind::GainTable;  // value = x * table[c B + (global sample) mod B]
        m->table = sp.table;
        m->closed = 0;
    }
    return DSP_OK;
}

// DSP_EXEC_VERIFY_CLASS: after a GENERIC plugin rendered by its block class,
// run its callback on blocks of the call's own input -- the first, the last
// and two more (a hash of the call's length and offset) -- as render_audio
// hands them over (audio.cpp:13-175: the file, zeros past EOF and for the
// channels the file lacks), and compare with the rendered rows bit for bit.
// *ok = false on any difference.  Synchronises the stream.
static int verify_class(const SampleMap &orig, const float *const *in, uint32_t in_ch, uint64_t L,
                        float *const *out, uint32_t C, uint32_t B, uint64_t goff, hipStream_t s, bool *ok) {
    *ok = true;
    const uint64_t nb = (L + B - 1) / B;
    if (nb == 0) return DSP_OK;
    uint64_t pick[4] = {0, nb - 1, 0, 0};
    uint64_t h = (L * 0x9e3779b97f4a7c15ull) ^ (goff + 0x632be59bd9b4e019ull);
    for (int i = 2; i < 4; ++i) {
        h ^= h >> 29;
        h *= 0xbf58476d1ce4e5b9ull;
        h ^= h >> 32;
        pick[i] = h % nb;
    }
    const uint64_t n = (uint64_t)C * B;
    float *d = nullptr;
    DSPB_HIP(hipMalloc(&d, sizeof(float) * n));
    struct Free {
        float *p;
        ~Free() { (void)hipFree(p); }
    } fr{d};
    std::vector<float> blk(n), got(n), want(n);
    for (uint64_t b : pick) {
        const uint64_t i0 = b * B;
        const uint64_t m = L > i0 ? std::min<uint64_t>(B, L - i0) : 0;  // file samples in the block
        std::fill(blk.begin(), blk.end(), 0.f);
        for (uint32_t c = 0; c < std::min(in_ch, C); ++c)
            if (m) DSPB_HIP(hipMemcpyAsync(blk.data() + (uint64_t)c * B, in[c] + i0, m * sizeof(float),
                                           hipMemcpyDeviceToHost, s));
        for (uint32_t c = 0; c < C; ++c)
            DSPB_HIP(hipMemcpyAsync(got.data() + (uint64_t)c * B, out[c] + i0, (uint64_t)B * sizeof(float),
                                    hipMemcpyDeviceToHost, s));
        DSPB_HIP(hipStreamSynchronize(s));
        DSPB_HIP(hipMemcpyAsync(d, blk.data(), sizeof(float) * n, hipMemcpyHostToDevice, s));
        std::vector<float *> rows(C);
        for (uint32_t c = 0; c < C; ++c) rows[c] = d + (uint64_t)c * B;
        if (int st = module_callback_once((::dsp_module *)orig.module, orig.gparams, orig.gparams_size, rows.data(),
                                          C, B, orig.sr, s))
            return st;
        DSPB_HIP(hipMemcpyAsync(want.data(), d, sizeof(float) * n, hipMemcpyDeviceToHost, s));
        DSPB_HIP(hipStreamSynchronize(s));
        if (std::memcmp(want.data(), got.data(), sizeof(float) * n) != 0) {
            *ok = false;
            set_last_error("DSP_EXEC_VERIFY_CLASS: block %llu rendered by the block class differs from the "
                           "plugin's callback; rendered again with the callback",
                           (unsigned long long)b);
            return DSP_OK;
        }
    }
    return DSP_OK;
}

static void set_result(const dsp_exec *ex, uint32_t bits) {
    if (ex && ex->result) *ex->result = bits;
}
static void or_result(const dsp_exec *ex, uint32_t bits) {
    if (ex && ex->result) *ex->result |= bits;
}

static hipStream_t stream_of(const dsp_exec *ex) { return ex ? (hipStream_t)ex->stream : nullptr; }
static bool host_mode(const dsp_exec *ex) { return ex && (ex->flags & DSP_EXEC_HOST_BUFFERS); }
static uint64_t goff_of(const dsp_exec *ex) { return ex ? ex->sample_offset : 0; }

// a GENERIC plugin rendered by its block class (specialize_generic) rather than its callback
static bool by_class(MapKind plugin, MapKind rendered) {
    return plugin == MapKind::Generic && rendered != MapKind::Generic;
}

// DSP_EXEC_VERIFY_CLASS after a render by block class: the check, and the
// VERIFIED / RERENDERED bit.  *rerender: the caller renders again with `orig`.
static int verify_class_result(const dsp_exec *ex, const SampleMap &orig, const SampleMap &map,
                               const float *const *in, uint32_t in_ch, uint64_t L, float *const *out, uint32_t C,
                               uint32_t B, hipStream_t s, bool *rerender) {
    *rerender = false;
    if (!by_class(orig.kind, map.kind) || !(ex && (ex->flags & DSP_EXEC_VERIFY_CLASS))) return DSP_OK;
    bool ok = true;
    if (int st = verify_class(orig, in, in_ch, L, out, C, B, goff_of(ex), s, &ok)) return st;
    set_result(ex, DSP_RESULT_CLASS | (ok ? DSP_RESULT_VERIFIED : DSP_RESULT_RERENDERED));
    *rerender = !ok;
    return DSP_OK;
}

// ---------------------------------------------------------------------------
// argument checks (before DeviceGuard: they need no device)
// ---------------------------------------------------------------------------
static int check_rows(const char *name, const float *const *rows, uint32_t n) {
    if (n && !rows) return invalid("%s is NULL", name);
    for (uint32_t c = 0; c < n; ++c)
        if (!rows[c]) return invalid("%s[%u] is NULL", name, c);
    return DSP_OK;
}

static int check_offset(const dsp_exec *ex, uint32_t B) {
    if (ex && ex->sample_offset % B) return invalid("sample_offset must be a multiple of B");
    return DSP_OK;
}

// ---------------------------------------------------------------------------
// host-buffer staging (DSP_EXEC_HOST_BUFFERS), one Stage per call.  Device
// mode: in() / out() hand the caller's pointer back.  Host mode: a device
// buffer each (freed when the call returns), the input copied on the call's
// stream, the outputs copied back by copy_back(); finish() then synchronises.
// The first failure sticks in `status` (checked once after the call's in() /
// out()s); zero-length buffers are one float and are not copied.
// ---------------------------------------------------------------------------
struct Stage {
    const bool host;
    const hipStream_t s;
    int status = DSP_OK;
    struct Back { void *host; const void *dev; size_t bytes; };
    std::vector<void *> bufs;
    std::vector<Back> back;

    explicit Stage(const dsp_exec *ex) : host(host_mode(ex)), s(stream_of(ex)) {}
    ~Stage() {
        for (void *p : bufs) (void)hipFree(p);
    }
    int alloc(size_t bytes, void **p) {  // whole floats
        *p = nullptr;
        if (status) return status;
        DSPB_HIP(hipMalloc(p, std::max<size_t>((bytes + 3) & ~(size_t)3, sizeof(float))));
        bufs.push_back(*p);
        return DSP_OK;
    }
    int copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
        if (bytes) DSPB_HIP(hipMemcpyAsync(dst, src, bytes, kind, s));
        return DSP_OK;
    }
    const void *in_bytes(const void *p, size_t bytes) {
        if (!host) return p;
        void *d;
        if ((status = alloc(bytes, &d)) == DSP_OK) status = copy(d, p, bytes, hipMemcpyHostToDevice);
        return d;
    }
    void *out_bytes(void *p, size_t bytes) {
        if (!host) return p;
        void *d;
        if ((status = alloc(bytes, &d)) == DSP_OK) back.push_back(Back{p, d, bytes});
        return d;
    }
    const float *in(const float *p, uint64_t n) { return (const float *)in_bytes(p, n * sizeof(float)); }
    float *out(float *p, uint64_t n) { return (float *)out_bytes(p, n * sizeof(float)); }
    std::vector<const float *> in_rows(const float *const *rows, uint32_t C, uint64_t n) {
        std::vector<const float *> d(C);
        for (uint32_t c = 0; c < C; ++c) d[c] = in(rows[c], n);
        return d;
    }
    std::vector<float *> out_rows(float *const *rows, uint32_t C, uint64_t n) {
        std::vector<float *> d(C);
        for (uint32_t c = 0; c < C; ++c) d[c] = out(rows[c], n);
        return d;
    }
    int copy_back() {  // in the order of the out()s
        for (const Back &b : back)
            if (int st = copy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost)) return st;
        return DSP_OK;
    }
};

// ---------------------------------------------------------------------------
// channel groups: a kernel takes at most kMaxChannels row pointers
// ---------------------------------------------------------------------------
// f(c0, cn) for rows [c0, c0 + cn) of C, group after group; the first error ends the walk
template <class F>
static int for_groups(uint32_t C, F f) {
    for (uint32_t c0 = 0; c0 < C; c0 += kMaxChannels) {
        if (int st = f(c0, std::min<uint32_t>(C - c0, kMaxChannels))) return st;
    }
    return DSP_OK;
}

// A group's rows split for the kernels that run two channels per wavefront:
// f(first, count, 2) for its even run of pairs (when `pairs`), then
// f(first, count, 1) for what is left -- the odd last channel, or every row
template <class F>
static int for_pairs_then_rest(uint32_t cn, bool pairs, F f) {
    const uint32_t np = pairs ? cn & ~1u : 0;  // (kMaxChannels is even)
    if (np)
        if (int st = f(0u, np, 2u)) return st;
    return cn > np ? f(np, cn - np, 1u) : DSP_OK;
}

// Rows [c0, c0 + cn) of a call as a launch's pointer tables: every output
// row, and the input rows the file has (*in_ch: one past the last of them).
// Returns which of the pointers it touched are all `align`-byte aligned.
enum : uint32_t { kOutAligned = 1, kInAligned = 2, kAllAligned = 3 };
static uint32_t fill_rows(const float *const *in, uint32_t in_channels, float *const *out, uint32_t c0, uint32_t cn,
                          ChanIn *src, uint32_t *in_ch, ChanOut *dst, size_t align = 4) {
    uint32_t al = kAllAligned;
    *in_ch = 0;
    for (uint32_t j = 0; j < cn; ++j) {
        dst->p[j] = out[c0 + j];
        if (!aligned(out[c0 + j], align)) al &= ~kOutAligned;
        if (c0 + j < in_channels) {
            src->p[j] = in[c0 + j];
            *in_ch = j + 1;
            if (!aligned(in[c0 + j], align)) al &= ~kInAligned;
        }
    }
    return al;
}

// a group's view of the call's map: a GainTable's rows start at the group's
// first channel (module_specialize refuses C > kMaxChannels, so c0 is 0 today)
static SampleMap group_map(const SampleMap &m, uint32_t c0) {
    SampleMap g = m;
    if (m.kind == MapKind::GainTable) g.table += (uint64_t)c0 * m.B;
    return g;
}

static int finish(const dsp_exec *ex) {
    if (ex && (ex->flags & (DSP_EXEC_SYNC | DSP_EXEC_HOST_BUFFERS)))
        DSPB_HIP(hipStreamSynchronize(stream_of(ex)));
    return DSP_OK;
}

// ---------------------------------------------------------------------------
// core device-pointer implementations
// ---------------------------------------------------------------------------
static int render_device(const float *const *in, uint32_t in_ch, uint64_t L, float *const *out,
                         uint32_t C, uint32_t B, const SampleMap &map, uint64_t start,
                         uint64_t goff, hipStream_t s) {
    const uint64_t nblocks = (L + B - 1) / B;
    const uint64_t end = nblocks * B;
    if (map.kind == MapKind::Generic) {
        if (start != 0) return invalid("GENERIC render: the fused tail path does not apply");
        return module_render((::dsp_module *)map.module, map.gparams, map.gparams_size, in, in_ch, L, out, C, B,
                             map.sr, goff, s, map.gflags);
    }
    if (map.kind == MapKind::Biquad) {  // the cascade from zero state at the start of the file
        if (start != 0 || goff != 0) return invalid("BIQUAD render: whole files only (sample_offset 0)");
        int dev = 0;
        DSPB_HIP(hipGetDevice(&dev));
        const uint32_t S = map.sections, D = 2 * S;
        // channel pairs in one wavefront (packed math) from kIirPairSections
        // sections on; an odd last channel on its own
        const bool pairs = S >= kIirPairSections;
        return for_groups(C, [&](uint32_t c0, uint32_t cn) {
            return for_pairs_then_rest(cn, pairs, [&](uint32_t first, uint32_t count, uint32_t nch) {
                BiquadArgs A{};
                const uint32_t al = fill_rows(in, in_ch, out, c0 + first, count, &A.in, &A.in_ch, &A.out, 16);
                A.in_aligned16 = (al & kInAligned) ? 1u : 0u;
                A.out_aligned16 = (al & kOutAligned) ? 1u : 0u;
                A.L = L;
                A.Ly = end;
                A.C = count;
                A.ntiles_ch = biquad_tiles(end);
                A.coef = map.iir_tab;
                A.Q = map.iir_tab + 20;
                A.P = A.Q + (size_t)65 * D * D;
                A.window = map.iir_window;
                return iir_launch(dev, s, &A, S, nch);
            });
        });
    }
    if (map.kind == MapKind::Conv) {  // partitioned convolution from the start of the file
        if (start != 0 || goff != 0) return invalid("CONV render: whole files only (sample_offset 0)");
        if (rows_overlap(in, std::min(in_ch, C), L, out, C, end))
            return invalid("CONV render: output rows overlap input rows (a frame's input is read after its "
                           "neighbour's output is written)");
        const v2f *tw = nullptr;
        int dev = 0;
        DSPB_HIP(hipGetDevice(&dev));
        if (int st = get_tw(dev, s, &tw)) return st;
        // sized by dsp_conv_plan's own function: one channel group's spectra
        uint64_t F = 0, scratch_bytes = 0;
        if (const char *why = conv_plan(map.ntaps, L, B, C, nullptr, &F, &scratch_bytes)) return invalid("%s", why);
        float *scratch = nullptr;
        if (int st = get_scratch(dev, s, scratch_bytes, &scratch, 2)) return st;
        return for_groups(C, [&](uint32_t c0, uint32_t cn) {
            ConvArgs A{};
            fill_rows(in, in_ch, out, c0, cn, &A.in, &A.in_ch, &A.out);
            A.L = L;
            A.Ly = end;
            A.F = F;
            A.H = reinterpret_cast<const float4 *>(map.convH);
            A.parts = map.conv_parts;
            A.X = reinterpret_cast<float4 *>(scratch);
            A.Y = A.X + (uint64_t)cn * F * kConvSpec4;
            A.tw = tw;
            return launch_conv(A, cn, s);
        });
    }
    if (map.kind == MapKind::Fir) {  // convolution from the start of the file
        if (start != 0 || goff != 0) return invalid("FIR render: whole files only (sample_offset 0)");
        if (map.ntaps <= 1025 && !map.fir_direct) {
            // overlap-save: channel pairs as one complex signal (fir_pair_kernel,
            // 4096-point frames); an odd last channel on its own
            // (fir_fft_kernel, 8192-point real frames)
            const v2f *tw = nullptr;
            int dev = 0;
            DSPB_HIP(hipGetDevice(&dev));
            int st = get_tw(dev, s, &tw);
            if (st) return st;
            return for_groups(C, [&](uint32_t c0, uint32_t cn) {
                return for_pairs_then_rest(cn, true, [&](uint32_t first, uint32_t count, uint32_t nch) {
                    FirFftArgs A{};
                    fill_rows(in, in_ch, out, c0 + first, count, &A.in, &A.in_ch, &A.out);
                    A.L = L;
                    A.Ly = end;
                    A.tw = tw;
                    if (nch == 2) {
                        A.F = (end + kPairHop - 1) / kPairHop;
                        A.H = map.pairH;
                        return launch_fir_pair(A, count, s);
                    }
                    A.F = (end + 7167) / 7168;
                    A.H = map.olsH;
                    A.h2048 = v2f{map.olsH2048[0], map.olsH2048[1]};
                    return launch_fir_fft(A, 1, s);
                });
            });
        }
        for (uint32_t c = 0; c < C; ++c) {
            int st = launch_fir(c < in_ch ? in[c] : nullptr, L, out[c], end, map.taps, map.ntaps8,
                                aligned(out[c], 16), s);
            if (st) return st;
        }
        return DSP_OK;
    }
    return for_groups(C, [&](uint32_t c0, uint32_t cn) {
        RenderArgs A{};
        const bool vec = fill_rows(in, in_ch, out, c0, cn, &A.in, &A.in_ch, &A.out, 16) == kAllAligned &&
                         (start % 4) == 0;
        A.L = L;
        A.start = start;
        A.end = end;
        A.map = group_map(map, c0);
        A.goff = goff;
        return launch_render(A, cn, vec, s);
    });
}

static int check_stft_args(uint32_t N, uint32_t H, uint32_t K, uint64_t ld, int32_t window) {
    if (window != DSP_WIN_HAMMING && window != DSP_WIN_HANN && window != DSP_WIN_RECT)
        return invalid("window=%d is not a DSP_WIN_* kind", window);
    if (!is_pow2(N) || N < 4 || N > 8192) return invalid("N=%u must be a power of two in [4, 8192]", N);
    if (H == 0) return invalid("hop H must be > 0");
    if (K == 0 || (K > N / 2 + 1 && K != N)) return invalid("K=%u must be <= N/2+1 or == N", K);
    if (ld < K) return invalid("ld=%llu < K=%u", (unsigned long long)ld, K);
    return DSP_OK;
}

// The memory-source part of an 8192-point STFT launch (launch_stft): tables,
// scale and frame geometry.  wincomp: the DSP_WIN_* kind whose computed form
// the launch may use (set_wincomp: a first-use table), or -1 for none.
static int stft8k_args(Stft8kArgs *A, int dev, hipStream_t s, const v2f *tw, const float *win, uint64_t F,
                       uint32_t H, uint32_t K, uint64_t ld, uint32_t valid, int wincomp) {
    A->F = F;
    A->H = H;
    A->K = K;
    A->ld = ld;
    A->valid = valid;
    A->win2 = reinterpret_cast<const v2f *>(win);
    A->tw = tw;
    A->scale = fft_scale(8192);
    return wincomp >= 0 ? set_wincomp(dev, s, wincomp, A) : DSP_OK;
}

static GenericFftArgs fft_args(const v2f *tw, uint32_t n, int dir) {
    GenericFftArgs A{};
    A.n = n;
    A.log2n = ilog2(n);
    A.dir = dir;
    A.tw = tw;
    A.scale = fft_scale(n);
    return A;
}

// frames of `valid` samples every `hop`, windowed and zero-padded to n -> K
// magnitudes per row of ld floats; the caller sets sig and mag
static GenericFftArgs fft_mag_args(const v2f *tw, const float *win, uint32_t n, uint32_t valid, uint64_t hop,
                                   uint32_t K, uint64_t ld) {
    GenericFftArgs A = fft_args(tw, n, -1);
    A.frame_hop = hop;
    A.valid = valid;
    A.win = win;
    A.K = K;
    A.ld = ld;
    A.mode = 2;
    return A;
}

static int stft_device(const float *const *in, uint32_t C, uint64_t L, uint32_t N, uint32_t H,
                       int window, uint32_t K, float *const *mag, uint64_t ld, int dev,
                       hipStream_t s) {
    const uint64_t F = dsp_stft_frame_count(L, N, H);
    if (F == 0) return DSP_OK;
    const v2f *tw = nullptr;
    const float *win = nullptr;
    int st = get_tw(dev, s, &tw);
    if (st) return st;
    bool fast = (N == 8192) && (H % 2 == 0);
    for (uint32_t c = 0; c < C; ++c) fast = fast && aligned(in[c], 8);
    st = get_window(dev, s, window, N, N, &win, fast ? window_prescale(N) : 1.0);
    if (st) return st;
    return for_groups(C, [&](uint32_t c0, uint32_t cn) {
        uint32_t in_ch;  // = cn: every row is signal
        if (!fast) {
            GenericFftArgs A = fft_mag_args(tw, win, N, N, H, K, ld);
            fill_rows(in, C, mag, c0, cn, &A.sig, &in_ch, &A.mag);
            return launch_fft_generic(A, F, cn, s);
        }
        Stft8kArgs A{};
        fill_rows(in, C, mag, c0, cn, &A.in, &A.in_ch, &A.mag);
        A.L = L;
        if (int e = stft8k_args(&A, dev, s, tw, win, F, H, K, ld, N, window)) return e;
        TimedLaunch tl{};
        if (int e = timing_begin(s, &tl)) return e;
        if (int e = launch_stft(A, cn, false, s)) return e;
        // algorithmic bytes: frame input read once per hop + magnitudes
        return timing_end(s, &tl, (uint64_t)cn * F * ((uint64_t)H * 4 + (uint64_t)K * 4));
    });
}

// GENERIC render + STFT: the plugin's own callback renders the whole file
// (module.cpp, the LDS-blocks driver), then the memory-source STFT reads the
// render back, both on the caller's stream.  Measured against the
// alternatives: chunks pipelined through the Infinity Cache on
// two streams, and three kernels fusing the callback with the FFT, were all
// slower -- a plugin callback runs serially over its block, and the LDS that
// holds blocks in flight is the same LDS the FFT's transposes need.
static int generic_render_stft(const float *const *in, uint32_t in_ch, uint64_t L, float *const *out, uint32_t C,
                               uint32_t B, const SampleMap &map, uint32_t N, uint32_t H, int window, uint32_t K,
                               float *const *mag, uint64_t ld, uint64_t goff, int dev, hipStream_t s) {
    const uint64_t Lr = (L + B - 1) / B * B;
    int st = module_render((::dsp_module *)map.module, map.gparams, map.gparams_size, in, in_ch, L, out, C, B,
                           map.sr, goff, s, map.gflags);
    return st ? st : stft_device(out, C, Lr, N, H, window, K, mag, ld, dev, s);
}

}  // namespace dspb

using namespace dspb;

// ===========================================================================
// extern "C"
// ===========================================================================
extern "C" {

int dsp_abi_version(void) { return DSPBENCH_ABI_VERSION; }



void dsp_kernel_timing_enable(int on) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_timing = on != 0;
    // a stock of events for the current device, created here rather than
    // between the launches being timed
    int dev = 0;
    if (g_timing && hipGetDevice(&dev) == hipSuccess) {
        auto &pool = g_event_pool[dev];
        while (pool.size() < 1024) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) break;
            pool.push_back(e);
        }
    }
}

int dsp_kernel_timing(double *total_ms, uint64_t *launches, uint64_t *bytes) {
    std::vector<TimedLaunch> v;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        v.swap(g_timed);
    }
    double ms = 0.0;
    uint64_t b = 0;
    for (auto &t : v) {
        float e = 0.f;
        DSPB_HIP(hipEventSynchronize(t.stop));
        DSPB_HIP(hipEventElapsedTime(&e, t.start, t.stop));
        ms += e;
        b += t.bytes;
    }
    {
        std::lock_guard<std::mutex> lk(g_mu);
        for (auto &t : v) {
            g_event_pool[t.dev].push_back(t.stop);
            g_event_pool[t.dev].push_back(t.start);
        }
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = v.size();
    if (bytes) *bytes = b;
    return DSP_OK;
}

const char *dsp_last_error(void) { return g_last_error; }

const char *dsp_status_string(int s) {
    switch (s) {
    case DSP_OK: return "ok";
    case DSP_ERR_INVALID: return "invalid argument";
    case DSP_ERR_HIP: return "HIP runtime error";
    case DSP_ERR_UNSUPPORTED: return "unsupported";
    case DSP_ERR_NOMEM: return "out of device memory";
    case DSP_ERR_NO_DEVICE: return "no device";
    default: return "unknown status";
    }
}

int dsp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int dsp_debug_set(int what, uint64_t value) {
    if (what == DSP_DEBUG_FRAME_RUN) {
        if (value > 0xffffu) return invalid("dsp_debug_set: frame run %llu > 65535", (unsigned long long)value);
        g_frame_run.store((uint32_t)value);
        return DSP_OK;
    }
    if (what != DSP_DEBUG_BIQUAD_SPIN_LIMIT) return invalid("dsp_debug_set: unknown hook %d", what);
    g_iir_spin_limit.store(value > 0xffffffffull ? kIirSpinLimit : (uint32_t)value);
    return DSP_OK;
}

int dsp_debug_get(int what, uint64_t *value) {
    if (what == DSP_DEBUG_FRAME_RUN && value) {
        *value = g_frame_run.load();
        return DSP_OK;
    }
    if (what != DSP_DEBUG_BIQUAD_REPAIRS || !value) return invalid("dsp_debug_get: unknown hook %d", what);
    int dev = 0;
    if (int st = current_device(&dev)) return st;
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceRes &r = g_res[dev];
    *value = 0;
    if (r.iir_fb_host) {
        *value = __atomic_exchange_n(r.iir_fb_host, 0u, __ATOMIC_SEQ_CST);
    }
    return DSP_OK;
}

int dsp_biquad_plan(const float *coef, uint32_t sections, uint32_t *window) {
    if (!coef || !window || sections == 0 || sections > 4) return invalid("dsp_biquad_plan: 1..4 sections");
    for (uint32_t q = 0; q < 5 * sections; ++q)
        if (!std::isfinite(coef[q])) return invalid("BIQUAD coefficients must be finite");
    std::vector<float> h;
    *window = biquad_tables(coef, sections, biquad_lane_samples(), h);
    return DSP_OK;
}

int dsp_conv_plan(uint32_t taps, uint64_t L, uint32_t B, uint32_t C, uint32_t *partitions, uint64_t *frames,
                  uint64_t *scratch_bytes) {
    if (const char *why = conv_plan(taps, L, B, C, partitions, frames, scratch_bytes)) return invalid("%s", why);
    return DSP_OK;
}

// dsp_resample_plan's checks and the library's ResamplePlan (NULL spec: the defaults)
static int resample_plan_checked(uint32_t sr_in, uint32_t sr_out, uint64_t L, const dsp_resample_spec *spec,
                                 ResamplePlan *plan) {
    const dsp_resample_spec def{64u, 14.769656459379492, 0.9475937167399596};
    if (!spec) spec = &def;
    const char *why = nullptr;
    const int r = resample_plan(sr_in, sr_out, L, spec->zeros, spec->beta, spec->rolloff, plan, &why);
    if (r == 0) return DSP_OK;
    set_last_error("%s", why);
    return r == 1 ? DSP_ERR_INVALID : DSP_ERR_UNSUPPORTED;
}

int dsp_resample_plan(uint32_t sr_in, uint32_t sr_out, uint64_t L, const dsp_resample_spec *spec, uint32_t *up,
                      uint32_t *down, uint32_t *taps_per_phase, uint64_t *Lout, uint64_t *table_bytes) {
    ResamplePlan p;
    if (int st = resample_plan_checked(sr_in, sr_out, L, spec, &p)) return st;
    if (up) *up = p.up;
    if (down) *down = p.down;
    if (taps_per_phase) *taps_per_phase = p.taps;
    if (Lout) *Lout = p.Lout;
    if (table_bytes) *table_bytes = p.table_bytes;
    return DSP_OK;
}

int dsp_resample_taps(uint32_t sr_in, uint32_t sr_out, const dsp_resample_spec *spec, float *table, uint64_t count) {
    ResamplePlan p;
    if (int st = resample_plan_checked(sr_in, sr_out, 0, spec, &p)) return st;
    if (!table) return invalid("dsp_resample_taps: NULL table");
    if (count != (uint64_t)p.up * p.taps)
        return invalid("dsp_resample_taps: count %llu != up * taps = %llu", (unsigned long long)count,
                       (unsigned long long)p.up * p.taps);
    resample_table(p, table, p.taps, 0);
    return DSP_OK;
}

// The device table of a conversion's blocking (resample.hip), cached per device
// by (up, down, spec); *table is the caller's hold on it.
static int resample_cached_table(const ResamplePlan &p, const ResampleArgs &A, int dev, hipStream_t s,
                                 DevTable *table) {
    // (a double as three floats: the key compares by value)
    auto split = [](double v, std::vector<float> &k) {
        const float a = (float)v, b = (float)(v - (double)a), c = (float)(v - (double)a - (double)b);
        k.insert(k.end(), {a, b, c});
    };
    std::vector<float> key{(float)p.up, (float)p.down, (float)p.zeros};
    split(p.beta, key);
    split(p.rolloff, key);
    std::lock_guard<std::mutex> lk(g_mu);
    const CachedTable *rt = nullptr;
    const int st = cached_table(g_res[dev].resample, key, dev, s, "a sample-rate conversion's filter table",
                                [&](std::vector<float> &h, CachedTable &) {
        std::vector<float> plain((size_t)p.up * p.taps);
        resample_table(p, plain.data(), p.taps, 0);
        h.resize(resample_device_floats(A));
        resample_device_table(A, plain.data(), h.data());
    }, &rt, kConvCacheBytes);
    if (st) return st;
    *table = rt->dev;
    return DSP_OK;
}

int dsp_resample(const float *const *in, uint32_t C, uint64_t L, float *const *out, uint64_t Lout, uint32_t sr_in,
                 uint32_t sr_out, const dsp_resample_spec *spec, const dsp_exec *ex) {
    ResamplePlan p;
    int st;
    if ((st = resample_plan_checked(sr_in, sr_out, L, spec, &p))) return st;
    if (Lout != p.Lout)
        return invalid("dsp_resample: Lout %llu != the plan's %llu", (unsigned long long)Lout,
                       (unsigned long long)p.Lout);
    if (goff_of(ex) != 0) return invalid("dsp_resample: whole rows only (sample_offset 0)");
    if (C == 0 || L == 0) return DSP_OK;
    if ((st = check_rows("out", out, C)) || (st = check_rows("in", in, C))) return st;
    if (rows_overlap(in, C, L, out, C, Lout)) return invalid("dsp_resample: output rows overlap input rows");
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    Stage stage(ex);
    const std::vector<const float *> din = stage.in_rows(in, C, L);
    const std::vector<float *> dout = stage.out_rows(out, C, Lout);
    if (stage.status) return stage.status;
    if (p.up == 1 && p.down == 1) {  // the same rate: a copy, no filter
        for (uint32_t c = 0; c < C; ++c)
            DSPB_HIP(hipMemcpyAsync(dout[c], din[c], L * sizeof(float), hipMemcpyDeviceToDevice, s));
        return (st = stage.copy_back()) ? st : finish(ex);
    }
    ResampleArgs A{};
    A.L = L;
    A.Lout = Lout;
    A.up = p.up;
    A.down = p.down;
    A.half = p.half;
    A.Tp = p.taps;
    resample_blocking(&A);
    DevTable table;  // held until the call's launches are enqueued
    if ((st = resample_cached_table(p, A, g.dev, s, &table))) return st;
    A.table = table.get();
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        ResampleArgs G = A;
        G.out_aligned16 = 1;
        for (uint32_t j = 0; j < cn; ++j) {
            G.in.p[j] = din[c0 + j];
            G.out.p[j] = dout[c0 + j];
            if (!aligned(dout[c0 + j], 16)) G.out_aligned16 = 0;
        }
        return launch_resample(G, cn, s);
    });
    if (st) return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

// The true-peak detector's table (dsp_loudness, dsp_limiter): dsp_resample's
// cached device table for sr -> ovs sr, whose blocking must be one group of ovs
// phases with coinciding windows, table[step][phase], R->S steps
static int oversampler_table(const ResamplePlan &rp, uint64_t L, uint32_t ovs, int dev, hipStream_t s,
                             ResampleArgs *R, DevTable *table) {
    R->L = L;
    R->Lout = rp.Lout;
    R->up = rp.up;
    R->down = rp.down;
    R->half = rp.half;
    R->Tp = rp.taps;
    resample_blocking(R);
    if (!R->phase || R->R != ovs || R->S != ((rp.taps + 3) & ~3u)) {
        set_last_error("unexpected blocking of the oversampling filter");
        return DSP_ERR_UNSUPPORTED;
    }
    return resample_cached_table(rp, *R, dev, s, table);
}

static int loudness_plan_checked(uint32_t sr, uint64_t L, LoudnessPlan *p) {
    const char *why = nullptr;
    if (loudness_plan(sr, L, p, &why) == 0) return DSP_OK;
    set_last_error("%s", why);
    return DSP_ERR_UNSUPPORTED;
}

int dsp_loudness_plan(uint32_t sr, uint64_t L, uint32_t *hop, uint64_t *hops, uint32_t *oversample, float kcoef[10],
                      uint64_t *scratch_bytes) {
    LoudnessPlan p;
    if (int st = loudness_plan_checked(sr, L, &p)) return st;
    if (hop) *hop = p.hop;
    if (hops) *hops = p.hops;
    if (oversample) *oversample = p.oversample;
    if (kcoef) std::memcpy(kcoef, p.kcoef, sizeof p.kcoef);
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return DSP_OK;
}

int dsp_loudness_gate(const double *const *hop_energy, uint32_t C, uint64_t hops, uint32_t hop, const float *weights,
                      dsp_loudness_result *res) {
    if (!res || C == 0 || hop == 0) return invalid("dsp_loudness_gate: needs res, C >= 1 and hop >= 1");
    if (hops) {
        if (!hop_energy) return invalid("hop_energy is NULL");
        for (uint32_t c = 0; c < C; ++c)
            if (!hop_energy[c]) return invalid("hop_energy[%u] is NULL", c);
    }
    loudness_gate(hop_energy, C, hops, hop, weights, res);
    return DSP_OK;
}

int dsp_loudness(const float *const *in, uint32_t C, uint64_t L, uint32_t sr, const float *weights, uint32_t flags,
                 const dsp_resample_spec *tp_spec, double *const *hop_energy, double *chan_peaks,
                 dsp_loudness_result *res, const dsp_exec *ex) {
    LoudnessPlan lp;
    int st;
    if ((st = loudness_plan_checked(sr, L, &lp))) return st;
    if (!res || C == 0) return invalid("dsp_loudness: needs res and C >= 1");
    if (flags & ~DSP_LOUDNESS_TRUE_PEAK) return invalid("dsp_loudness: unknown flags");
    if (goff_of(ex) != 0) return invalid("dsp_loudness: whole rows only (sample_offset 0)");
    if ((st = check_rows("in", in, C))) return st;
    if (lp.hops && hop_energy)
        for (uint32_t c = 0; c < C; ++c)
            if (!hop_energy[c]) return invalid("hop_energy[%u] is NULL", c);
    const bool want_tp = (flags & DSP_LOUDNESS_TRUE_PEAK) != 0;
    const bool run_tp = want_tp && lp.oversample > 1 && L > 0;
    ResamplePlan rp;
    if (want_tp && (st = resample_plan_checked(sr, sr * lp.oversample, L, tp_spec, &rp))) return st;  // (the spec's ranges)
    hipStream_t s = stream_of(ex);
    if (capturing(s)) {
        set_last_error("stream capture: dsp_loudness returns host values and synchronises its stream");
        return DSP_ERR_INVALID;
    }

    std::vector<double> z((size_t)C * lp.hops, 0.0);
    std::vector<uint32_t> peaks((size_t)C * 2, 0u);  // per channel: the bits of the sample and of the true peak
    if (L > 0) {
        DeviceGuard g(ex);
        if (g.status) return g.status;
        Stage stage(ex);
        const std::vector<const float *> din = stage.in_rows(in, C, L);
        if (stage.status) return stage.status;
        DevTable ktab, ttab;  // held until the call's launches are enqueued
        {
            // (an eleventh float: never a BIQUAD cascade's key, whose tables differ)
            std::vector<float> key(lp.kcoef, lp.kcoef + 10);
            key.push_back(0.f);
            std::lock_guard<std::mutex> lk(g_mu);
            const CachedTable *it = nullptr;
            st = cached_table(g_res[g.dev].iir, key, g.dev, s, "the K-weighting cascade's state-transition tables",
                              [&](std::vector<float> &h, CachedTable &) { loudness_tables(lp.kcoef, h); }, &it);
            if (st) return st;
            ktab = it->dev;
        }
        ResampleArgs R{};
        if (run_tp && (st = oversampler_table(rp, L, lp.oversample, g.dev, s, &R, &ttab))) return st;
        float *scratch = nullptr;
        if ((st = get_scratch(g.dev, s, lp.scratch_bytes, &scratch, 3))) return st;
        LoudnessArgs A{};
        A.L = L;
        A.tiles = lp.tiles;
        A.hop = lp.hop;
        A.hops = lp.hops;
        A.coef = ktab.get();
        A.Q = A.coef + 20;
        A.P = A.Q + (size_t)65 * 16;
        A.window = lp.window;
        A.run = lp.run;
        A.z = (double *)scratch;
        A.peaks = (uint32_t *)(A.z + (size_t)kLoudGroup * lp.hops);
        A.part = (float *)(A.peaks + 2 * kLoudGroup);
        st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
            LoudnessArgs G = A;
            G.in_aligned16 = 1;
            for (uint32_t j = 0; j < cn; ++j) {
                G.in.p[j] = din[c0 + j];
                if (!aligned(din[c0 + j], 16)) G.in_aligned16 = 0;
            }
            DSPB_HIP(hipMemsetAsync(G.peaks, 0, 2 * kLoudGroup * sizeof(uint32_t), s));
            int e = for_pairs_then_rest(cn, true, [&](uint32_t first, uint32_t count, uint32_t nch) {
                LoudnessArgs K = G;
                K.first = first;
                K.count = count;
                return launch_loudness_kweight(K, nch, s);
            });
            if (e) return e;
            if ((e = launch_loudness_finish(G, cn, s))) return e;
            if (run_tp && (e = launch_loudness_truepeak(G, cn, lp.oversample, ttab.get(), R.S, rp.half, s))) return e;
            for (uint32_t j = 0; j < cn; ++j) {
                if (lp.hops)
                    DSPB_HIP(hipMemcpyAsync(z.data() + (size_t)(c0 + j) * lp.hops, G.z + (size_t)j * lp.hops,
                                            lp.hops * sizeof(double), hipMemcpyDeviceToHost, s));
                DSPB_HIP(hipMemcpyAsync(&peaks[2 * (size_t)(c0 + j)], G.peaks + j, sizeof(uint32_t),
                                        hipMemcpyDeviceToHost, s));
                DSPB_HIP(hipMemcpyAsync(&peaks[2 * (size_t)(c0 + j) + 1], G.peaks + kLoudGroup + j, sizeof(uint32_t),
                                        hipMemcpyDeviceToHost, s));
            }
            return (int)DSP_OK;
        });
        if (st) return st;
        DSPB_HIP(hipStreamSynchronize(s));
    }

    std::vector<const double *> rows(C);
    for (uint32_t c = 0; c < C; ++c) rows[c] = z.data() + (size_t)c * lp.hops;
    loudness_gate(rows.data(), C, lp.hops, lp.hop, weights, res);
    res->sample_peak = 0.0;
    res->true_peak = want_tp ? 0.0 : std::nan("");
    for (uint32_t c = 0; c < C; ++c) {
        float sp, tp;
        std::memcpy(&sp, &peaks[2 * (size_t)c], 4);
        std::memcpy(&tp, &peaks[2 * (size_t)c + 1], 4);
        const double spd = (double)sp, tpd = !want_tp ? std::nan("") : lp.oversample > 1 ? (double)tp : spd;
        res->sample_peak = std::max(res->sample_peak, spd);
        if (want_tp) res->true_peak = std::max(res->true_peak, tpd);
        if (chan_peaks) chan_peaks[2 * c] = spd, chan_peaks[2 * c + 1] = tpd;
        if (hop_energy && lp.hops) std::memcpy(hop_energy[c], rows[c], lp.hops * sizeof(double));
    }
    return DSP_OK;
}

// dsp_limiter_plan's checks: the limiter's own, then (TRUE_PEAK at ovs > 1) the oversampler's
static int limiter_plan_checked(uint32_t sr, uint64_t L, uint32_t C, const dsp_limiter_spec *spec,
                                const dsp_resample_spec *tp_spec, LimiterPlan *p, ResamplePlan *rp) {
    const char *why = nullptr;
    if (const int r = limiter_plan(sr, L, C, spec, p, &why)) {
        set_last_error("%s", why);
        return r == 1 ? DSP_ERR_INVALID : DSP_ERR_UNSUPPORTED;
    }
    if (spec->flags & DSP_LIMITER_TRUE_PEAK) return resample_plan_checked(sr, sr * p->oversample, L, tp_spec, rp);
    return DSP_OK;
}

int dsp_limiter_plan(uint32_t sr, uint64_t L, uint32_t C, const dsp_limiter_spec *spec, const dsp_resample_spec *tp_spec,
                     uint32_t *groups, uint32_t *oversample, float *rho, float *window, uint64_t *scratch_bytes) {
    LimiterPlan p;
    ResamplePlan rp;
    if (int st = limiter_plan_checked(sr, L, C, spec, tp_spec, &p, &rp)) return st;
    if (groups) *groups = p.groups;
    if (oversample) *oversample = p.oversample;
    if (rho) *rho = p.rho;
    if (window) limiter_window(p.lookahead, window);
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return DSP_OK;
}

// whether rows a[0..na) of la floats and b[0..nb) of lb floats overlap; with
// `same_ok`, a[c] == b[c] (in place) does not count
static bool limiter_rows_clash(const float *const *a, uint32_t na, const float *const *b, uint32_t nb, uint64_t n,
                               bool same_ok, bool self) {
    for (uint32_t i = 0; i < na; ++i)
        for (uint32_t j = self ? i + 1 : 0; j < nb; ++j) {
            if (same_ok && i == j && a[i] == b[j]) continue;
            const uintptr_t p = reinterpret_cast<uintptr_t>(a[i]), q = reinterpret_cast<uintptr_t>(b[j]);
            if (p < q + 4 * n && q < p + 4 * n) return true;
        }
    return false;
}

int dsp_limiter(const float *const *in, uint32_t C, uint64_t L, float *const *out, uint32_t sr,
                const dsp_limiter_spec *spec, const dsp_resample_spec *tp_spec, float *const *gain,
                float *const *detector, dsp_limiter_result *res, const dsp_exec *ex) {
    LimiterPlan lp;
    ResamplePlan rp;
    int st;
    if ((st = limiter_plan_checked(sr, L, C, spec, tp_spec, &lp, &rp))) return st;
    if (goff_of(ex) != 0) return invalid("dsp_limiter: whole rows only (sample_offset 0)");
    if (L == 0) {  // nothing to read or write: the rows are not looked at
        if (res) res->min_gain = 1.0, res->limited = 0;
        return DSP_OK;
    }
    if ((st = check_rows("in", in, C)) || (st = check_rows("out", out, C))) return st;
    const uint32_t G = lp.groups;
    if (gain && (st = check_rows("gain", gain, G))) return st;
    if (detector && (st = check_rows("detector", detector, G))) return st;
    {
        const float *const *o = out, *const *gr = gain, *const *dr = detector;
        bool clash = limiter_rows_clash(in, C, o, C, L, true, false) || limiter_rows_clash(o, C, o, C, L, false, true);
        if (gr) clash = clash || limiter_rows_clash(gr, G, in, C, L, false, false) ||
                        limiter_rows_clash(gr, G, o, C, L, false, false) || limiter_rows_clash(gr, G, gr, G, L, false, true);
        if (dr) clash = clash || limiter_rows_clash(dr, G, in, C, L, false, false) ||
                        limiter_rows_clash(dr, G, o, C, L, false, false) || limiter_rows_clash(dr, G, dr, G, L, false, true);
        if (gr && dr) clash = clash || limiter_rows_clash(gr, G, dr, G, L, false, false);
        if (clash) return invalid("dsp_limiter: rows overlap (only out[c] == in[c] is allowed)");
    }
    hipStream_t s = stream_of(ex);
    if (res) {
        res->min_gain = 1.0;
        res->limited = 0;
        if (capturing(s)) {
            set_last_error("stream capture: dsp_limiter with a result returns host values and synchronises its stream");
            return DSP_ERR_INVALID;
        }
    }
    DeviceGuard g(ex);
    if (g.status) return g.status;
    Stage stage(ex);
    std::vector<const float *> din(C);
    std::vector<float *> dout(C);
    for (uint32_t c = 0; c < C; ++c) {  // (in place stays in place on the device)
        dout[c] = stage.out(out[c], L);
        din[c] = stage.host && in[c] != out[c] ? stage.in(in[c], L) : stage.host ? dout[c] : in[c];
        if (stage.host && in[c] == out[c] && !stage.status)
            stage.status = stage.copy(dout[c], in[c], L * sizeof(float), hipMemcpyHostToDevice);
    }
    std::vector<float *> dgain(G, nullptr), ddet(G, nullptr);
    if (gain) dgain = stage.out_rows(gain, G, L);
    if (detector) ddet = stage.out_rows(detector, G, L);
    if (stage.status) return stage.status;

    DevTable ltab, ttab;  // held until the call's launches are enqueued
    {
        std::vector<float> key{lp.rho, (float)lp.lookahead};
        std::lock_guard<std::mutex> lk(g_mu);
        const CachedTable *it = nullptr;
        st = cached_table(g_res[g.dev].limiter, key, g.dev, s, "the limiter's release powers and attack window",
                          [&](std::vector<float> &h, CachedTable &) { limiter_table(lp, h); }, &it);
        if (st) return st;
        ltab = it->dev;
    }
    ResampleArgs R{};
    if (lp.oversample > 1 && (st = oversampler_table(rp, L, lp.oversample, g.dev, s, &R, &ttab))) return st;
    float *scratch = nullptr;
    if ((st = get_scratch(g.dev, s, lp.scratch_bytes, &scratch, 4))) return st;

    const uint64_t rowlen = lp.tiles * kLimTile;
    LimiterArgs A{};
    A.L = L;
    A.tiles = lp.tiles;
    A.A = lp.lookahead;
    A.wpad = lp.wpad;
    A.c = spec->ceiling;
    A.tab = ltab.get();
    A.h = scratch;
    A.pmax = lp.chunks > 1 ? scratch + (uint64_t)lp.rows * rowlen : nullptr;
    A.E = scratch + ((uint64_t)lp.rows + (lp.chunks > 1 ? 1 : 0)) * rowlen;
    A.carry = A.E + (uint64_t)lp.rows * lp.tiles;
    // (8-byte aligned: whole tiles before it, then two rows of `tiles` floats per scratch row)
    uint32_t *words = (uint32_t *)(A.carry + (uint64_t)lp.rows * lp.tiles);
    A.tp = ttab.get();
    A.steps = R.S;
    A.half = rp.half;
    DSPB_HIP(hipMemsetAsync(words, 0xff, 8, s));
    DSPB_HIP(hipMemsetAsync(words + 2, 0, 8, s));

    // rows [c0, c0 + cn) as a launch's tables
    auto rows_of = [&](uint32_t c0, uint32_t cn, LimiterArgs *K) {
        K->in_aligned16 = K->out_aligned16 = K->gain_aligned16 = 1;
        for (uint32_t j = 0; j < cn; ++j) {
            K->in.p[j] = din[c0 + j];
            K->out.p[j] = dout[c0 + j];
            if (!aligned(din[c0 + j], 16)) K->in_aligned16 = 0;
            if (!aligned(dout[c0 + j], 16)) K->out_aligned16 = 0;
        }
    };
    auto group_rows = [&](uint32_t g0, uint32_t gn, LimiterArgs *K) {
        for (uint32_t j = 0; j < gn; ++j) {
            K->gain.p[j] = dgain[g0 + j];
            K->det.p[j] = ddet[g0 + j];
            if (!aligned(dgain[g0 + j], 16)) K->gain_aligned16 = 0;
        }
    };
    if (G == 1) {
        // linked: pass 1 once per 16 channels, p combined (max, exact) in the
        // scratch row before the last launch takes the hold; pass 3 once per 16
        uint32_t chunk = 0;
        st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
            LimiterArgs K = A;
            rows_of(c0, cn, &K);
            group_rows(0, 1, &K);
            K.ngroups = 1;
            K.nch = cn;
            const bool last = chunk + 1 == lp.chunks;
            K.pmode = last ? 0u : chunk == 0 ? 1u : 2u;
            K.use_pmax = last && lp.chunks > 1;
            ++chunk;
            return launch_limiter_detect(K, lp.oversample, s);
        });
        if (st) return st;
        A.ngroups = 1;
        A.nch = 1;
        if ((st = launch_limiter_carry(A, s))) return st;
        st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
            LimiterArgs K = A;
            rows_of(c0, cn, &K);
            K.ngroups = 1;
            K.nch = cn;
            if (c0 == 0) {  // the group's gain row and counts: once
                group_rows(0, 1, &K);
                K.words = words;
            }
            return launch_limiter_apply(K, s);
        });
    } else {
        // unlinked: 16 groups of one channel per launch, the scratch rows reused in stream order
        st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
            LimiterArgs K = A;
            rows_of(c0, cn, &K);
            group_rows(c0, cn, &K);
            K.ngroups = cn;
            K.nch = 1;
            K.words = words;
            int e;
            if ((e = launch_limiter_detect(K, lp.oversample, s))) return e;
            if ((e = launch_limiter_carry(K, s))) return e;
            return launch_limiter_apply(K, s);
        });
    }
    if (st) return st;
    uint32_t w[4] = {0, 0, 0, 0};
    if (res) DSPB_HIP(hipMemcpyAsync(w, words, sizeof w, hipMemcpyDeviceToHost, s));
    if ((st = stage.copy_back())) return st;
    if (res) {
        DSPB_HIP(hipStreamSynchronize(s));
        const uint32_t b = (w[0] & 0x80000000u) ? (w[0] & 0x7fffffffu) : ~w[0];
        float m;
        std::memcpy(&m, &b, 4);
        res->min_gain = (double)m;
        res->limited = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
        return DSP_OK;
    }
    return finish(ex);
}

int dsp_rfft_plan(uint32_t n, uint32_t *passes, uint32_t radix[4], uint64_t *scratch_bytes_per_channel) {
    if (!rfft_plan(n, passes, radix)) return invalid("dsp_rfft: n must be a power of two in [2^10, 2^24]");
    if (scratch_bytes_per_channel) *scratch_bytes_per_channel = rfft_scratch_bytes(n);
    return DSP_OK;
}

// the twiddle table of n, cached per device; *hold keeps it until the call's launches are enqueued
static int rfft_cached_table(uint32_t n, int dev, hipStream_t s, DevTable *hold) {
    std::vector<float> key{(float)n};  // (a power of two: exact)
    std::lock_guard<std::mutex> lk(g_mu);
    const CachedTable *it = nullptr;
    const int st = cached_table(g_res[dev].rfft, key, dev, s, "the large FFT's twiddle table",
                                [&](std::vector<float> &h, CachedTable &) { rfft_twiddles(n, h); }, &it);
    if (st) return st;
    *hold = it->dev;
    return DSP_OK;
}

// a launch's plan, table and the work buffers of `nch` channels at `work`
static int big_fft_args(uint32_t n, uint32_t nch, const float *table, float *work, BigFftArgs *A) {
    A->n = n;
    A->nch = nch;
    if (!rfft_plan(n, &A->passes, A->radix)) return DSP_ERR_INVALID;
    A->tw = reinterpret_cast<const v2f *>(table);
    A->buf0 = reinterpret_cast<v2f *>(work);
    A->buf1 = A->buf0 + (uint64_t)nch * (n / 2);
    A->in_aligned8 = A->out_aligned8 = 1;
    return DSP_OK;
}

static bool rows_clash_each_other(float *const *rows, uint32_t C, uint64_t n) {
    for (uint32_t i = 0; i < C; ++i)
        if (rows_overlap(rows + i, 1, n, rows + i + 1, C - i - 1, n)) return true;
    return false;
}

int dsp_rfft(const float *const *in, uint32_t C, uint64_t L, uint32_t n, float *const *spec, const dsp_exec *ex) {
    int st;
    if ((st = dsp_rfft_plan(n, nullptr, nullptr, nullptr))) return st;
    if (L > n) return invalid("dsp_rfft: L %llu > n %u", (unsigned long long)L, n);
    if (goff_of(ex) != 0) return invalid("dsp_rfft: whole rows only (sample_offset 0)");
    if (C == 0) return DSP_OK;
    if ((st = check_rows("spec", spec, C)) || (L && (st = check_rows("in", in, C)))) return st;
    const uint64_t bins2 = (uint64_t)n + 2;  // floats of a spectrum
    if ((L && rows_overlap(in, C, L, spec, C, bins2)) || rows_clash_each_other(spec, C, bins2))
        return invalid("dsp_rfft: spectrum rows overlap input rows or each other");
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    Stage stage(ex);
    const std::vector<float *> dspec = stage.out_rows(spec, C, bins2);
    std::vector<const float *> din(C);
    for (uint32_t c = 0; c < C; ++c) din[c] = L ? stage.in(in[c], L) : dspec[c];  // (L = 0: never read)
    if (stage.status) return stage.status;
    DevTable table;
    if ((st = rfft_cached_table(n, g.dev, s, &table))) return st;
    const uint32_t rows = std::min<uint32_t>(C, kMaxChannels);
    float *work = nullptr;
    if ((st = get_scratch(g.dev, s, rows * rfft_scratch_bytes(n), &work, 5))) return st;
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        BigFftArgs A{};
        if (int e = big_fft_args(n, cn, table.get(), work, &A)) return e;
        A.L = L;
        for (uint32_t j = 0; j < cn; ++j) {
            A.in.p[j] = din[c0 + j];
            A.out.p[j] = dspec[c0 + j];
            if (!aligned(din[c0 + j], 8)) A.in_aligned8 = 0;
            if (!aligned(dspec[c0 + j], 8)) A.out_aligned8 = 0;
        }
        return launch_big_rfft(A, s);
    });
    if (st) return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

int dsp_irfft(const float *const *spec, uint32_t C, uint32_t n, float *const *out, uint64_t Lout,
              const dsp_exec *ex) {
    int st;
    if ((st = dsp_rfft_plan(n, nullptr, nullptr, nullptr))) return st;
    if (Lout > n) return invalid("dsp_irfft: Lout %llu > n %u", (unsigned long long)Lout, n);
    if (goff_of(ex) != 0) return invalid("dsp_irfft: whole rows only (sample_offset 0)");
    if (C == 0 || Lout == 0) return DSP_OK;
    if ((st = check_rows("spec", spec, C)) || (st = check_rows("out", out, C))) return st;
    const uint64_t bins2 = (uint64_t)n + 2;
    if (rows_overlap(spec, C, bins2, out, C, Lout) || rows_clash_each_other(out, C, Lout))
        return invalid("dsp_irfft: output rows overlap spectrum rows or each other");
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    Stage stage(ex);
    const std::vector<const float *> dspec = stage.in_rows(spec, C, bins2);
    const std::vector<float *> dout = stage.out_rows(out, C, Lout);
    if (stage.status) return stage.status;
    DevTable table;
    if ((st = rfft_cached_table(n, g.dev, s, &table))) return st;
    const uint32_t rows = std::min<uint32_t>(C, kMaxChannels);
    float *work = nullptr;
    if ((st = get_scratch(g.dev, s, rows * rfft_scratch_bytes(n), &work, 5))) return st;
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        BigFftArgs A{};
        if (int e = big_fft_args(n, cn, table.get(), work, &A)) return e;
        A.Lout = Lout;
        for (uint32_t j = 0; j < cn; ++j) {
            A.in.p[j] = dspec[c0 + j];
            A.out.p[j] = dout[c0 + j];
            if (!aligned(dspec[c0 + j], 8)) A.in_aligned8 = 0;
            if (!aligned(dout[c0 + j], 8)) A.out_aligned8 = 0;
        }
        return launch_big_irfft(A, s);
    });
    if (st) return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

int dsp_deconv_plan(uint64_t Ly, uint64_t Ls, uint32_t C, uint32_t *n, uint64_t *scratch_bytes) {
    const char *why = nullptr;
    if (const int r = deconv_plan(Ly, Ls, C, n, scratch_bytes, &why)) {
        set_last_error("%s", why);
        return r == 1 ? DSP_ERR_INVALID : DSP_ERR_UNSUPPORTED;
    }
    return DSP_OK;
}

int dsp_deconvolve(const float *const *rec, uint32_t C, uint64_t Ly, const float *ref, uint64_t Ls,
                   float *const *ir, uint64_t ir_len, const dsp_deconv_spec *spec, const dsp_exec *ex) {
    int st;
    uint32_t n = 0;
    uint64_t scratch_bytes = 0;
    if ((st = dsp_deconv_plan(Ly, Ls, C, &n, &scratch_bytes))) return st;
    const double eps = spec ? spec->eps : 1e-6;
    const uint32_t pre = spec ? spec->pre : 0;
    if (!std::isfinite(eps) || eps < 1e-12 || eps > 1.0) return invalid("dsp_deconvolve: eps must be in [1e-12, 1]");
    if (ir_len > n || pre > ir_len)
        return invalid("dsp_deconvolve: needs pre <= ir_len <= n (%u, %llu, %u)", pre, (unsigned long long)ir_len, n);
    if (goff_of(ex) != 0) return invalid("dsp_deconvolve: whole rows only (sample_offset 0)");
    if (!ref) return invalid("ref is NULL");
    if ((st = check_rows("rec", rec, C)) || (st = check_rows("ir", ir, C))) return st;
    if (rows_overlap(rec, C, Ly, ir, C, ir_len) || rows_overlap(&ref, 1, Ls, ir, C, ir_len) ||
        rows_clash_each_other(ir, C, ir_len))
        return invalid("dsp_deconvolve: ir rows overlap rec, ref or each other");
    hipStream_t s = stream_of(ex);
    DeviceGuard g(ex);
    if (g.status) return g.status;
    if (capturing(s)) {
        set_last_error("stream capture: dsp_deconvolve reads the excitation's maximum back and synchronises its stream");
        return DSP_ERR_INVALID;
    }
    Stage stage(ex);
    const std::vector<const float *> drec = stage.in_rows(rec, C, Ly);
    const float *dref = stage.in(ref, Ls);
    const std::vector<float *> dir = stage.out_rows(ir, C, ir_len);
    if (stage.status) return stage.status;
    DevTable table;
    if ((st = rfft_cached_table(n, g.dev, s, &table))) return st;
    float *scratch = nullptr;
    if ((st = get_scratch(g.dev, s, scratch_bytes, &scratch, 5))) return st;
    // [rows][2][M] work, [rows][M + 1] the recordings' spectra, [M + 1] the excitation's, the word of the maximum
    const uint32_t rows = std::min<uint32_t>(C, kMaxChannels), bins = n / 2 + 1;
    v2f *Y = reinterpret_cast<v2f *>(scratch) + (uint64_t)rows * n;
    v2f *S = Y + (uint64_t)rows * bins;
    uint32_t *word = reinterpret_cast<uint32_t *>(S + bins);
    DSPB_HIP(hipMemsetAsync(word, 0, 16, s));
    {
        BigFftArgs A{};
        if ((st = big_fft_args(n, 1, table.get(), scratch, &A))) return st;
        A.L = Ls;
        A.in.p[0] = dref;
        A.out.p[0] = reinterpret_cast<float *>(S);
        A.in_aligned8 = aligned(dref, 8);
        if ((st = launch_big_rfft(A, s)) || (st = launch_deconv_max(S, bins, word, s))) return st;
    }
    uint32_t maxbits = 0;
    DSPB_HIP(hipMemcpyAsync(&maxbits, word, sizeof maxbits, hipMemcpyDeviceToHost, s));
    DSPB_HIP(hipStreamSynchronize(s));
    if (maxbits == 0) return invalid("dsp_deconvolve: the excitation's spectrum is all zeros");
    if (ir_len) {
        st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
            BigFftArgs A{};
            if (int e = big_fft_args(n, cn, table.get(), scratch, &A)) return e;
            BigFftArgs B = A;
            A.L = Ly;
            B.Lout = ir_len;
            B.rot = pre & (n - 1);
            for (uint32_t j = 0; j < cn; ++j) {
                A.in.p[j] = drec[c0 + j];
                A.out.p[j] = B.out.p[j] = reinterpret_cast<float *>(Y + (uint64_t)j * bins);
                if (!aligned(drec[c0 + j], 8)) A.in_aligned8 = 0;
                B.in.p[j] = A.out.p[j];
                B.out.p[j] = dir[c0 + j];
                if (!aligned(dir[c0 + j], 8)) B.out_aligned8 = 0;
            }
            int e;
            if ((e = launch_big_rfft(A, s))) return e;
            if ((e = launch_deconv_divide(Y, S, bins, cn, (float)eps, word, s))) return e;
            return launch_big_irfft(B, s);
        });
        if (st) return st;
    }
    return (st = stage.copy_back()) ? st : finish(ex);
}

static int sweep_plan_checked(uint32_t sr, const dsp_sweep_spec *spec, SweepPlan *p) {
    const char *why = nullptr;
    if (sweep_plan(sr, spec, p, &why) == 0) return DSP_OK;
    set_last_error("%s", why);
    return DSP_ERR_INVALID;
}

int dsp_sweep_plan(uint32_t sr, const dsp_sweep_spec *spec, uint64_t *L, double *rate) {
    SweepPlan p;
    if (int st = sweep_plan_checked(sr, spec, &p)) return st;
    if (L) *L = p.L;
    if (rate) *rate = p.rate;
    return DSP_OK;
}

int dsp_sweep(uint32_t sr, const dsp_sweep_spec *spec, float *out, uint64_t count) {
    SweepPlan p;
    if (int st = sweep_plan_checked(sr, spec, &p)) return st;
    if (count > p.L) return invalid("dsp_sweep: count %llu > L %llu", (unsigned long long)count, (unsigned long long)p.L);
    if (count && !out) return invalid("out is NULL");
    sweep_fill(sr, spec, p, out, count);
    return DSP_OK;
}

int dsp_sweep_harmonic_offset(uint32_t sr, const dsp_sweep_spec *spec, uint32_t order, double *samples) {
    SweepPlan p;
    if (int st = sweep_plan_checked(sr, spec, &p)) return st;
    if (order == 0) return invalid("dsp_sweep_harmonic_offset: order must be >= 1");
    if (samples) *samples = sweep_harmonic_offset(sr, p, order);
    return DSP_OK;
}

uint64_t dsp_stft_frame_count(uint64_t L, uint32_t N, uint32_t H) {
    if (N == 0 || H == 0 || L < N) return 0;
    return (L - N) / H + 1;
}

int dsp_render_offline(const float *const *in, uint32_t in_channels, uint64_t L,
                       float *const *out, uint32_t C, uint32_t B, float sr,
                       const dsp_plugin *plugin, const dsp_exec *ex) {
    // (only a GENERIC plugin reads the sample rate)
    if (B == 0) return invalid("block size B must be > 0");
    if (C == 0) return DSP_OK;
    int st;
    if ((st = check_rows("out", out, C)) || (st = check_rows("in", in, in_channels)) || (st = check_offset(ex, B)))
        return st;
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    const uint64_t nblocks = (L + B - 1) / B;
    const uint64_t Lr = nblocks * B;

    Stage stage(ex);
    const std::vector<const float *> din = stage.in_rows(in, in_channels, L);
    const std::vector<float *> dout = stage.out_rows(out, C, Lr);
    if (stage.status) return stage.status;
    SpecHold hold;  // released after the call's launches
    SampleMap map;
    if ((st = plugin_map(plugin, B, g.dev, s, &map, sr, ex ? ex->flags : 0, &hold.table))) return st;
    const SampleMap orig = map;
    if ((st = specialize_generic(&map, C, B, s, ex, rows_overlap(din.data(), in_channels, L, dout.data(), C, Lr), &hold)))
        return st;
    TimedLaunch tl{};
    if ((st = timing_begin(s, &tl))) return st;
    st = render_device(din.data(), in_channels, L, dout.data(), C, B, map, 0, goff_of(ex), s);
    if (st) return st;
    {   // algorithmic bytes: file read (unless the map ignores its input) + render write
        uint64_t bytes = (uint64_t)C * Lr * 4;
        if (map.kind != MapKind::Ramp) bytes += (uint64_t)std::min(in_channels, C) * L * 4;
        if ((st = timing_end(s, &tl, bytes))) return st;
    }
    set_result(ex, by_class(orig.kind, map.kind) ? DSP_RESULT_CLASS : 0u);
    bool rerender = false;
    if ((st = verify_class_result(ex, orig, map, din.data(), in_channels, L, dout.data(), C, B, s, &rerender))) return st;
    if (rerender && (st = render_device(din.data(), in_channels, L, dout.data(), C, B, orig, 0, goff_of(ex), s)))
        return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

int dsp_render_loop(const float *const *in, uint32_t in_channels, uint64_t L, uint64_t cursor,
                    float *const *out, uint32_t C, uint32_t B, uint64_t nblocks, float sr,
                    const dsp_plugin *plugin, uint64_t *cursor_out, const dsp_exec *ex) {
    if (B == 0) return invalid("block size B must be > 0");
    if (in_channels && L == 0) return invalid("loop mode over an empty file (the reference spins forever, audio.cpp:104)");
    if (in_channels && cursor >= L) return invalid("cursor %llu past the file (L = %llu)", (unsigned long long)cursor,
                                                   (unsigned long long)L);
    if (cursor_out) *cursor_out = in_channels ? (uint64_t)((cursor + (unsigned __int128)nblocks * B) % L) : cursor;
    if (C == 0 || nblocks == 0) return DSP_OK;
    int st;
    if ((st = check_rows("out", out, C)) || (st = check_rows("in", in, in_channels))) return st;
    if (host_mode(ex)) return invalid("dsp_render_loop: device buffers only");
    if ((st = check_offset(ex, B))) return st;
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    const uint64_t Lr = nblocks * B;
    SpecHold hold;  // released after the call's launches
    SampleMap map;
    if ((st = plugin_map(plugin, B, g.dev, s, &map, sr, ex ? ex->flags : 0, &hold.table))) return st;
    // DSP_EXEC_VERIFY_CLASS: loop mode renders with the callback on every
    // block (as an in-place call does) rather than a class it would not check
    const bool verify = ex && (ex->flags & DSP_EXEC_VERIFY_CLASS);
    const MapKind before = map.kind;
    if ((st = specialize_generic(&map, C, B, s, ex, verify, &hold))) return st;
    set_result(ex, by_class(before, map.kind) ? DSP_RESULT_CLASS : 0u);
    if ((st = ensure_ramp_table(map, s))) return st;
    const uint32_t in_ch = std::min(in_channels, C);  // channels_to_write (audio.cpp:66)
    auto wrap = [&](const float *const *src, float *const *dst, uint32_t nc, const SampleMap &m) -> int {
        return for_groups(nc, [&](uint32_t c0, uint32_t cn) {
            RenderArgs A{};
            fill_rows(src, in_ch, dst, c0, cn, &A.in, &A.in_ch, &A.out);
            A.L = L;
            A.start = 0;
            A.end = Lr;
            A.map = group_map(m, c0);
            A.goff = goff_of(ex);
            return launch_render_wrap(A, cn, cursor, s);
        });
    };
    if (map.kind == MapKind::Noop || map.kind == MapKind::Gain || map.kind == MapKind::Ramp ||
        map.kind == MapKind::GainTable)
        return (st = wrap(in, out, C, map)) ? st : finish(ex);
    // FIR / CONV / GENERIC: the wrapped file is materialised (the plugin's block
    // stream), then rendered as a one-shot file of nblocks B samples
    float *tmp = nullptr;
    if (in_ch) {
        if ((st = get_scratch(g.dev, s, sizeof(float) * Lr * in_ch, &tmp, 1))) return st;
        std::vector<float *> rows(in_ch);
        for (uint32_t c = 0; c < in_ch; ++c) rows[c] = tmp + (uint64_t)c * Lr;
        SampleMap id{};
        id.kind = MapKind::Noop;
        id.B = B;
        if ((st = wrap(in, rows.data(), in_ch, id))) return st;
        std::vector<const float *> crow(rows.begin(), rows.end());
        st = render_device(crow.data(), in_ch, Lr, out, C, B, map, 0, goff_of(ex), s);
    } else {
        st = render_device(nullptr, 0, Lr, out, C, B, map, 0, goff_of(ex), s);
    }
    return st ? st : finish(ex);
}

int dsp_stft_magnitude(const float *const *in, uint32_t C, uint64_t L, uint32_t N, uint32_t H,
                       int32_t window, uint32_t K, float *const *mag, uint64_t ld,
                       const dsp_exec *ex) {
    int st = check_stft_args(N, H, K, ld, window);
    if (st) return st;
    if (C == 0) return DSP_OK;
    if (!in || !mag) return invalid("in / mag is NULL");
    for (uint32_t c = 0; c < C; ++c)
        if (!in[c] || !mag[c]) return invalid("in[%u] / mag[%u] is NULL", c, c);
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    const uint64_t F = dsp_stft_frame_count(L, N, H);
    Stage stage(ex);
    const std::vector<const float *> din = stage.in_rows(in, C, L);
    const std::vector<float *> dmag = stage.out_rows(mag, C, F * ld);  // (F == 0: nothing to copy back)
    if (stage.status) return stage.status;
    if ((st = stft_device(din.data(), C, L, N, H, window, K, dmag.data(), ld, g.dev, s))) return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

int dsp_render_stft(const float *const *in, uint32_t in_channels, uint64_t L,
                    float *const *out, uint32_t C, uint32_t B, float sr,
                    const dsp_plugin *plugin, uint32_t N, uint32_t H, int32_t window,
                    uint32_t K, float *const *mag, uint64_t ld, const dsp_exec *ex) {

    if (B == 0) return invalid("block size B must be > 0");
    int st = check_stft_args(N, H, K, ld, window);
    if (st) return st;
    if (C == 0) return DSP_OK;
    if (!out || !mag) return invalid("out / mag is NULL");
    for (uint32_t c = 0; c < C; ++c)
        if (!out[c] || !mag[c]) return invalid("out[%u] / mag[%u] is NULL", c, c);
    if ((st = check_rows("in", in, in_channels)) || (st = check_offset(ex, B))) return st;
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    const uint64_t nblocks = (L + B - 1) / B;
    const uint64_t Lr = nblocks * B;
    const uint64_t F = dsp_stft_frame_count(Lr, N, H);

    Stage stage(ex);
    const std::vector<const float *> din = stage.in_rows(in, in_channels, L);
    const std::vector<float *> dout = stage.out_rows(out, C, Lr);
    const std::vector<float *> dmag = stage.out_rows(mag, C, F * ld);  // (F == 0: nothing to copy back)
    if (stage.status) return stage.status;
    SpecHold hold;  // released after the call's launches
    SampleMap map;
    if ((st = plugin_map(plugin, B, g.dev, s, &map, sr, ex ? ex->flags : 0, &hold.table))) return st;
    const SampleMap orig = map;
    if ((st = specialize_generic(&map, C, B, s, ex, rows_overlap(din.data(), in_channels, L, dout.data(), C, Lr), &hold)))
        return st;
    const uint64_t goff = goff_of(ex);
    set_result(ex, by_class(orig.kind, map.kind) ? DSP_RESULT_CLASS : 0u);

    bool fused = (N == 8192) && (H % 128 == 0) && (H <= N) && (goff % 2 == 0) && F > 0 &&
                 map.kind != MapKind::Fir && map.kind != MapKind::Generic && map.kind != MapKind::Biquad &&
                 map.kind != MapKind::Conv;
    for (uint32_t c = 0; c < C; ++c) fused = fused && aligned(dout[c], 8);
    for (uint32_t c = 0; c < in_channels; ++c) fused = fused && aligned(din[c], 8);

    if (!fused && map.kind == MapKind::Generic) {
        // the plugin's own callback, then the STFT (generic_render_stft), timed
        // as one region: file read + render write + magnitude write
        TimedLaunch tl{};
        if ((st = timing_begin(s, &tl))) return st;
        tl_timing_outer = true;
        st = generic_render_stft(din.data(), in_channels, L, dout.data(), C, B, map, N, H, window, K, dmag.data(),
                                 ld, goff, g.dev, s);
        tl_timing_outer = false;
        if (st) return st;
        const uint64_t bytes = (uint64_t)std::min(in_channels, C) * L * 4 + (uint64_t)C * Lr * 4 +
                               (uint64_t)C * F * K * 4;
        if ((st = timing_end(s, &tl, bytes))) return st;
    } else if (!fused) {
        st = render_device(din.data(), in_channels, L, dout.data(), C, B, map, 0, goff, s);
        if (st) return st;
        st = stft_device(dout.data(), C, Lr, N, H, window, K, dmag.data(), ld, g.dev, s);
        if (st) return st;
    } else {
        const v2f *tw = nullptr;
        const float *win = nullptr;
        if ((st = get_tw(g.dev, s, &tw))) return st;
        if ((st = get_window(g.dev, s, window, N, N, &win, window_prescale(N)))) return st;
        bool tail_in_kernel = false, reused = false;
        st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
            Stft8kArgs A{};
            fill_rows(din.data(), in_channels, dout.data(), c0, cn, &A.in, &A.in_ch, &A.out);
            std::copy_n(dmag.data() + c0, cn, A.mag.p);
            A.L = L;
            if (int e = stft8k_args(&A, g.dev, s, tw, win, F, H, K, ld, N, window)) return e;
            A.map = group_map(map, c0);
            A.goff = goff;
            // the PER kernel also renders the tail no frame owns
            if (stft8192_pk_per_path(A, true)) A.tail_end = Lr, tail_in_kernel = true;
            // frame reuse (H % B == 0 on that path: one spectrum serves a run of
            // frames) unless the caller asks for every frame's own FFT; a call
            // that verifies a GENERIC plugin's class takes no shortcut that
            // rests on the class either
            const bool every_frame = ex && ((ex->flags & DSP_EXEC_EVERY_FRAME) ||
                                            (orig.kind == MapKind::Generic && (ex->flags & DSP_EXEC_VERIFY_CLASS)));
            A.run = every_frame ? 1u : stft8192_pk_frame_run(A, true, cn, g_frame_run.load());
            if (A.run > 1) reused = true;
            TimedLaunch tl{};
            if (int e = timing_begin(s, &tl)) return e;
            if (int e = launch_stft(A, cn, true, s)) return e;
            // algorithmic bytes: render write 4 B + magnitudes 4 K/H B
            // per hop sample, plus the file read when the map uses its input
            const uint64_t hop_samples = (uint64_t)cn * F * H;
            uint64_t bytes = hop_samples * 4 + (uint64_t)cn * F * K * 4;
            if (map.kind != MapKind::Ramp) bytes += (uint64_t)A.in_ch * F * H * 4;
            if (A.tail_end) bytes += (uint64_t)cn * (A.tail_end - F * (uint64_t)H) * 4;
            return timing_end(s, &tl, bytes);
        });
        if (st) return st;
        if (reused) or_result(ex, DSP_RESULT_FRAME_REUSE);
        // the render tail no frame owns: [F*H, Lr)
        if (!tail_in_kernel) {
            st = render_device(din.data(), in_channels, L, dout.data(), C, B, map, F * (uint64_t)H, goff, s);
            if (st) return st;
        }
    }
    bool rerender = false;
    if ((st = verify_class_result(ex, orig, map, din.data(), in_channels, L, dout.data(), C, B, s, &rerender))) return st;
    if (rerender && (st = generic_render_stft(din.data(), in_channels, L, dout.data(), C, B, orig, N, H, window, K,
                                              dmag.data(), ld, goff, g.dev, s)))
        return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

int dsp_ir_analysis(const dsp_plugin *plugin, uint32_t C, float sr, uint32_t ir_len,
                    float *const *ir_out, float *mag, const dsp_exec *ex) {
    if (C == 0 || ir_len == 0) return invalid("C and ir_len must be > 0");
    if (!is_pow2(ir_len) || 4ull * ir_len > 8192) return invalid("4*ir_len must be a power of two <= 8192");
    if (!ir_out || !mag) return invalid("ir_out / mag is NULL");
    int st;
    if ((st = check_rows("ir_out", ir_out, C))) return st;
    if (plugin && plugin->kind == DSP_PLUGIN_GENERIC && C > (uint32_t)kMaxChannels)
        return invalid("GENERIC plugin: IR analysis of 1..%d channels", kMaxChannels);
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    const uint32_t n = 4 * ir_len;
    Stage stage(ex);
    const std::vector<float *> dir = stage.out_rows(ir_out, C, ir_len);
    float *dmag = stage.out(mag, n);
    if (stage.status) return stage.status;
    // compute_IR (plugin.cpp:27-34): IR[c] = delta, then one callback of ir_len
    SampleMap map;
    DevTable table;  // held until the call's launches are enqueued
    if ((st = plugin_map(plugin, ir_len, g.dev, s, &map, sr, ex ? ex->flags : 0, &table))) return st;
    if (map.kind == MapKind::Generic) {  // the impulse in place, a fresh scratch State, one callback
        st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
            ChanOut imp{};
            std::copy_n(dir.data() + c0, cn, imp.p);
            return launch_impulse(imp, cn, ir_len, s);
        });
        if (st) return st;
        if ((st = module_ir((::dsp_module *)map.module, map.gparams, map.gparams_size, dir.data(), C, ir_len, sr, s)))
            return st;
    } else {  // map plugins: render the read-only impulse into IR[c], one launch
        const float *delta;
        if ((st = get_delta(g.dev, s, &delta))) return st;
        std::vector<const float *> cin(C, delta);
        if ((st = render_device(cin.data(), C, ir_len, dir.data(), C, ir_len, map, 0, 0, s))) return st;
    }

    // fft_perform_and_get_magnitude (dsp.cpp:53-66): channel 0 only
    const v2f *tw = nullptr;
    const float *win = nullptr;
    if ((st = get_tw(g.dev, s, &tw))) return st;
    const bool fast_ir = n == 8192 && aligned(dir[0], 8);
    if ((st = get_window(g.dev, s, DSP_WIN_HAMMING, n, ir_len, &win, fast_ir ? window_prescale(n) : 1.0)))
        return st;
    // one frame of ir_len samples, all n bins, as the reference stores them (dsp.cpp:65)
    if (fast_ir) {
        Stft8kArgs A{};
        A.in.p[0] = dir[0];
        A.in_ch = 1;
        A.L = ir_len;
        A.mag.p[0] = dmag;
        // (no computed window: its base angles would be one more first-use table)
        if ((st = stft8k_args(&A, g.dev, s, tw, win, 1, n, n, n, ir_len, -1))) return st;
        if ((st = launch_stft(A, 1, false, s))) return st;
    } else {
        GenericFftArgs A = fft_mag_args(tw, win, n, ir_len, 0, n, n);
        A.sig.p[0] = dir[0];
        A.mag.p[0] = dmag;
        if ((st = launch_fft_generic(A, 1, 1, s))) return st;
    }
    return (st = stage.copy_back()) ? st : finish(ex);
}

static int fft_service(const float *re_in, const float *im_in, float *re_out, float *im_out,
                       uint32_t n, int dir, const dsp_exec *ex) {
    if (!is_pow2(n) || n < 2 || n > 8192) return invalid("n=%u must be a power of two in [2, 8192]", n);
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    const v2f *tw = nullptr;
    int st = get_tw(g.dev, s, &tw);
    if (st) return st;
    Stage stage(ex);
    GenericFftArgs A = fft_args(tw, n, dir);
    A.re_in = stage.in(re_in, n);
    A.im_in = im_in ? stage.in(im_in, n) : nullptr;
    A.re_out = stage.out(re_out, n);
    A.im_out = im_out ? stage.out(im_out, n) : nullptr;
    A.mode = im_out ? 0 : 1;
    if (stage.status) return stage.status;
    if ((st = launch_fft_generic(A, 1, 1, s))) return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

int dsp_fft_forward(const float *in, float *re, float *im, uint32_t n, const dsp_exec *ex) {
    if (!in || !re || !im) return invalid("fft_forward: NULL buffer");
    return fft_service(in, nullptr, re, im, n, -1, ex);
}

int dsp_fft_reverse(const float *re, const float *im, float *out, uint32_t n, const dsp_exec *ex) {
    if (!re || !im || !out) return invalid("fft_reverse: NULL buffer");
    return fft_service(re, im, out, nullptr, n, +1, ex);
}

int dsp_gain(const float *in, float *out, float gain, uint64_t n, const dsp_exec *ex) {
    if (!in || !out) return invalid("NULL buffer");
    DeviceGuard g(ex);
    if (g.status) return g.status;
    int st = launch_gain(in, out, gain, n, stream_of(ex));
    return st ? st : finish(ex);
}

int dsp_copy(const float *in, float *out, uint64_t n, const dsp_exec *ex) {
    if (!in || !out) return invalid("NULL buffer");
    DeviceGuard g(ex);
    if (g.status) return g.status;
    bool done = false;
    if (!host_mode(ex)) {
        const int st = launch_copy(in, out, n, stream_of(ex), &done);
        if (st) return st;
    }
    if (!done) DSPB_HIP(hipMemcpyAsync(out, in, n * sizeof(float), hipMemcpyDeviceToDevice, stream_of(ex)));
    return finish(ex);
}

int dsp_set(float value, float *out, uint64_t n, const dsp_exec *ex) {
    if (!out) return invalid("NULL buffer");
    DeviceGuard g(ex);
    if (g.status) return g.status;
    // the runtime's 32-bit memset with the value's bit pattern: 6.5 TB/s
    // against 6.0 for the float4 kernel (profiles/r02_elementwise_bw.txt)
    if (!host_mode(ex) && n) {
        uint32_t bits;
        std::memcpy(&bits, &value, 4);
        DSPB_HIP(hipMemsetD32Async((hipDeviceptr_t)out, (int)bits, n, stream_of(ex)));
        return finish(ex);
    }
    int st = launch_set(value, out, n, stream_of(ex));
    return st ? st : finish(ex);
}

int dsp_magnitude(const float *re, const float *im, float *out, uint64_t n, const dsp_exec *ex) {
    if (!re || !im || !out) return invalid("NULL buffer");
    DeviceGuard g(ex);
    if (g.status) return g.status;
    int st = launch_magnitude(re, im, out, n, stream_of(ex));
    return st ? st : finish(ex);
}

// ---------------------------------------------------------------------------
// WAV payload decode / encode (wav.h)
// ---------------------------------------------------------------------------
static int wav_fmt_ok(uint16_t format, uint16_t bits) {
    return (format == DSP_WAV_FORMAT_PCM && (bits == 16 || bits == 24 || bits == 32)) ||
           (format == DSP_WAV_FORMAT_FLOAT && bits == 32);
}

int dsp_wav_decode(const void *payload, const dsp_wav_info *info, uint64_t frame0, uint64_t frames,
                   float *const *out, const dsp_exec *ex) {
    if (!info || !wav_fmt_ok(info->format, info->bits_per_sample)) return invalid("bad dsp_wav_info format");
    const uint32_t C = info->channels;
    if (C == 0 || C > (uint32_t)kMaxChannels) return invalid("channels must be 1..%d", kMaxChannels);
    if (frame0 > info->frames || frames > info->frames - frame0) return invalid("frame range past the payload");
    if (frames == 0) return DSP_OK;
    if (!payload || !out) return invalid("NULL buffer");
    int st;
    if ((st = check_rows("out", out, C))) return st;
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    const uint64_t ba = (uint64_t)C * (info->bits_per_sample / 8u);
    const uint8_t *src = (const uint8_t *)payload;
    uint64_t f0 = frame0;
    Stage stage(ex);
    if (stage.host) {  // only the frames of the call are staged
        src = (const uint8_t *)stage.in_bytes(src + frame0 * ba, frames * ba);
        f0 = 0;
    }
    ChanOut o{};
    bool al = true;
    for (uint32_t c = 0; c < C; ++c) {
        o.p[c] = stage.out(out[c], frames);
        al = al && aligned(o.p[c], 16);
    }
    if (stage.status) return stage.status;
    if ((st = launch_wav_decode(src, C, info->bits_per_sample, info->format == DSP_WAV_FORMAT_FLOAT, f0, frames, o,
                                al, s)))
        return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

int dsp_wav_encode(const float *const *in, uint32_t C, uint64_t frames, uint16_t format, uint16_t bits,
                   void *payload, const dsp_exec *ex) {
    if (!wav_fmt_ok(format, bits)) return invalid("unsupported WAV sample format");
    if (C == 0 || C > (uint32_t)kMaxChannels) return invalid("channels must be 1..%d", kMaxChannels);
    if (frames == 0) return DSP_OK;
    if (!in || !payload) return invalid("NULL buffer");
    int st;
    if ((st = check_rows("in", in, C))) return st;
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    Stage stage(ex);
    uint8_t *dst = (uint8_t *)stage.out_bytes(payload, frames * C * (bits / 8u));
    ChanOut i{};
    for (uint32_t c = 0; c < C; ++c) i.p[c] = const_cast<float *>(stage.in(in[c], frames));
    if (stage.status) return stage.status;
    if ((st = launch_wav_encode(dst, C, bits, format == DSP_WAV_FORMAT_FLOAT, frames, i, s))) return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

// ---------------------------------------------------------------------------
// display reductions
// ---------------------------------------------------------------------------
int dsp_minmax_decimate(const float *x, uint64_t n, uint32_t pixels, float *vmax, float *vmin,
                        const dsp_exec *ex) {
    if (pixels == 0) return DSP_OK;
    if (!vmax || !vmin || (n && !x)) return invalid("NULL buffer");
    if (pixels > (1u << 24) || n >= (1ull << 39)) return invalid("pixels <= 2^24 and n < 2^39");
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    Stage stage(ex);
    const float *dx = stage.in(x, n);
    float *dmax = stage.out(vmax, pixels), *dmin = stage.out(vmin, pixels);
    if (stage.status) return stage.status;
    int st = launch_minmax(dx, n, pixels, dmax, dmin, s);
    if (st) return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

int dsp_spectrogram_decimate(const float *mag, uint64_t F, uint32_t K, uint64_t ld, uint32_t pixels,
                             float *out, const dsp_exec *ex) {
    if (pixels == 0 || K == 0) return DSP_OK;
    if (!out || (F && !mag)) return invalid("NULL buffer");
    if (ld < K) return invalid("ld < K");
    if (pixels > (1u << 24) || F >= (1ull << 39)) return invalid("pixels <= 2^24 and F < 2^39");
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    Stage stage(ex);
    const float *dm = stage.in(mag, F ? (F - 1) * ld + K : 0);  // the last row ends at its K-th bin
    float *dout = stage.out(out, (uint64_t)pixels * K);
    if (stage.status) return stage.status;
    int st = launch_spectro(dm, F, K, ld, pixels, dout, s);
    if (st) return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

}  // extern "C"
