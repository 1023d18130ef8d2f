// capi.cpp -- the extern "C" boundary of libdspbench (include/dspbench/dspbench.h):
// what its five translation units share (capi_impl.hpp) and the small services.
//
// Owns the errors, the per-device constant tables (twiddles, windows: the
// analogue of the IPP FFT spec / plan cache of dsp.cpp:84-95 and
// IPP_FFT_Context, structs.h:170-178), the table caches, the per-stream
// scratch, the kernel timing and the debug hooks; the Plugin family is in
// capi_render.cpp, the Plugin-free row calls in capi_rate.cpp, capi_bigfft.cpp
// and capi_grid.cpp.  Fails loudly (negative status) on anything it cannot run on the GPU -- there is no CPU
// path here.
#include <cstdarg>

#include "capi_impl.hpp"
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

int invalid(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof g_last_error, fmt, ap);
    va_end(ap);
    return DSP_ERR_INVALID;
}

// ---------------------------------------------------------------------------
// per-device resources
// ---------------------------------------------------------------------------
DevTable dev_table(float *p, int dev) {
    return DevTable(p, [dev](float *q) {
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(dev);
        (void)hipDeviceSynchronize();
        (void)hipFree(q);
        if (prev >= 0) (void)hipSetDevice(prev);
    });
}

std::mutex g_mu;
// (never destroyed: its tables must not be freed after the HIP runtime's own
// teardown at process exit)
std::map<int, DeviceRes> &g_res = *new std::map<int, DeviceRes>;

int refuse_capture(hipStream_t s, const char *what) {
    if (capturing(s)) {
        set_last_error("stream capture: %s is created on first use; make one eager call of this shape on the "
                       "capturing stream first", what);
        return DSP_ERR_INVALID;
    }
    return DSP_OK;
}

int refuse_sync_under_capture(hipStream_t s, const char *text) {
    if (!capturing(s)) return DSP_OK;
    set_last_error("%s", text);
    return DSP_ERR_INVALID;
}

// Synchronous upload of a constant table (launch_upload: kernel arguments,
// not a copy -- see render.hip); the tables are shared by every stream of the
// device, so the upload completes before the first use.  (Callers check the
// caller's stream for capture first: refuse_capture.)
int upload_table(void *dst, const void *src, size_t bytes) {
    if (int st = launch_upload((float *)dst, (const float *)src, bytes / sizeof(float), nullptr)) return st;
    DSPB_HIP(hipStreamSynchronize(nullptr));
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

int get_tw(int dev, hipStream_t s, const v2f **out) {
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceRes &r = g_res[dev];
    if (int st = first_use_table(r.tw8192, s, "the FFT twiddle table", twiddle_table)) return st;
    *out = r.tw8192;
    return DSP_OK;
}

// compute_IR's impulse (plugin.cpp:27-34) as a read-only device buffer: the
// IR render of a map plugin reads it as its file, so no impulse launch
constexpr uint32_t kDeltaLen = 2048;  // the largest ir_len (4 ir_len <= 8192)
int get_delta(int dev, hipStream_t s, const float **out) {
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

int get_window(int dev, hipStream_t s, int kind, uint32_t N, uint32_t valid, const float **out, double scale) {
    std::lock_guard<std::mutex> lk(g_mu);
    float *&slot = g_res[dev].windows[std::make_tuple(kind, N, valid, (float)scale)];
    const int st = first_use_table(slot, s, "a window table", [&] {
        std::vector<float> h(N);
        window_table(kind, N, valid, scale, h.data());  // (host_tables.cpp)
        return h;
    });
    *out = slot;
    return st;
}

// Inputs of the computed-window kernels (stft_pk.hpp kOptWinComp): per-lane
// base angles and the (pre-scaled) cosine-window coefficients.
int set_wincomp(int dev, hipStream_t s, int kind, Stft8kArgs *A) {
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

int get_scratch(int dev, hipStream_t s, size_t bytes, float **out, ScratchSlot slot_id) {
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceRes &r = g_res[dev];
    auto &slot = r.scratch[std::make_pair((void *)s, (int)slot_id)];
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
// the spectrum rows of the fused IR_test STFT (capi_render.cpp)
// ---------------------------------------------------------------------------
// A retired row that nobody holds and no stream still reads leaves the list to
// serve again (g_mu held): its buffer and its events, all completed.  Rows are
// recycled, never freed -- hipFree would make the caller wait for the device --
// so a device holds kSpectrumRows of them plus what was in flight at once.
static std::shared_ptr<SpectrumRow> spectrum_recycle(DeviceRes &r) {
    for (size_t i = 0; i < r.spectrum_retired.size(); ++i) {
        auto &e = r.spectrum_retired[i];
        if (!spectrum_row_idle(*e, e.use_count(), [](hipEvent_t ev) { return hipEventQuery(ev) == hipSuccess; }))
            continue;
        std::shared_ptr<SpectrumRow> out = std::move(e);
        r.spectrum_retired.erase(r.spectrum_retired.begin() + (long)i);
        return out;
    }
    return nullptr;
}

int spectrum_row(int dev, hipStream_t s, const std::vector<uint64_t> &key,
                 const std::function<int(float *)> &compute, std::shared_ptr<SpectrumRow> *out) {
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceRes &r = g_res[dev];
    for (auto &e : r.spectrum)
        if (e->key == key) {
            // (the stream that computed the row too: a wait on an event of its own costs next to
            // nothing, and a stream handle does not identify a stream once streams are destroyed)
            // A completed ready event orders the row before every later launch on any stream:
            // once it has been seen so, hits enqueue no wait
            if (spectrum_row_must_wait(*e, [](hipEvent_t ev) { return hipEventQuery(ev) == hipSuccess; }))
                DSPB_HIP(hipStreamWaitEvent(s, e->ready, 0));
            *out = e;
            return DSP_OK;
        }
    std::shared_ptr<SpectrumRow> e = spectrum_recycle(r);
    if (!e) {
        e = std::make_shared<SpectrumRow>();
        DSPB_HIP(hipEventCreateWithFlags(&e->ready, hipEventDisableTiming));
        if (hipError_t err = hipMalloc(&e->row, sizeof(float) * kSpectrumRowFloats)) {
            (void)hipEventDestroy(e->ready);
            return hip_fail(err, "hipMalloc");
        }
    }
    e->key = key;
    e->ready_seen = false;
    // with g_mu held, so that a second call of this key finds the event recorded
    int st = compute(e->row);
    if (st == DSP_OK && hipEventRecord(e->ready, s) != hipSuccess) st = DSP_ERR_HIP;
    if (st) {  // the row serves a later miss
        r.spectrum_retired.push_back(e);
        return st;
    }
    if (r.spectrum.size() >= kSpectrumRows) {
        r.spectrum_retired.push_back(std::move(r.spectrum.front()));
        r.spectrum.erase(r.spectrum.begin());
    }
    r.spectrum.push_back(e);
    *out = e;
    return DSP_OK;
}

int spectrum_row_event(hipStream_t s, const std::shared_ptr<SpectrumRow> &e, hipEvent_t *out) {
    std::lock_guard<std::mutex> lk(g_mu);
    hipEvent_t &ev = e->used[(void *)s];
    if (!ev) DSPB_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    *out = ev;
    return DSP_OK;
}

int spectrum_row_used(hipStream_t s, const std::shared_ptr<SpectrumRow> &e) {
    hipEvent_t ev = nullptr;
    if (int st = spectrum_row_event(s, e, &ev)) return st;
    DSPB_HIP(hipEventRecord(ev, s));
    return DSP_OK;
}

// ---------------------------------------------------------------------------
// optional per-launch timing of the dominant kernel (HIP events on the
// launch stream), read back by dsp_kernel_timing(); used by bench.py
// ---------------------------------------------------------------------------
static bool g_timing = false;
// recycled timing events per device (g_mu): a hipEventCreate pair per timed
// launch cost more than the records themselves
static std::map<int, std::vector<hipEvent_t>> g_event_pool;

static std::vector<TimedLaunch> g_timed;
// (file-local: a thread-local that other files named would be reached through
// its hidden, undefined initialiser's address)
static thread_local bool tl_timing_outer = false;
void timing_outer(bool on) { tl_timing_outer = on; }

int timing_begin(hipStream_t s, TimedLaunch *t) {
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

int timing_end(hipStream_t s, TimedLaunch *t, uint64_t bytes) {
    if (!t->start) return DSP_OK;
    DSPB_HIP(hipEventRecord(t->stop, s));
    t->bytes = bytes;
    std::lock_guard<std::mutex> lk(g_mu);
    g_timed.push_back(*t);
    return DSP_OK;
}

// DSP_DEBUG_FRAME_RUN (stft8192_pk_frame_run) and DSP_DEBUG_BIQUAD_SPIN_LIMIT
// (capi_render.cpp iir_launch)
std::atomic<uint32_t> g_frame_run{0}, g_iir_spin_limit{kIirSpinLimit};
// DSP_DEBUG_SPECTRUM_CACHE, DSP_DEBUG_ROW_RUN and DSP_DEBUG_ROW_PACE (capi_render.cpp dsp_render_stft)
std::atomic<uint32_t> g_spectrum_cache{0}, g_row_run{0}, g_row_pace{0};
// DSP_DEBUG_PVOC_CHUNK and DSP_DEBUG_PVOC_VARIANT (capi_grid.cpp dsp_pvoc)
std::atomic<uint32_t> g_pvoc_chunk{0}, g_pvoc_variant{0};

// ---------------------------------------------------------------------------
// argument checks (before DeviceGuard: they need no device)
// ---------------------------------------------------------------------------
int check_rows(const char *name, const float *const *rows, uint32_t n) {
    if (n && !rows) return invalid("%s is NULL", name);
    for (uint32_t c = 0; c < n; ++c)
        if (!rows[c]) return invalid("%s[%u] is NULL", name, c);
    return DSP_OK;
}

int double_rows(const char *call, const char *name, double *const *rows, uint32_t C,
                std::vector<const float *> *out) {
    if (!rows) return invalid("%s is NULL", name);
    out->resize(C);
    for (uint32_t c = 0; c < C; ++c) {
        if (!rows[c]) return invalid("%s[%u] is NULL", name, c);
        if (!aligned(rows[c], 8)) return invalid("%s: %s[%u] is not 8-byte aligned", call, name, c);
        (*out)[c] = reinterpret_cast<const float *>(rows[c]);
    }
    return DSP_OK;
}

int whole_rows_only(const dsp_exec *ex, const char *call) {
    return goff_of(ex) != 0 ? invalid("%s: whole rows only (sample_offset 0)", call) : (int)DSP_OK;
}

int plan_status(int r, const char *why) {
    if (r == 0) return DSP_OK;
    set_last_error("%s", why);
    return r == 1 ? DSP_ERR_INVALID : DSP_ERR_UNSUPPORTED;
}

uint32_t fill_rows(const float *const *in, uint32_t in_channels, float *const *out, uint32_t c0, uint32_t cn,
                   ChanIn *src, uint32_t *in_ch, ChanOut *dst, size_t align) {
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

int finish(const dsp_exec *ex) {
    if (ex && (ex->flags & (DSP_EXEC_SYNC | DSP_EXEC_HOST_BUFFERS)))
        DSPB_HIP(hipStreamSynchronize(stream_of(ex)));
    return DSP_OK;
}

GenericFftArgs fft_args(const v2f *tw, uint32_t n, int dir) {
    GenericFftArgs A{};
    A.n = n;
    A.log2n = ilog2(n);
    A.dir = dir;
    A.tw = tw;
    A.scale = fft_scale(n);
    return A;
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
    if (what == DSP_DEBUG_SPECTRUM_CACHE) {
        if (value > 2) return invalid("dsp_debug_set: spectrum cache mode %llu > 2", (unsigned long long)value);
        g_spectrum_cache.store((uint32_t)value);
        return DSP_OK;
    }
    if (what == DSP_DEBUG_ROW_RUN) {
        if (value > 0xffffu) return invalid("dsp_debug_set: row run %llu > 65535", (unsigned long long)value);
        g_row_run.store((uint32_t)value);
        return DSP_OK;
    }
    if (what == DSP_DEBUG_ROW_PACE) {
        if (value && (value > 0xffffffffull || !row_pace_valid((uint32_t)value)))
            return invalid("dsp_debug_set: row pace 0x%llx is not nap (0..%u) | waves (%u..9) << 8 [| 1 << 16]",
                           (unsigned long long)value, kRowPaceMaxNap, kRowPaceMinWaves);
        g_row_pace.store((uint32_t)value);
        return DSP_OK;
    }
    if (what == DSP_DEBUG_PVOC_CHUNK) {
        if (value && (value < 8 || value > 4096)) return invalid("dsp_debug_set: pvoc chunk %llu is not 0 or 8..4096", (unsigned long long)value);
        g_pvoc_chunk.store((uint32_t)value);
        return DSP_OK;
    }
    if (what == DSP_DEBUG_PVOC_VARIANT) {
        if (value > 7) return invalid("dsp_debug_set: pvoc variant %llu > 7", (unsigned long long)value);
        g_pvoc_variant.store((uint32_t)value);
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
    if ((what == DSP_DEBUG_SPECTRUM_CACHE || what == DSP_DEBUG_ROW_RUN || what == DSP_DEBUG_ROW_PACE) && value) {
        *value = (what == DSP_DEBUG_ROW_RUN ? g_row_run : what == DSP_DEBUG_ROW_PACE ? g_row_pace : g_spectrum_cache).load();
        return DSP_OK;
    }
    if ((what == DSP_DEBUG_PVOC_CHUNK || what == DSP_DEBUG_PVOC_VARIANT) && value) {
        *value = (what == DSP_DEBUG_PVOC_CHUNK ? g_pvoc_chunk : g_pvoc_variant).load();
        return DSP_OK;
    }
    if (what != DSP_DEBUG_BIQUAD_REPAIRS || !value) return invalid("dsp_debug_get: unknown hook %d", what);
    int dev = 0;
    DSPB_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceRes &r = g_res[dev];
    *value = 0;
    if (r.iir_fb_host) {
        *value = __atomic_exchange_n(r.iir_fb_host, 0u, __ATOMIC_SEQ_CST);
    }
    return DSP_OK;
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
