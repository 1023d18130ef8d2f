// capi_impl.hpp -- what the C ABI's translation units share: capi.cpp (errors,
// per-device resources, the small services), capi_render.cpp (the Plugin
// family) and the Plugin-free row calls: capi_rate.cpp (rate and level),
// capi_bigfft.cpp (the large FFT) and capi_grid.cpp (the 8192-point grid).
// Everything here is internal to the library: hidden visibility.
#pragma once
#include "spectrum_rules.hpp"
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "host_hip.hpp"
#include "host_tables.hpp"
#include "kernels.hpp"

#pragma GCC visibility push(hidden)
namespace dspb {

int invalid(const char *fmt, ...);  // sets the error text; returns DSP_ERR_INVALID

// ---------------------------------------------------------------------------
// per-device resources (capi.cpp)
// ---------------------------------------------------------------------------
// A cached device table (FIR taps and spectra, BIQUAD transition powers):
// each call that maps it holds it until its launches are enqueued; the table
// is freed when the cache has evicted it and no call holds it, after the
// device has finished the work already enqueued
typedef std::shared_ptr<float> DevTable;
DevTable dev_table(float *p, int dev);

// what a cache entry carries beside its table
struct TablePayload {
    float h2048r = 0.f, h2048i = 0.f;  // FIR: H[2048] of the 8192-point spectrum
    uint32_t window = 0;               // BIQUAD: biquad_tables' W
};

// One entry of a keyed cache of device tables (cached_table): a FIR filter's
// taps + overlap-save spectra, keyed by the taps, or a biquad cascade's
// coefficients + state-transition powers (biquad_tables), keyed by the
// coefficients
struct CachedTable : TablePayload {
    std::vector<float> key;
    DevTable dev;
    size_t bytes = 0;  // of the device table
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

// One cached spectrum row of the fused IR_test STFT (spectrum_row): the 4097
// magnitudes every frame of a call with H % B == 0 has, computed once per key
// by the one-frame kernel.  The key is everything the row depends on.  A call
// holds the entry (the shared_ptr) while it enqueues; an evicted entry is
// retired, and its buffer serves a later miss once no call holds it and every
// stream that read it has passed the event of its last use.
struct SpectrumRow {
    std::vector<uint64_t> key;
    float *row = nullptr;              // kSpectrumRowFloats
    hipEvent_t ready = nullptr;        // after the launch that computed the row, on that launch's stream
    bool ready_seen = false;           // `ready` was seen completed: the row is there for every later launch
    std::map<void *, hipEvent_t> used;  // per stream: completes with its last launch that read the row
};
// (the rules of its events: spectrum_rules.hpp)
constexpr size_t kSpectrumRowFloats = 4100;  // 4097 bins, whole 16-byte pieces
constexpr size_t kSpectrumRows = 8;          // rows a device keeps

struct DeviceRes {
    v2f *tw8192 = nullptr;  // exp(-2 pi i k / 8192), then 896 lane-major stage twiddles
    float4 *wbase = nullptr;  // (cos, sin)(theta 2l), (cos, sin)(theta (2l+1)), theta = 2 pi / 8191
    std::map<std::tuple<int, uint32_t, uint32_t, float>, float *> windows;  // (kind, N, valid, scale)
    std::map<std::pair<void *, int>, std::pair<float *, size_t>> scratch;  // per (stream, slot)
    TableCache fir;                                            // FIR filters seen (plugin_map)
    TableCache iir;                                            // biquad cascades seen (plugin_map, dsp_loudness)
    TableCache conv;                                           // CONV impulse responses seen (plugin_map)
    TableCache resample;                                       // dsp_resample conversions seen (up, down, spec)
    TableCache limiter;                                        // dsp_limiter tables seen (rho, lookahead)
    TableCache rfft;                                           // dsp_rfft twiddle tables seen (n)
    std::vector<std::shared_ptr<SpectrumRow>> spectrum;        // fused IR_test spectrum rows seen, oldest first
    std::vector<std::shared_ptr<SpectrumRow>> spectrum_retired;  // evicted: for the next misses
    std::map<void *, IirWork> iir_work;                        // per stream
    uint32_t *iir_fb_host = nullptr, *iir_fb_dev = nullptr;  // host-mapped counter of repaired launches
    float *delta = nullptr;  // 2048 floats: 1, 0, 0, ... (compute_IR's impulse, read-only)
};

extern std::mutex g_mu;
extern std::map<int, DeviceRes> &g_res;

// A call on a stream that is being captured into a graph cannot make a
// first-use table or scratch allocation (an allocation, a legacy-stream
// launch and a sync would invalidate the capture): it is refused instead, and
// one eager call of the same shape beforehand creates what it needs.
int refuse_capture(hipStream_t s, const char *what);
// ... nor can a call that reads values back and synchronises its stream:
// refused with `text` while s is being captured
int refuse_sync_under_capture(hipStream_t s, const char *text);
// synchronous upload of a constant table (callers check the caller's stream for capture first)
int upload_table(void *dst, const void *src, size_t bytes);

// A constant device table made on first use, with g_mu held: `slot` if it is
// set already; else the host values from build(), uploaded to a fresh
// allocation.  `what` names the table in the capture refusal.
template <class T, class Build>
int first_use_table(T *&slot, hipStream_t s, const char *what, Build build) {
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

// device bytes of CONV or resampler tables a device keeps cached beside the
// newest one (a 2^20-tap table is 8.25 MiB)
constexpr size_t kConvCacheBytes = 64u << 20;

// The entry of `key` in a cache of at most 8 device tables -- and, with
// max_bytes set, of at most that many bytes of them beside the newest, the
// oldest leaving first -- with g_mu held.
// On a miss build(h, entry) fills the host table and the entry's payload; the
// table is uploaded once per key, not once per render.  The caller copies
// what it needs out of *out (the DevTable as its hold) before it unlocks.
template <class Build>
int cached_table(TableCache &cache, const std::vector<float> &key, int dev, hipStream_t s, const char *what,
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

// A call's hold on the cached table of `key` in the device's cache `which`
// (cached_table, under g_mu): *hold keeps the table until the call's launches
// are enqueued; *payload, when asked for, is the entry's.
template <class Build>
int hold_table(TableCache DeviceRes::*which, const std::vector<float> &key, int dev, hipStream_t s, const char *what,
               Build build, DevTable *hold, size_t max_bytes = 0, TablePayload *payload = nullptr) {
    std::lock_guard<std::mutex> lk(g_mu);
    const CachedTable *e = nullptr;
    if (int st = cached_table(g_res[dev].*which, key, dev, s, what, build, &e, max_bytes)) return st;
    *hold = e->dev;
    if (payload) *payload = *e;
    return DSP_OK;
}

int get_tw(int dev, hipStream_t s, const v2f **out);       // the 8192-point twiddles and stage twiddles
int get_delta(int dev, hipStream_t s, const float **out);  // compute_IR's impulse, kDeltaLen floats
// Window of length `valid` (symmetric, ref ippsWinHamming_32f convention)
// zero-padded to N.  Computed in double, rounded once to float.
int get_window(int dev, hipStream_t s, int kind, uint32_t N, uint32_t valid, const float **out, double scale = 1.0);
// inputs of the computed-window kernels (stft_pk.hpp kOptWinComp)
int set_wincomp(int dev, hipStream_t s, int kind, Stft8kArgs *A);

// stft8192_pk_kernel folds DIV_BY_SQRTN and the 1/2 of the real split into
// the window: 0.5 / sqrt(N)
inline float window_prescale(uint32_t N) { return (float)(0.5 / std::sqrt((double)N)); }
// DIV_BY_SQRTN (dsp.cpp:74-132): every transform scales by 1 / sqrt(n)
inline float fft_scale(uint32_t n) { return (float)(1.0 / std::sqrt((double)n)); }
GenericFftArgs fft_args(const v2f *tw, uint32_t n, int dir);

// Stream-ordered scratch: calls on one stream are serialised by the stream,
// so one buffer per (device, stream, user) is enough.
enum ScratchSlot : int {
    kScratchBlockTable = 0,  // the IR_test block table
    kScratchLoopFile = 1,    // loop mode's wrapped file
    kScratchConv = 2,        // a CONV channel group's spectra
    kScratchLoudness = 3,    // a dsp_loudness channel group's partial sums, hop energies and peaks
    kScratchLimiter = 4,     // a dsp_limiter call's hold rows, tile aggregates, carries and result words
    kScratchBigFft = 5,      // a dsp_rfft / dsp_irfft / dsp_deconvolve / dsp_decay group's work buffers, spectra and rows
    kScratchSpectrumHop = 6, // the hop the one-frame launch of a spectrum-row miss renders beside its row
    kScratchWelch = 7,       // a dsp_welch channel group's chunk of spectra and its runs' partial sums
    kScratchIstft = 8,       // a dsp_istft channel group's chunk of windowed inverse frames
    kScratchPvoc = 9,        // a dsp_pvoc channel group's chunk phase sums and carries
};
int get_scratch(int dev, hipStream_t s, size_t bytes, float **out, ScratchSlot slot);

// The cached spectrum row of `key` on `dev` for launches on s (not while s is
// being captured).  A miss takes a retired row or allocates one, runs
// compute(row) -- which enqueues on s the launch that fills it -- and records
// the entry's ready event; a hit makes s wait for that event unless the event
// has been seen completed.  *out holds the entry while the caller enqueues.
// The launch that reads the row on s completes the row's event of that stream,
// spectrum_row_event(): either as the launch's own completion event
// (launch_stft8192_rows' `done`) or by spectrum_row_used() after it.
int spectrum_row(int dev, hipStream_t s, const std::vector<uint64_t> &key,
                 const std::function<int(float *)> &compute, std::shared_ptr<SpectrumRow> *out);
int spectrum_row_event(hipStream_t s, const std::shared_ptr<SpectrumRow> &e, hipEvent_t *ev);
int spectrum_row_used(hipStream_t s, const std::shared_ptr<SpectrumRow> &e);

// ---------------------------------------------------------------------------
// optional per-launch timing of the dominant kernel (capi.cpp)
// ---------------------------------------------------------------------------
struct TimedLaunch {
    hipEvent_t start, stop;
    uint64_t bytes;
    int dev;
};
// on while a call (of this thread) times its launches as one region (the
// GENERIC render + STFT): the launches inside record nothing of their own
void timing_outer(bool on);
int timing_begin(hipStream_t s, TimedLaunch *t);
int timing_end(hipStream_t s, TimedLaunch *t, uint64_t bytes);

// the debug hooks' values (dsp_debug_set): frames per wave of the fused
// IR_test launch's frame reuse (0: the launch's own choice), and the sleeps a
// BIQUAD look-back waits before it gives up
constexpr uint32_t kIirSpinLimit = 1u << 16;
extern std::atomic<uint32_t> g_frame_run, g_iir_spin_limit;
// DSP_DEBUG_SPECTRUM_CACHE (0: the launch's own choice, 1: wherever it is
// valid, 2: never) and DSP_DEBUG_ROW_RUN (frames per wave of the store-only
// launch; 0: kRowRun), DSP_DEBUG_ROW_PACE (that launch's pacing; 0: kRowPace)
extern std::atomic<uint32_t> g_spectrum_cache, g_row_run, g_row_pace;
// DSP_DEBUG_PVOC_CHUNK (output frames per chunk of dsp_pvoc; 0: kPvocChunk) and
// DSP_DEBUG_PVOC_VARIANT (the A/B bits of pvoc.hip; 0: the product)
extern std::atomic<uint32_t> g_pvoc_chunk, g_pvoc_variant;

inline bool is_pow2(uint64_t n) { return n && !(n & (n - 1)); }
inline uint32_t ilog2(uint64_t n) { uint32_t l = 0; while ((1ull << l) < n) ++l; return l; }
inline bool aligned(const void *p, size_t a) { return ((uintptr_t)p % a) == 0; }

inline hipStream_t stream_of(const dsp_exec *ex) { return ex ? (hipStream_t)ex->stream : nullptr; }
inline bool host_mode(const dsp_exec *ex) { return ex && (ex->flags & DSP_EXEC_HOST_BUFFERS); }
inline uint64_t goff_of(const dsp_exec *ex) { return ex ? ex->sample_offset : 0; }

// ---------------------------------------------------------------------------
// argument checks (before DeviceGuard: they need no device)
// ---------------------------------------------------------------------------
int check_rows(const char *name, const float *const *rows, uint32_t n);
// float64 output rows (dsp_welch, dsp_decay): none NULL, each 8-byte aligned; *out = the rows as float rows
int double_rows(const char *call, const char *name, double *const *rows, uint32_t C, std::vector<const float *> *out);
// "<call>: whole rows only (sample_offset 0)"
int whole_rows_only(const dsp_exec *ex, const char *call);
// a host plan's (0 | 1 | 2, why) as DSP_OK | DSP_ERR_INVALID | DSP_ERR_UNSUPPORTED and the error text
int plan_status(int r, const char *why);
// ... of plan(args..., &why)
template <class Plan, class... A>
int plan_checked(Plan plan, A &&...a) {
    const char *why = nullptr;
    const int r = plan(std::forward<A>(a)..., &why);
    return plan_status(r, why);
}
// dsp_resample_plan's checks and the library's ResamplePlan (NULL spec: the defaults; capi_rate.cpp)
int resample_plan_checked(uint32_t sr_in, uint32_t sr_out, uint64_t L, const dsp_resample_spec *spec,
                          ResamplePlan *plan);

// ---------------------------------------------------------------------------
// host-buffer staging (DSP_EXEC_HOST_BUFFERS), one Stage per call.  Device
// mode: in() / out() hand the caller's pointer back.  Host mode: a device
// buffer each (freed when the call returns), the input copied on the call's
// stream, the outputs copied back by copy_back(); finish() then synchronises.
// The first failure sticks in `status` (checked once after the call's in() /
// out()s); zero-length buffers are one float and are not copied.
// Framed rows (dsp_stft, dsp_pvoc: `frames` frames of `dense` floats, `ld`
// floats apart): the device row of a host row is dense -- the launch's leading
// dimension is framed_ld() -- and copy_back() copies it out frame by frame, so
// that the floats [dense, ld) of a frame stay the caller's.
// ---------------------------------------------------------------------------
struct Stage {
    const bool host;
    const hipStream_t s;
    int status = DSP_OK;
    // pitch 0: `bytes` in one piece; else `frames` pieces of `bytes`, `pitch` bytes apart at the host
    struct Back { void *host; const void *dev; size_t bytes, pitch, frames; };
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
        if ((status = alloc(bytes, &d)) == DSP_OK) back.push_back(Back{p, d, bytes, 0, 1});
        return d;
    }
    uint64_t framed_ld(uint64_t dense, uint64_t ld) const { return host ? dense : ld; }
    std::vector<float *> out_framed_rows(float *const *rows, uint32_t C, uint64_t frames, uint64_t dense, uint64_t ld) {
        std::vector<float *> d(C);
        for (uint32_t c = 0; c < C; ++c) {
            void *p = rows[c];
            if (host && (status = alloc(sizeof(float) * frames * dense, &p)) == DSP_OK)
                back.push_back(Back{rows[c], p, dense * sizeof(float), ld * sizeof(float), frames});
            d[c] = (float *)p;
        }
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
        for (const Back &b : back) {
            if (b.pitch)
                DSPB_HIP(hipMemcpy2DAsync(b.host, b.pitch, b.dev, b.bytes, b.bytes, b.frames, hipMemcpyDeviceToHost, s));
            else if (int st = copy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost)) return st;
        }
        return DSP_OK;
    }
};

// DSP_EXEC_SYNC / DSP_EXEC_HOST_BUFFERS: the call returns when its stream has finished
int finish(const dsp_exec *ex);

// A row call's device context: its device made current until it returns, its
// stream and its staging.  `status` is the device's, tested once after
// construction; done() is the call's ending, the outputs copied back and finish().
struct RowCall {
    const dsp_exec *const ex;
    const DeviceGuard guard;
    const int status, dev;
    const hipStream_t s;
    Stage stage;
    explicit RowCall(const dsp_exec *ex) : ex(ex), guard(ex), status(guard.status), dev(guard.dev), s(stream_of(ex)), stage(ex) {}
    int done() { const int st = stage.copy_back(); return st ? st : finish(ex); }
};

// ---------------------------------------------------------------------------
// channel groups: a kernel takes at most kMaxChannels row pointers
// ---------------------------------------------------------------------------
// f(c0, cn) for rows [c0, c0 + cn) of C, group after group; the first error ends the walk
template <class F>
int for_groups(uint32_t C, F f) {
    for (uint32_t c0 = 0; c0 < C; c0 += kMaxChannels) {
        if (int st = f(c0, std::min<uint32_t>(C - c0, kMaxChannels))) return st;
    }
    return DSP_OK;
}

// A group's rows split for the kernels that run two channels per wavefront:
// f(first, count, 2) for its even run of pairs (when `pairs`), then
// f(first, count, 1) for what is left -- the odd last channel, or every row
template <class F>
int for_pairs_then_rest(uint32_t cn, bool pairs, F f) {
    const uint32_t np = pairs ? cn & ~1u : 0;  // (kMaxChannels is even)
    if (np)
        if (int st = f(0u, np, 2u)) return st;
    return cn > np ? f(np, cn - np, 1u) : DSP_OK;
}

// Rows [c0, c0 + cn) of a call as a launch's pointer tables: every output
// row, and the input rows the file has (*in_ch: one past the last of them).
// Returns which of the pointers it touched are all `align`-byte aligned.
enum : uint32_t { kOutAligned = 1, kInAligned = 2, kAllAligned = 3 };
uint32_t fill_rows(const float *const *in, uint32_t in_channels, float *const *out, uint32_t c0, uint32_t cn,
                   ChanIn *src, uint32_t *in_ch, ChanOut *dst, size_t align = 4);

// Rows [c0, c0 + cn) of one staged table (Stage::in_rows / out_rows) as a
// launch's pointer table; whether all of them are `align`-byte aligned.
template <class P, class Chan>
bool group_rows(const std::vector<P> &rows, uint32_t c0, uint32_t cn, Chan *dst, size_t align) {
    bool al = true;
    for (uint32_t j = 0; j < cn; ++j) {
        dst->p[j] = rows[c0 + j];
        al = al && aligned(rows[c0 + j], align);
    }
    return al;
}

}  // namespace dspb
#pragma GCC visibility pop
