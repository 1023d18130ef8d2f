// capi_render.cpp -- the Plugin family of the C ABI (include/dspbench/dspbench.h):
// maps a dsp_plugin onto a kernel (plugin_map, specialize_generic), renders
// and analyses on the caller's stream (render_device, stft_device), and the
// extern "C" calls built on them: dsp_render_*, dsp_stft_magnitude,
// dsp_ir_analysis, dsp_biquad_plan, dsp_conv_plan.  What it shares with
// the C ABI's other files is in capi_impl.hpp.
#include "capi_impl.hpp"

namespace dspb {

// a closed-form IR ramp (plugin_map) leaves the block table unbuilt; every
// fused path but stft_pk's PER path reads it
static int ensure_ramp_table(const SampleMap &m, hipStream_t s) {
    if (m.kind != MapKind::Ramp || m.closed != 1) return DSP_OK;  // 2: the table holds it already
    return launch_ramp_table(const_cast<float *>(m.table), m.B, (float)m.rg0, (float)m.rs, s);
}

static int launch_stft(const Stft8kArgs &A, uint32_t C, bool fused, hipStream_t s) {
    if (fused && !(A.map.closed && stft8192_pk_per_path(A, fused))) {
        const int st = ensure_ramp_table(A.map, s);
        if (st) return st;
    }
    // (the A/B and ablation options: 0 but in the tools build, whose stft_pk_ab.hip sets them per thread)
    return launch_stft8192_pk(A, C, fused, stft_pk_ab_options(), s);
}

// frames per wave of the store-only launch of a cached spectrum row
// (stft8192_rows_kernel).  Measured at 1, 2 and 4 (profiles/r09_spectrum_cache_ab.txt):
// with no FFT to share, the shortest run is the fastest -- 1 is 5% ahead of
// the reuse launch, 2 level with it, 4 behind it
constexpr uint32_t kRowRun = 1;
// ... and its pacing (launch_stft8192_rows): sleep units between a wave's hop
// burst and its row burst | the waves a CU holds << 8.  Measured in
// profiles/r10_rows_pacing_ab.txt: 6 waves are 3.5% ahead of the 9 the kernel's
// LDS tile allows (4 and 5 level with 6, 3 far behind); no sleep beats none in
// the kernel, though one did in the probe (r10_rows_pacing_probe.txt).
// kRowPaceRecord on top (DSP_DEBUG_ROW_PACE only) records the row's lifetime
// event after the launch, as a packet of its own, for the A/B of the launch's
// own completion event.
constexpr uint32_t kRowPace = 0u | 6u << 8;

// The device's cached spectrum row for the fused launch A (PER path, H % B ==
// 0: every frame has the samples of frame 0) on s, not under capture.  The key
// is what the row depends on: the block (a ramp's two parameters and whether
// the kernel evaluates or loads it), B, the sample phase goff mod B, the
// window's kind and pre-scaled coefficients, N and K.  A miss runs the
// one-frame kernel on one frame of one channel -- its row is the cache's, its
// hop goes to the stream's scratch -- so the row is what that kernel stores.
static int cached_spectrum_row(const Stft8kArgs &A, int32_t window, int dev, hipStream_t s,
                               std::shared_ptr<SpectrumRow> *row) {
    auto bits = [](auto v) {
        uint64_t u = 0;
        std::memcpy(&u, &v, sizeof v);
        return u;
    };
    const std::vector<uint64_t> key{A.map.closed, bits(A.map.rg0), bits(A.map.rs), A.map.B, A.goff % A.map.B,
                                    (uint64_t)(uint32_t)window, bits(A.wa), bits(A.wb), 8192u, A.K};
    float *hop = nullptr;
    if (int st = get_scratch(dev, s, sizeof(float) * A.H, &hop, kScratchSpectrumHop)) return st;
    return spectrum_row(dev, s, key, [&](float *dst) {
        Stft8kArgs A1 = A;
        A1.in_ch = 0;
        A1.out.p[0] = hop;
        A1.mag.p[0] = dst;
        A1.F = 1;
        A1.ld = A.K;
        A1.tail_end = 0;
        A1.run = 1;
        return launch_stft8192_pk(A1, 1, true, 0, s);
    }, row);
}

// ---------------------------------------------------------------------------
// plugin -> sample map
// ---------------------------------------------------------------------------
// takes the stream's workspace for one launch (a fresh epoch) and launches,
// under one lock: launches on a stream are enqueued in epoch order.
// spin_limit: the sleeps a look-back waits for a predecessor's words before it
// gives up (a legitimate wait is a few rounds: a tile waits only for waves
// dispatched before it); the launch is then rendered again serially
// (iir.hip biquad_repair_kernel, on the same stream)
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

// *table: a hold on the call's cached device table (FIR / BIQUAD), kept by
// the caller until the call's launches are enqueued
static int plugin_map(const dsp_plugin *p, uint32_t B, int dev, hipStream_t s, SampleMap *m, float sr,
                      uint32_t flags, DevTable *table) {
    *m = SampleMap{};  // (Noop; every field a kind does not set is zero)
    m->fir_direct = (flags & DSP_EXEC_FIR_DIRECT) ? 1u : 0u;
    m->a = 1.f;
    m->B = B;
    m->b_mask = is_pow2(B) ? B - 1 : 0;
    m->sr = sr;
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
        int st = get_scratch(dev, s, sizeof(float) * B, &table, kScratchBlockTable);
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
        TablePayload pl;
        const int st = hold_table(&DeviceRes::fir, key, dev, s, "a FIR filter's device taps",
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
        }, table, 0, &pl);
        if (st) return st;
        float *tp = table->get();
        m->kind = MapKind::Fir;
        m->taps = tp;
        m->ntaps8 = T8;
        m->ntaps = T;
        m->olsH = tp + T8;
        m->pairH = tp + T8 + 8196;  // 16-byte aligned: T8 and 8196 are multiples of 4
        m->olsH2048[0] = pl.h2048r;
        m->olsH2048[1] = pl.h2048i;
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
        const int st = hold_table(&DeviceRes::conv, key, dev, s, "a CONV impulse response's partition spectra",
                                  [&](std::vector<float> &h, CachedTable &) {
            h.assign((size_t)parts * 4 * kConvSpec4, 0.f);
            conv_table(key.data(), T, h.data());
        }, table, kConvCacheBytes);
        if (st) return st;
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
        TablePayload pl;
        const int st = hold_table(&DeviceRes::iir, key, dev, s, "a BIQUAD cascade's state-transition tables",
                                  [&](std::vector<float> &h, CachedTable &e) {
            e.window = biquad_tables(key.data(), S, biquad_lane_samples(), h);
        }, table, 0, &pl);
        if (st) return st;
        m->kind = MapKind::Biquad;
        m->iir_tab = table->get();
        m->sections = S;
        m->iir_window = pl.window;
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

static int check_offset(const dsp_exec *ex, uint32_t B) {
    if (ex && ex->sample_offset % B) return invalid("sample_offset must be a multiple of B");
    return DSP_OK;
}

// a group's view of the call's map: a GainTable's rows start at the group's
// first channel (module_specialize refuses C > kMaxChannels, so c0 is 0 today)
static SampleMap group_map(const SampleMap &m, uint32_t c0) {
    SampleMap g = m;
    if (m.kind == MapKind::GainTable) g.table += (uint64_t)c0 * m.B;
    return g;
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
        if (rows_overlap(Rows{in, std::min(in_ch, C), L}, Rows{out, C, end}))
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
        if (int st = get_scratch(dev, s, scratch_bytes, &scratch, kScratchConv)) return st;
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

extern "C" {

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
    if ((st = specialize_generic(&map, C, B, s, ex, rows_overlap(Rows{din.data(), in_channels, L}, Rows{dout.data(), C, Lr}), &hold)))
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
        if ((st = get_scratch(g.dev, s, sizeof(float) * Lr * in_ch, &tmp, kScratchLoopFile))) return st;
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
    if ((st = specialize_generic(&map, C, B, s, ex, rows_overlap(Rows{din.data(), in_channels, L}, Rows{dout.data(), C, Lr}), &hold)))
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
        timing_outer(true);
        st = generic_render_stft(din.data(), in_channels, L, dout.data(), C, B, map, N, H, window, K, dmag.data(),
                                 ld, goff, g.dev, s);
        timing_outer(false);
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
        bool tail_in_kernel = false, reused = false, cached = false;
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
            const uint32_t forced_run = g_frame_run.load();
            A.run = every_frame ? 1u : stft8192_pk_frame_run(A, true, cn, forced_run);
            // ... and outside stream capture that one spectrum is the device's
            // cached row of this block, phase and window (spectrum_row), which
            // the launch only stores.  The row's key is the block's content:
            // a ramp (closed form or IR_RAMP's own table) is its two
            // parameters; a GENERIC plugin's table without a closed form has
            // no content the host knows, and keeps the reuse launch.  Calls too
            // short for frame reuse keep one frame per wave, and a forced
            // DSP_DEBUG_FRAME_RUN keeps the reuse launch it asks for
            const uint32_t mode = g_spectrum_cache.load();
            const bool keyed = map.closed != 0 || orig.kind == MapKind::Ramp;
            const bool row_path = !every_frame && !(ex && (ex->flags & DSP_EXEC_VERIFY_CLASS)) && mode != 2 && keyed &&
                                  stft8192_pk_frame_run(A, true, cn, 2) == 2 &&  // (a forced run: wherever reuse is valid)
                                  !capturing(s) &&
                                  stft_pk_ab_options() == 0 &&  // (the tools build's variants are of the reuse launch)
                                  (mode == 1 || (forced_run == 0 && A.run > 1));
            std::shared_ptr<SpectrumRow> row;
            if (row_path) {
                if (int e = cached_spectrum_row(A, window, g.dev, s, &row)) return e;
                A.run = g_row_run.load() ? g_row_run.load() : kRowRun;
                cached = true;
            }
            if (A.run > 1 || row) reused = true;
            TimedLaunch tl{};
            if (int e = timing_begin(s, &tl)) return e;
            const uint32_t pace = g_row_pace.load() ? g_row_pace.load() : kRowPace;
            hipEvent_t row_done = nullptr;  // the row's lifetime event of this stream: completes with the launch
            if (row && !(pace & kRowPaceRecord))
                if (int e = spectrum_row_event(s, row, &row_done)) return e;
            if (int e = row ? launch_stft8192_rows(A, cn, row->row, pace, row_done, s) : launch_stft(A, cn, true, s))
                return e;
            // algorithmic bytes: render write 4 B + magnitudes 4 K/H B
            // per hop sample, plus the file read when the map uses its input
            const uint64_t hop_samples = (uint64_t)cn * F * H;
            uint64_t bytes = hop_samples * 4 + (uint64_t)cn * F * K * 4;
            if (map.kind != MapKind::Ramp) bytes += (uint64_t)A.in_ch * F * H * 4;
            if (A.tail_end) bytes += (uint64_t)cn * (A.tail_end - F * (uint64_t)H) * 4;
            if (int e = timing_end(s, &tl, bytes)) return e;
            return row && !row_done ? spectrum_row_used(s, row) : (int)DSP_OK;
        });
        if (st) return st;
        if (reused) or_result(ex, DSP_RESULT_FRAME_REUSE);
        if (cached) or_result(ex, DSP_RESULT_SPECTRUM_CACHE);
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

}  // extern "C"
