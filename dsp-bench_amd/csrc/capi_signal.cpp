// capi_signal.cpp -- the Plugin-free row calls of the C ABI
// (include/dspbench/dspbench.h): dsp_resample, dsp_loudness, dsp_limiter,
// dsp_rfft / dsp_irfft, dsp_deconvolve, dsp_sweep, dsp_welch, dsp_stft / dsp_istft,
// dsp_pvoc / dsp_time_stretch and dsp_decay, with
// their plans.  Each checks its arguments and its rows' layout before it looks at a
// device, holds its cached tables until its launches are enqueued, and walks
// its channels in groups of kMaxChannels.  What it shares with capi.cpp and
// capi_render.cpp is in capi_impl.hpp.
#include "capi_impl.hpp"
#include "decay_host.hpp"
#include "limiter_host.hpp"
#include "loudness_host.hpp"
#include "pvoc_host.hpp"
#include "stft_cx_host.hpp"
#include "sweep_host.hpp"
#include "welch_host.hpp"

namespace dspb {

// dsp_resample_plan's checks and the library's ResamplePlan (NULL spec: the defaults)
static int resample_plan_checked(uint32_t sr_in, uint32_t sr_out, uint64_t L, const dsp_resample_spec *spec,
                                 ResamplePlan *plan) {
    const dsp_resample_spec def{64u, 14.769656459379492, 0.9475937167399596};
    if (!spec) spec = &def;
    const char *why = nullptr;
    const int r = resample_plan(sr_in, sr_out, L, spec->zeros, spec->beta, spec->rolloff, plan, &why);
    return plan_status(r, why);
}

// a conversion's launch arguments but for its rows and table: the plan and its blocking (resample.hip)
static ResampleArgs resample_args(const ResamplePlan &p, uint64_t L) {
    ResampleArgs A{};
    A.L = L;
    A.Lout = p.Lout;
    A.up = p.up;
    A.down = p.down;
    A.half = p.half;
    A.Tp = p.taps;
    resample_blocking(&A);
    return A;
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
    return hold_table(&DeviceRes::resample, key, dev, s, "a sample-rate conversion's filter table",
                      [&](std::vector<float> &h, CachedTable &) {
        std::vector<float> plain((size_t)p.up * p.taps);
        resample_table(p, plain.data(), p.taps, 0);
        h.resize(resample_device_floats(A));
        resample_device_table(A, plain.data(), h.data());
    }, table, kConvCacheBytes);
}

// The true-peak detector's table (dsp_loudness, dsp_limiter): dsp_resample's
// cached device table for sr -> ovs sr, whose blocking must be one group of ovs
// phases with coinciding windows, table[step][phase], R->S steps
static int oversampler_table(const ResamplePlan &rp, uint64_t L, uint32_t ovs, int dev, hipStream_t s,
                             ResampleArgs *R, DevTable *table) {
    *R = resample_args(rp, L);
    if (!R->phase || R->R != ovs || R->S != ((rp.taps + 3) & ~3u)) {
        set_last_error("unexpected blocking of the oversampling filter");
        return DSP_ERR_UNSUPPORTED;
    }
    return resample_cached_table(rp, *R, dev, s, table);
}

static int loudness_plan_checked(uint32_t sr, uint64_t L, LoudnessPlan *p) {
    const char *why = nullptr;
    const int r = loudness_plan(sr, L, p, &why);
    return plan_status(r ? 2 : 0, why);  // (the rate or the length is out of range: unsupported)
}

// dsp_limiter_plan's checks: the limiter's own, then (TRUE_PEAK at ovs > 1) the oversampler's
static int limiter_plan_checked(uint32_t sr, uint64_t L, uint32_t C, const dsp_limiter_spec *spec,
                                const dsp_resample_spec *tp_spec, LimiterPlan *p, ResamplePlan *rp) {
    const char *why = nullptr;
    const int r = limiter_plan(sr, L, C, spec, p, &why);
    if (r) return plan_status(r, why);
    if (spec->flags & DSP_LIMITER_TRUE_PEAK) return resample_plan_checked(sr, sr * p->oversample, L, tp_spec, rp);
    return DSP_OK;
}

static int sweep_plan_checked(uint32_t sr, const dsp_sweep_spec *spec, SweepPlan *p) {
    const char *why = nullptr;
    const int r = sweep_plan(sr, spec, p, &why);
    return plan_status(r ? 1 : 0, why);  // (every refusal is the spec's: invalid)
}

static_assert(kWelchGroup == kMaxChannels, "welch_plan sizes the scratch for for_groups' channel groups");
static int welch_plan_checked(uint64_t L, uint32_t C, int has_ref, const dsp_welch_spec *spec, WelchPlan *p) {
    const char *why = nullptr;
    const int r = welch_plan(L, C, has_ref, spec, p, &why);
    return plan_status(r, why);
}

static_assert(kStftCxGroup == kMaxChannels, "istft_plan sizes the scratch for for_groups' channel groups");
static_assert(kPvocGroup == kMaxChannels, "pvoc_plan sizes the scratch for for_groups' channel groups");
// spectrum rows (dsp_stft's outputs, dsp_istft's inputs, both of dsp_pvoc's): none NULL, each 8-byte aligned
static int spectrum_rows(const char *call, const float *const *rows, uint32_t C) {
    if (int st = check_rows("spec", rows, C)) return st;
    for (uint32_t c = 0; c < C; ++c)
        if (!aligned(rows[c], 8)) return invalid("%s: spec[%u] is not 8-byte aligned", call, c);
    return DSP_OK;
}

// float64 output rows (dsp_welch, dsp_decay): none NULL, each 8-byte aligned; *out = the rows as float rows
static int double_rows(const char *call, const char *name, double *const *rows, uint32_t C,
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

static_assert(kDecayGroup == kMaxChannels, "decay_plan sizes the scratch for launches of kMaxChannels rows");
static int decay_plan_checked(uint64_t L, uint32_t C, uint32_t sr, const dsp_decay_spec *spec, DecayPlan *p) {
    const char *why = nullptr;
    const int r = decay_plan(L, C, sr, spec, p, &why);
    return plan_status(r, why);
}

// A call's large-FFT context (fft_big.hip): the hold on n's cached twiddle
// table, and the stream's work buffers and spectra
namespace {
struct BigFft {
    uint32_t n = 0;
    DevTable table;  // held until the call's launches are enqueued
    float *work = nullptr;
};
}  // namespace

static int big_fft_open(uint32_t n, size_t scratch_bytes, int dev, hipStream_t s, BigFft *f) {
    f->n = n;
    const std::vector<float> key{(float)n};  // (a power of two: exact)
    if (int st = hold_table(&DeviceRes::rfft, key, dev, s, "the large FFT's twiddle table",
                            [&](std::vector<float> &h, CachedTable &) { rfft_twiddles(n, h); }, &f->table))
        return st;
    return get_scratch(dev, s, scratch_bytes, &f->work, kScratchBigFft);
}

// a launch's plan, table and the work buffers of `nch` channels
static int big_fft_args(const BigFft &f, uint32_t nch, BigFftArgs *A) {
    A->n = f.n;
    A->nch = nch;
    if (!rfft_plan(f.n, &A->passes, A->radix)) return DSP_ERR_INVALID;
    A->tw = reinterpret_cast<const v2f *>(f.table.get());
    A->buf0 = reinterpret_cast<v2f *>(f.work);
    A->buf1 = A->buf0 + (uint64_t)nch * (f.n / 2);
    A->in_aligned8 = A->out_aligned8 = 1;
    return DSP_OK;
}

// dsp_rfft (rows of Lin samples -> spectra of Lout = n + 2 floats) and
// dsp_irfft (spectra of Lin = n + 2 floats -> rows of Lout samples) after
// their argument checks: the rows' layout, then the transforms.  Lin = 0
// (dsp_rfft of no samples): `in` is not looked at and nothing reads it.
static int big_fft_rows(bool inverse, const float *const *in, uint64_t Lin, uint32_t C, uint32_t n, float *const *out,
                        uint64_t Lout, const char *overlap_text, const dsp_exec *ex) {
    if (rows_overlap(Rows{in, C, Lin}, Rows{out, C, Lout}) || rows_overlap_each_other(Rows{out, C, Lout}))
        return invalid("%s", overlap_text);
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    Stage stage(ex);
    const std::vector<float *> dout = stage.out_rows(out, C, Lout);
    std::vector<const float *> din(C);
    for (uint32_t c = 0; c < C; ++c) din[c] = Lin ? stage.in(in[c], Lin) : dout[c];
    if (stage.status) return stage.status;
    int st;
    BigFft f;
    if ((st = big_fft_open(n, std::min<uint32_t>(C, kMaxChannels) * rfft_scratch_bytes(n), g.dev, s, &f))) return st;
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        BigFftArgs A{};
        if (int e = big_fft_args(f, cn, &A)) return e;
        if (inverse) A.Lout = Lout;
        else A.L = Lin;
        A.in_aligned8 = group_rows(din, c0, cn, &A.in, 8);
        A.out_aligned8 = group_rows(dout, c0, cn, &A.out, 8);
        return inverse ? launch_big_irfft(A, s) : launch_big_rfft(A, s);
    });
    if (st) return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

}  // namespace dspb

using namespace dspb;

extern "C" {

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

int dsp_resample(const float *const *in, uint32_t C, uint64_t L, float *const *out, uint64_t Lout, uint32_t sr_in,
                 uint32_t sr_out, const dsp_resample_spec *spec, const dsp_exec *ex) {
    ResamplePlan p;
    int st;
    if ((st = resample_plan_checked(sr_in, sr_out, L, spec, &p))) return st;
    if (Lout != p.Lout)
        return invalid("dsp_resample: Lout %llu != the plan's %llu", (unsigned long long)Lout,
                       (unsigned long long)p.Lout);
    if ((st = whole_rows_only(ex, "dsp_resample"))) return st;
    if (C == 0 || L == 0) return DSP_OK;
    if ((st = check_rows("out", out, C)) || (st = check_rows("in", in, C))) return st;
    if (rows_overlap(Rows{in, C, L}, Rows{out, C, Lout})) return invalid("dsp_resample: output rows overlap input rows");
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
    ResampleArgs A = resample_args(p, L);
    DevTable table;  // held until the call's launches are enqueued
    if ((st = resample_cached_table(p, A, g.dev, s, &table))) return st;
    A.table = table.get();
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        ResampleArgs G = A;
        group_rows(din, c0, cn, &G.in, 16);
        G.out_aligned16 = group_rows(dout, c0, cn, &G.out, 16);
        return launch_resample(G, cn, s);
    });
    if (st) return st;
    return (st = stage.copy_back()) ? st : finish(ex);
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
    if ((st = whole_rows_only(ex, "dsp_loudness"))) return st;
    if ((st = check_rows("in", in, C))) return st;
    if (lp.hops && hop_energy)
        for (uint32_t c = 0; c < C; ++c)
            if (!hop_energy[c]) return invalid("hop_energy[%u] is NULL", c);
    const bool want_tp = (flags & DSP_LOUDNESS_TRUE_PEAK) != 0;
    const bool run_tp = want_tp && lp.oversample > 1 && L > 0;
    ResamplePlan rp;
    if (want_tp && (st = resample_plan_checked(sr, sr * lp.oversample, L, tp_spec, &rp))) return st;  // (the spec's ranges)
    hipStream_t s = stream_of(ex);
    if ((st = refuse_sync_under_capture(
             s, "stream capture: dsp_loudness returns host values and synchronises its stream")))
        return st;

    std::vector<double> z((size_t)C * lp.hops, 0.0);
    std::vector<uint32_t> peaks((size_t)C * 2, 0u);  // per channel: the bits of the sample and of the true peak
    if (L > 0) {
        DeviceGuard g(ex);
        if (g.status) return g.status;
        Stage stage(ex);
        const std::vector<const float *> din = stage.in_rows(in, C, L);
        if (stage.status) return stage.status;
        DevTable ktab, ttab;  // held until the call's launches are enqueued
        // (an eleventh float: never a BIQUAD cascade's key, whose tables differ)
        std::vector<float> key(lp.kcoef, lp.kcoef + 10);
        key.push_back(0.f);
        st = hold_table(&DeviceRes::iir, key, g.dev, s, "the K-weighting cascade's state-transition tables",
                        [&](std::vector<float> &h, CachedTable &) { loudness_tables(lp.kcoef, h); }, &ktab);
        if (st) return st;
        ResampleArgs R{};
        if (run_tp && (st = oversampler_table(rp, L, lp.oversample, g.dev, s, &R, &ttab))) return st;
        float *scratch = nullptr;
        if ((st = get_scratch(g.dev, s, lp.scratch_bytes, &scratch, kScratchLoudness))) return st;
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
            G.in_aligned16 = group_rows(din, c0, cn, &G.in, 16);
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

int dsp_limiter(const float *const *in, uint32_t C, uint64_t L, float *const *out, uint32_t sr,
                const dsp_limiter_spec *spec, const dsp_resample_spec *tp_spec, float *const *gain,
                float *const *detector, dsp_limiter_result *res, const dsp_exec *ex) {
    LimiterPlan lp;
    ResamplePlan rp;
    int st;
    if ((st = limiter_plan_checked(sr, L, C, spec, tp_spec, &lp, &rp))) return st;
    if ((st = whole_rows_only(ex, "dsp_limiter"))) return st;
    if (L == 0) {  // nothing to read or write: the rows are not looked at
        if (res) res->min_gain = 1.0, res->limited = 0;
        return DSP_OK;
    }
    if ((st = check_rows("in", in, C)) || (st = check_rows("out", out, C))) return st;
    const uint32_t G = lp.groups;
    if (gain && (st = check_rows("gain", gain, G))) return st;
    if (detector && (st = check_rows("detector", detector, G))) return st;
    {
        // (a row set the call does not have is empty)
        const Rows I{in, C, L}, O{out, C, L}, Gn{gain, gain ? G : 0, L}, D{detector, detector ? G : 0, L};
        if (rows_overlap(I, O, true) || rows_overlap_each_other(O) ||
            rows_overlap(Gn, I) || rows_overlap(Gn, O) || rows_overlap_each_other(Gn) ||
            rows_overlap(D, I) || rows_overlap(D, O) || rows_overlap_each_other(D) || rows_overlap(Gn, D))
            return invalid("dsp_limiter: rows overlap (only out[c] == in[c] is allowed)");
    }
    hipStream_t s = stream_of(ex);
    if (res) {
        res->min_gain = 1.0;
        res->limited = 0;
        if ((st = refuse_sync_under_capture(s, "stream capture: dsp_limiter with a result returns host values and "
                                               "synchronises its stream")))
            return st;
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
    st = hold_table(&DeviceRes::limiter, {lp.rho, (float)lp.lookahead}, g.dev, s,
                    "the limiter's release powers and attack window",
                    [&](std::vector<float> &h, CachedTable &) { limiter_table(lp, h); }, &ltab);
    if (st) return st;
    ResampleArgs R{};
    if (lp.oversample > 1 && (st = oversampler_table(rp, L, lp.oversample, g.dev, s, &R, &ttab))) return st;
    float *scratch = nullptr;
    if ((st = get_scratch(g.dev, s, lp.scratch_bytes, &scratch, kScratchLimiter))) return st;

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

    // channels [c0, c0 + cn), and groups [g0, g0 + gn), as a launch's tables
    auto chan_rows = [&](uint32_t c0, uint32_t cn, LimiterArgs *K) {
        K->in_aligned16 = group_rows(din, c0, cn, &K->in, 16);
        K->out_aligned16 = group_rows(dout, c0, cn, &K->out, 16);
        K->gain_aligned16 = 1;  // (until link_rows: no gain row, nothing to store)
    };
    auto link_rows = [&](uint32_t g0, uint32_t gn, LimiterArgs *K) {
        K->gain_aligned16 = group_rows(dgain, g0, gn, &K->gain, 16);
        group_rows(ddet, g0, gn, &K->det, 16);
    };
    if (G == 1) {
        // linked: pass 1 once per 16 channels, p combined (max, exact) in the
        // scratch row before the last launch takes the hold; pass 3 once per 16
        uint32_t chunk = 0;
        st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
            LimiterArgs K = A;
            chan_rows(c0, cn, &K);
            link_rows(0, 1, &K);
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
            chan_rows(c0, cn, &K);
            K.ngroups = 1;
            K.nch = cn;
            if (c0 == 0) {  // the group's gain row and counts: once
                link_rows(0, 1, &K);
                K.words = words;
            }
            return launch_limiter_apply(K, s);
        });
    } else {
        // unlinked: 16 groups of one channel per launch, the scratch rows reused in stream order
        st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
            LimiterArgs K = A;
            chan_rows(c0, cn, &K);
            link_rows(c0, cn, &K);
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

int dsp_rfft(const float *const *in, uint32_t C, uint64_t L, uint32_t n, float *const *spec, const dsp_exec *ex) {
    int st;
    if ((st = dsp_rfft_plan(n, nullptr, nullptr, nullptr))) return st;
    if (L > n) return invalid("dsp_rfft: L %llu > n %u", (unsigned long long)L, n);
    if ((st = whole_rows_only(ex, "dsp_rfft"))) return st;
    if (C == 0) return DSP_OK;
    if ((st = check_rows("spec", spec, C)) || (L && (st = check_rows("in", in, C)))) return st;
    return big_fft_rows(false, in, L, C, n, spec, (uint64_t)n + 2,
                        "dsp_rfft: spectrum rows overlap input rows or each other", ex);
}

int dsp_irfft(const float *const *spec, uint32_t C, uint32_t n, float *const *out, uint64_t Lout,
              const dsp_exec *ex) {
    int st;
    if ((st = dsp_rfft_plan(n, nullptr, nullptr, nullptr))) return st;
    if (Lout > n) return invalid("dsp_irfft: Lout %llu > n %u", (unsigned long long)Lout, n);
    if ((st = whole_rows_only(ex, "dsp_irfft"))) return st;
    if (C == 0 || Lout == 0) return DSP_OK;
    if ((st = check_rows("spec", spec, C)) || (st = check_rows("out", out, C))) return st;
    return big_fft_rows(true, spec, (uint64_t)n + 2, C, n, out, Lout,
                        "dsp_irfft: output rows overlap spectrum rows or each other", ex);
}

int dsp_deconv_plan(uint64_t Ly, uint64_t Ls, uint32_t C, uint32_t *n, uint64_t *scratch_bytes) {
    const char *why = nullptr;
    const int r = deconv_plan(Ly, Ls, C, n, scratch_bytes, &why);
    return plan_status(r, why);
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
    if ((st = whole_rows_only(ex, "dsp_deconvolve"))) return st;
    if (!ref) return invalid("ref is NULL");
    if ((st = check_rows("rec", rec, C)) || (st = check_rows("ir", ir, C))) return st;
    {
        const Rows I{ir, C, ir_len};
        if (rows_overlap(Rows{rec, C, Ly}, I) || rows_overlap(Rows{&ref, 1, Ls}, I) || rows_overlap_each_other(I))
            return invalid("dsp_deconvolve: ir rows overlap rec, ref or each other");
    }
    hipStream_t s = stream_of(ex);
    DeviceGuard g(ex);
    if (g.status) return g.status;
    if ((st = refuse_sync_under_capture(s, "stream capture: dsp_deconvolve reads the excitation's maximum back and "
                                           "synchronises its stream")))
        return st;
    Stage stage(ex);
    const std::vector<const float *> drec = stage.in_rows(rec, C, Ly);
    const float *dref = stage.in(ref, Ls);
    const std::vector<float *> dir = stage.out_rows(ir, C, ir_len);
    if (stage.status) return stage.status;
    BigFft f;
    if ((st = big_fft_open(n, scratch_bytes, g.dev, s, &f))) return st;
    // [rows][2][M] work, [rows][M + 1] the recordings' spectra, [M + 1] the excitation's, the word of the maximum
    const uint32_t rows = std::min<uint32_t>(C, kMaxChannels), bins = n / 2 + 1;
    v2f *Y = reinterpret_cast<v2f *>(f.work) + (uint64_t)rows * n;
    v2f *S = Y + (uint64_t)rows * bins;
    uint32_t *word = reinterpret_cast<uint32_t *>(S + bins);
    DSPB_HIP(hipMemsetAsync(word, 0, 16, s));
    {
        BigFftArgs A{};
        if ((st = big_fft_args(f, 1, &A))) return st;
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
            if (int e = big_fft_args(f, cn, &A)) return e;
            BigFftArgs B = A;  // rec -> Y (A), Y / S in place, Y -> ir (B)
            A.L = Ly;
            B.Lout = ir_len;
            B.rot = pre & (n - 1);
            A.in_aligned8 = group_rows(drec, c0, cn, &A.in, 8);
            B.out_aligned8 = group_rows(dir, c0, cn, &B.out, 8);
            for (uint32_t j = 0; j < cn; ++j) B.in.p[j] = A.out.p[j] = reinterpret_cast<float *>(Y + (uint64_t)j * bins);
            int e;
            if ((e = launch_big_rfft(A, s))) return e;
            if ((e = launch_deconv_divide(Y, S, bins, cn, (float)eps, word, s))) return e;
            return launch_big_irfft(B, s);
        });
        if (st) return st;
    }
    return (st = stage.copy_back()) ? st : finish(ex);
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

int dsp_welch_plan(uint64_t L, uint32_t C, int has_ref, const dsp_welch_spec *spec, uint64_t *frames, uint32_t *bins,
                   uint32_t *run, uint64_t *scratch_bytes, double *win_sum, double *win_sumsq) {
    WelchPlan p;
    if (int st = welch_plan_checked(L, C, has_ref, spec, &p)) return st;
    if (frames) *frames = p.frames;
    if (bins) *bins = kWelchBins;
    if (run) *run = kWelchRun;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    if (win_sum) *win_sum = p.win_sum;
    if (win_sumsq) *win_sumsq = p.win_sumsq;
    return DSP_OK;
}

int dsp_welch(const float *const *in, uint32_t C, uint64_t L, const float *ref, double *const *sxx, double *srr,
              double *const *sxy, const dsp_welch_spec *spec, const dsp_exec *ex) {
    WelchPlan p;
    int st;
    if ((st = welch_plan_checked(L, C, ref != nullptr, spec, &p))) return st;
    if ((st = whole_rows_only(ex, "dsp_welch"))) return st;
    if ((srr != nullptr) != (ref != nullptr) || (sxy != nullptr) != (ref != nullptr))
        return invalid("dsp_welch: srr and sxy go with ref (all three, or none)");
    if ((st = check_rows("in", in, C))) return st;
    // the float64 rows as float rows of twice the length, for the layout checks
    std::vector<const float *> fxx, fxy;
    if ((st = double_rows("dsp_welch", "sxx", sxx, C, &fxx)) || (ref && (st = double_rows("dsp_welch", "sxy", sxy, C, &fxy)))) return st;
    const float *frr = reinterpret_cast<const float *>(srr);
    if (ref && !aligned(srr, 8)) return invalid("dsp_welch: srr is not 8-byte aligned");
    {
        const uint32_t nr = ref ? 1u : 0u;
        const Rows I{in, C, L}, Rf{&ref, nr, L}, XX{fxx.data(), C, 2ull * kWelchBins},
            XY{fxy.data(), ref ? C : 0u, 4ull * kWelchBins}, RR{&frr, nr, 2ull * kWelchBins};
        if (rows_overlap(I, XX) || rows_overlap(I, XY) || rows_overlap(I, RR) || rows_overlap(Rf, XX) ||
            rows_overlap(Rf, XY) || rows_overlap(Rf, RR) || rows_overlap(XX, XY) || rows_overlap(XX, RR) ||
            rows_overlap(XY, RR) || rows_overlap_each_other(XX) || rows_overlap_each_other(XY))
            return invalid("dsp_welch: an output row overlaps an input row or another output row");
    }
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    Stage stage(ex);
    const std::vector<const float *> din = stage.in_rows(in, C, L);
    const float *dref = ref ? stage.in(ref, L) : nullptr;
    std::vector<double *> dxx(C), dxy(C, nullptr);
    for (uint32_t c = 0; c < C; ++c) {
        dxx[c] = (double *)stage.out_bytes(sxx[c], sizeof(double) * kWelchBins);
        if (ref) dxy[c] = (double *)stage.out_bytes(sxy[c], sizeof(double) * 2 * kWelchBins);
    }
    double *drr = ref ? (double *)stage.out_bytes(srr, sizeof(double) * kWelchBins) : nullptr;
    if (stage.status) return stage.status;

    WelchArgs A{};
    const float *win = nullptr;
    if ((st = get_tw(g.dev, s, &A.tw)) || (st = get_window(g.dev, s, p.window, kWelchN, kWelchN, &win))) return st;
    float *scratch = nullptr;
    if ((st = get_scratch(g.dev, s, p.scratch_bytes, &scratch, kScratchWelch))) return st;
    char *base = reinterpret_cast<char *>(scratch);
    A.win2 = reinterpret_cast<const v2f *>(win);
    A.ref = dref;
    A.has_ref = ref ? 1u : 0u;
    A.H = p.H;
    A.chunk = p.chunk;
    A.runs_cap = p.runs_cap;
    A.S = reinterpret_cast<float4 *>(base);
    A.pxx = reinterpret_cast<v2f *>(base + p.off_pxx);
    A.pxy = reinterpret_cast<float4 *>(base + p.off_pxy);
    A.prr = reinterpret_cast<v2f *>(base + p.off_prr);
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        WelchArgs G = A;
        G.cn = cn;
        for (uint32_t j = 0; j < cn; ++j) {
            G.in.p[j] = din[c0 + j];
            G.sxx[j] = dxx[c0 + j];
            G.sxy[j] = dxy[c0 + j];
        }
        G.srr = c0 == 0 ? drr : nullptr;  // the reference's own sums: once
        for (uint64_t f0 = 0; f0 < p.frames; f0 += p.chunk) {
            G.f0 = f0;
            G.nf = (uint32_t)std::min<uint64_t>(p.frames - f0, p.chunk);
            G.first = f0 == 0;
            if (int e = launch_welch_chunk(G, s)) return e;
        }
        return (int)DSP_OK;
    });
    if (st) return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

int dsp_welch_derive(const double *const *sxx, const double *srr, const double *const *sxy, uint32_t C, uint32_t bins,
                     uint64_t frames, double sr, double win_sum, double win_sumsq, uint32_t flags, double *const *psd,
                     double *const *H1, double *const *coherence) {
    if (C == 0 || bins == 0 || frames == 0) return invalid("dsp_welch_derive: needs C >= 1, bins >= 1 and frames >= 1");
    if (flags & ~DSP_WELCH_SPECTRUM) return invalid("dsp_welch_derive: unknown flags");
    const bool cross = H1 || coherence;
    if ((psd || coherence) && !sxx) return invalid("sxx is NULL");
    if (cross && (!srr || !sxy)) return invalid("dsp_welch_derive: H1 and coherence need srr and sxy");
    for (uint32_t c = 0; c < C; ++c)
        if ((sxx && !sxx[c]) || (cross && !sxy[c]) || (psd && !psd[c]) || (H1 && !H1[c]) || (coherence && !coherence[c]))
            return invalid("dsp_welch_derive: row %u is NULL", c);
    if (psd) {
        const double scale = (flags & DSP_WELCH_SPECTRUM) ? win_sum * win_sum : sr * win_sumsq;
        if (!std::isfinite(scale) || scale <= 0.0)
            return invalid("dsp_welch_derive: the scale (sr, win_sum, win_sumsq) must be finite and positive");
    }
    welch_derive(sxx, srr, sxy, C, bins, frames, sr, win_sum, win_sumsq, flags, psd, H1, coherence);
    return DSP_OK;
}

int dsp_stft_plan(uint64_t L, uint32_t C, const dsp_stft_spec *spec, uint64_t *frames, uint32_t *bins,
                  uint64_t *min_ld) {
    StftCxPlan p;
    const char *why = nullptr;
    if (int st = plan_status(stft_cx_plan(L, C, spec, &p, &why), why)) return st;
    if (frames) *frames = p.frames;
    if (bins) *bins = kStftCxBins;
    if (min_ld) *min_ld = p.min_ld;
    return DSP_OK;
}

int dsp_stft(const float *const *in, uint32_t C, uint64_t L, float *const *spec, uint64_t ld, const dsp_stft_spec *sp,
             const dsp_exec *ex) {
    StftCxPlan p;
    const char *why = nullptr;
    int st;
    if ((st = plan_status(stft_cx_plan(L, C, sp, &p, &why), why))) return st;
    if ((st = plan_status(stft_cx_check_ld(false, p.frames, ld, &why), why))) return st;
    if ((st = whole_rows_only(ex, "dsp_stft"))) return st;
    if ((st = check_rows("in", in, C)) || (st = spectrum_rows("dsp_stft", spec, C))) return st;
    // a row's extent: its last frame ends at 2 K, not at ld
    const uint64_t span = (p.frames - 1) * ld + 2ull * kStftCxBins;
    if (rows_overlap(Rows{in, C, L}, Rows{spec, C, span}) || rows_overlap_each_other(Rows{spec, C, span}))
        return invalid("dsp_stft: an output row overlaps an input row or another output row");
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    Stage stage(ex);
    const std::vector<const float *> din = stage.in_rows(in, C, L);
    // host rows: a dense device row each, copied back frame by frame, so that
    // the floats [2 K, ld) of a frame stay the caller's
    const uint64_t dense = 2ull * kStftCxBins;
    std::vector<float *> dspec(C);
    for (uint32_t c = 0; c < C; ++c) {
        void *d = spec[c];
        if (stage.host && (stage.status = stage.alloc(sizeof(float) * p.frames * dense, &d))) break;
        dspec[c] = (float *)d;
    }
    if (stage.status) return stage.status;

    StftCxArgs A{};
    const float *win = nullptr;
    if ((st = get_tw(g.dev, s, &A.tw)) || (st = get_window(g.dev, s, p.window, kStftCxN, kStftCxN, &win))) return st;
    A.win2 = reinterpret_cast<const v2f *>(win);
    A.H = p.H;
    A.ld = stage.host ? dense : ld;
    A.f0 = 0;
    A.nf = p.frames;
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        StftCxArgs G = A;
        G.cn = cn;
        group_rows(din, c0, cn, &G.in, 4);
        group_rows(dspec, c0, cn, &G.spec, 8);
        return launch_stft_cx(G, s);
    });
    if (st) return st;
    if (stage.host)
        for (uint32_t c = 0; c < C; ++c)
            DSPB_HIP(hipMemcpy2DAsync(spec[c], ld * sizeof(float), dspec[c], dense * sizeof(float),
                                      dense * sizeof(float), p.frames, hipMemcpyDeviceToHost, s));
    return finish(ex);
}

int dsp_istft_plan(uint64_t F, uint32_t C, const dsp_istft_spec *spec, uint64_t *Lout, uint32_t *overlap,
                   uint32_t *chunk, uint64_t *scratch_bytes) {
    IstftPlan p;
    const char *why = nullptr;
    if (int st = plan_status(istft_plan(F, C, spec, &p, &why), why)) return st;
    if (Lout) *Lout = p.Lout_full;
    if (overlap) *overlap = p.overlap;
    if (chunk) *chunk = p.chunk;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return DSP_OK;
}

int dsp_istft(const float *const *spec, uint32_t C, uint64_t F, uint64_t ld, float *const *out, uint64_t Lout,
              const dsp_istft_spec *sp, const dsp_exec *ex) {
    IstftPlan p;
    const char *why = nullptr;
    int st;
    if ((st = plan_status(istft_plan(F, C, sp, &p, &why), why))) return st;
    if ((st = plan_status(stft_cx_check_ld(true, F, ld, &why), why))) return st;
    if ((st = plan_status(istft_check_lout(p, Lout, &why), why))) return st;
    if ((st = whole_rows_only(ex, "dsp_istft"))) return st;
    if ((st = spectrum_rows("dsp_istft", spec, C)) || (st = check_rows("out", out, C))) return st;
    const uint64_t span = (F - 1) * ld + 2ull * kStftCxBins;
    if (rows_overlap(Rows{spec, C, span}, Rows{out, C, Lout}) || rows_overlap_each_other(Rows{out, C, Lout}))
        return invalid("dsp_istft: an output row overlaps an input row or another output row");
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    Stage stage(ex);
    const std::vector<const float *> dspec = stage.in_rows(spec, C, span);
    const std::vector<float *> dout = stage.out_rows(out, C, Lout);
    if (stage.status) return stage.status;

    IstftArgs A{};
    if ((st = get_tw(g.dev, s, &A.tw)) || (st = get_window(g.dev, s, p.window, kStftCxN, kStftCxN, &A.win))) return st;
    if ((st = get_scratch(g.dev, s, p.scratch_bytes, &A.S, kScratchIstft))) return st;
    A.win2 = reinterpret_cast<const v2f *>(A.win);
    A.H = p.H;
    A.ld = ld;
    A.F = F;
    A.slots = p.slots;
    A.floor = p.floor;
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        IstftArgs G = A;
        G.cn = cn;
        group_rows(dspec, c0, cn, &G.spec, 8);
        group_rows(dout, c0, cn, &G.out, 4);
        for (uint64_t f0 = 0; f0 < F; f0 += p.chunk) {
            const IstftChunk ch = istft_chunk(p, f0, Lout);
            if (ch.nf == 0) break;  // past Lout
            G.fa = ch.fa, G.ns = ch.ns, G.i0 = ch.i0, G.i1 = ch.i1;
            if (int e = launch_istft_chunk(G, s)) return e;
        }
        return (int)DSP_OK;
    });
    if (st) return st;
    return (st = stage.copy_back()) ? st : finish(ex);
}

int dsp_pvoc_plan(uint64_t F, uint32_t C, const dsp_pvoc_spec *spec, uint64_t *frames_out, uint32_t *chunk,
                  uint64_t *scratch_bytes) {
    PvocPlan p;
    const char *why = nullptr;
    if (int st = plan_status(pvoc_plan(F, C, spec, &p, &why, g_pvoc_chunk.load()), why)) return st;
    if (frames_out) *frames_out = p.frames_out;
    if (chunk) *chunk = p.chunk;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return DSP_OK;
}

int dsp_pvoc(const float *const *spec_in, uint32_t C, uint64_t F, uint64_t ld_in, float *const *spec_out,
             uint64_t ld_out, const dsp_pvoc_spec *sp, const dsp_exec *ex) {
    PvocPlan p;
    const char *why = nullptr;
    int st;
    if ((st = plan_status(pvoc_plan(F, C, sp, &p, &why, g_pvoc_chunk.load()), why))) return st;
    if ((st = plan_status(pvoc_check_ld(F, ld_in, &why), why))) return st;
    if ((st = plan_status(pvoc_check_ld(p.frames_out, ld_out, &why), why))) return st;
    if ((st = whole_rows_only(ex, "dsp_pvoc"))) return st;
    if ((st = spectrum_rows("dsp_pvoc", spec_in, C)) || (st = spectrum_rows("dsp_pvoc", spec_out, C))) return st;
    // a row's extent: its last frame ends at 2 K, not at ld
    const uint64_t dense = 2ull * kStftCxBins;
    const uint64_t span_in = (F - 1) * ld_in + dense, span_out = (p.frames_out - 1) * ld_out + dense;
    if (rows_overlap(Rows{spec_in, C, span_in}, Rows{spec_out, C, span_out}) ||
        rows_overlap_each_other(Rows{spec_out, C, span_out}))
        return invalid("dsp_pvoc: an output row overlaps an input row or another output row");
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    Stage stage(ex);
    const std::vector<const float *> din = stage.in_rows(spec_in, C, span_in);
    // host rows: a dense device row each, copied back frame by frame (as dsp_stft does)
    std::vector<float *> dout(C);
    for (uint32_t c = 0; c < C; ++c) {
        void *d = spec_out[c];
        if (stage.host && (stage.status = stage.alloc(sizeof(float) * p.frames_out * dense, &d))) break;
        dout[c] = (float *)d;
    }
    if (stage.status) return stage.status;

    PvocArgs A{};
    float *scratch = nullptr;
    // (the A/B variant that stores every increment keeps them behind the sums)
    A.variant = g_pvoc_variant.load();
    const uint64_t inc_bytes = (A.variant & 4u) ? (uint64_t)p.rows * p.frames_out * kStftCxBins * sizeof(uint32_t) : 0;
    if ((st = get_scratch(g.dev, s, p.scratch_bytes + inc_bytes, &scratch, kScratchPvoc))) return st;
    A.S = reinterpret_cast<uint32_t *>(scratch);
    A.inc = inc_bytes ? A.S + p.scratch_bytes / sizeof(uint32_t) : nullptr;
    A.ld_in = ld_in;
    A.ld_out = stage.host ? dense : ld_out;
    A.F = F;
    A.frames_out = p.frames_out;
    A.rate = p.rate;
    A.chunk = p.chunk;
    A.chunks = p.chunks;
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        PvocArgs G = A;
        G.cn = cn;
        group_rows(din, c0, cn, &G.in, 8);
        group_rows(dout, c0, cn, &G.out, 8);
        return launch_pvoc(G, s);
    });
    if (st) return st;
    if (stage.host)
        for (uint32_t c = 0; c < C; ++c)
            DSPB_HIP(hipMemcpy2DAsync(spec_out[c], ld_out * sizeof(float), dout[c], dense * sizeof(float),
                                      dense * sizeof(float), p.frames_out, hipMemcpyDeviceToHost, s));
    return finish(ex);
}

int dsp_time_stretch_plan(uint64_t L, uint32_t C, const dsp_stretch_spec *spec, uint64_t *frames_in,
                          uint64_t *frames_out, uint64_t *Lout_full, uint64_t *Lout_default,
                          uint64_t *device_bytes) {
    StretchPlan p;
    const char *why = nullptr;
    if (int st = plan_status(stretch_plan(L, C, spec, &p, &why), why)) return st;
    if (frames_in) *frames_in = p.frames_in;
    if (frames_out) *frames_out = p.frames_out;
    if (Lout_full) *Lout_full = p.Lout_full;
    if (Lout_default) *Lout_default = p.Lout_default;
    if (device_bytes) *device_bytes = p.device_bytes;
    return DSP_OK;
}

namespace {
// the two spectrograms of a dsp_time_stretch call: freed when the call returns
struct StretchScratch {
    float *a = nullptr, *b = nullptr;
    ~StretchScratch() {
        (void)hipFree(a);
        (void)hipFree(b);
    }
};
}  // namespace

int dsp_time_stretch(const float *const *in, uint32_t C, uint64_t L, float *const *out, uint64_t Lout,
                     const dsp_stretch_spec *sp, const dsp_exec *ex) {
    StretchPlan p;
    const char *why = nullptr;
    int st;
    if ((st = plan_status(stretch_plan(L, C, sp, &p, &why), why))) return st;
    if (Lout == 0 || Lout > p.Lout_full) return invalid("dsp_time_stretch: needs 1 <= Lout <= N + (F' - 1) H");
    if ((st = whole_rows_only(ex, "dsp_time_stretch"))) return st;
    if ((st = check_rows("in", in, C)) || (st = check_rows("out", out, C))) return st;
    if (rows_overlap(Rows{in, C, L}, Rows{out, C, Lout}) || rows_overlap_each_other(Rows{out, C, Lout}))
        return invalid("dsp_time_stretch: an output row overlaps an input row or another output row");
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    if ((st = refuse_capture(s, "dsp_time_stretch's pair of spectrograms (allocated per call)"))) return st;
    Stage stage(ex);
    const std::vector<const float *> din = stage.in_rows(in, C, L);
    const std::vector<float *> dout = stage.out_rows(out, C, Lout);
    if (stage.status) return stage.status;
    StretchScratch sc;
    hipError_t me = hipMalloc(&sc.a, p.in_bytes);
    if (me == hipSuccess) me = hipMalloc(&sc.b, p.out_bytes);
    if (me != hipSuccess) {
        (void)hipGetLastError();  // the refusal is this call's answer, not a later launch's
        return hip_fail(me, "dsp_time_stretch: hipMalloc of the spectrograms");
    }
    // the three public calls on device rows, on the caller's stream
    dsp_exec dev{};
    dev.device = g.dev;
    dev.stream = (void *)s;
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        const float *zin[kMaxChannels];
        float *zout[kMaxChannels];
        for (uint32_t j = 0; j < cn; ++j) {
            zin[j] = sc.a + (uint64_t)j * p.frames_in * p.ld;
            zout[j] = sc.b + (uint64_t)j * p.frames_out * p.ld;
        }
        if (int e = dsp_stft(din.data() + c0, cn, L, const_cast<float *const *>(zin), p.ld, &p.fwd, &dev)) return e;
        if (int e = dsp_pvoc(zin, cn, p.frames_in, p.ld, zout, p.ld, &p.pv, &dev)) return e;
        return dsp_istft(zout, cn, p.frames_out, p.ld, dout.data() + c0, Lout, &p.inv, &dev);
    });
    if (!st) st = stage.copy_back();
    // the spectrograms leave with the call: what was enqueued must have read them
    const hipError_t e = hipStreamSynchronize(s);
    if (st) return st;
    DSPB_HIP(e);
    return finish(ex);
}

int dsp_pitch_shift_plan(uint64_t L, uint32_t C, double semitones, uint32_t H, int32_t window, uint32_t *p, uint32_t *q,
                         dsp_stretch_spec *stretch, uint64_t *padded, uint64_t *stretched, uint64_t *Lout) {
    PitchPlan pl;
    const char *why = nullptr;
    if (int st = plan_status(pitch_plan(L, C, semitones, H, window, &pl, &why), why)) return st;
    ResamplePlan rp;
    if (int st = resample_plan_checked(pl.p, pl.q, pl.stretched, nullptr, &rp)) return st;
    if (p) *p = pl.p;
    if (q) *q = pl.q;
    if (stretch) *stretch = pl.stretch;
    if (padded) *padded = pl.padded;
    if (stretched) *stretched = pl.stretched;
    if (Lout) *Lout = rp.Lout;
    return DSP_OK;
}

int dsp_pitch_ratio(double semitones, uint32_t *p, uint32_t *q) {
    const char *why = nullptr;
    return plan_status(pitch_ratio(semitones, p, q, &why), why);
}

int dsp_decay_plan(uint64_t L, uint32_t C, uint32_t sr, const dsp_decay_spec *spec, uint32_t *n, uint32_t *P,
                   uint32_t *hop, uint32_t *bands, uint64_t *hops, uint64_t *scratch_bytes, double *fm) {
    DecayPlan p;
    if (int st = decay_plan_checked(L, C, sr, spec, &p)) return st;
    if (n) *n = p.n;
    if (P) *P = p.P;
    if (hop) *hop = p.hop;
    if (bands) *bands = p.bands;
    if (hops) *hops = p.hops;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    if (fm) std::memcpy(fm, p.fm, sizeof p.fm);
    return DSP_OK;
}

int dsp_decay(const float *const *in, uint32_t C, uint64_t L, uint32_t sr, const dsp_decay_spec *spec, float *peak,
              uint64_t *onset, double *const *energy, double *const *moment, const dsp_exec *ex) {
    DecayPlan p;
    int st;
    if ((st = decay_plan_checked(L, C, sr, spec, &p))) return st;
    if ((st = whole_rows_only(ex, "dsp_decay"))) return st;
    if ((st = check_rows("in", in, C))) return st;
    if (!peak || !onset) return invalid("dsp_decay: peak or onset is NULL");
    if (!aligned(peak, 4) || !aligned(onset, 8)) return invalid("dsp_decay: peak or onset is misaligned");
    const uint32_t B = p.bands, R = C * B;
    if (R / B != C) return invalid("dsp_decay: too many rows");
    // the float64 rows as float rows of twice the length, for the layout checks
    std::vector<const float *> fe, fm;
    if ((st = double_rows("dsp_decay", "energy", energy, R, &fe)) || (moment && (st = double_rows("dsp_decay", "moment", moment, R, &fm))))
        return st;
    {
        const float *fp = peak, *fo = reinterpret_cast<const float *>(onset);
        const Rows I{in, C, L}, E{fe.data(), R, 2 * p.hops}, M{fm.data(), moment ? R : 0u, 2 * p.hops}, Pk{&fp, 1, C},
            On{&fo, 1, 2ull * C};
        const Rows *outs[] = {&E, &M, &Pk, &On};
        bool bad = rows_overlap_each_other(E) || rows_overlap_each_other(M);
        for (int i = 0; i < 4; ++i) {
            bad = bad || rows_overlap(I, *outs[i]);
            for (int j = i + 1; j < 4; ++j) bad = bad || rows_overlap(*outs[i], *outs[j]);
        }
        if (bad) return invalid("dsp_decay: an output row overlaps an input row or another output row");
    }
    DeviceGuard g(ex);
    if (g.status) return g.status;
    hipStream_t s = stream_of(ex);
    Stage stage(ex);
    const std::vector<const float *> din = stage.in_rows(in, C, L);
    float *dpeak = (float *)stage.out_bytes(peak, sizeof(float) * C);
    unsigned long long *donset = (unsigned long long *)stage.out_bytes(onset, sizeof(uint64_t) * C);
    std::vector<double *> de(R), dm(R, nullptr);
    for (uint32_t r = 0; r < R; ++r) {
        de[r] = (double *)stage.out_bytes(energy[r], sizeof(double) * p.hops);
        if (moment) dm[r] = (double *)stage.out_bytes(moment[r], sizeof(double) * p.hops);
    }
    if (stage.status) return stage.status;
    BigFft f;
    if ((st = big_fft_open(p.n, p.scratch_bytes, g.dev, s, &f))) return st;
    char *base = reinterpret_cast<char *>(f.work);
    const uint32_t bins = p.n / 2 + 1;
    v2f *X = reinterpret_cast<v2f *>(base + p.off_x), *Y = reinterpret_cast<v2f *>(base + p.off_y);
    float *ir = reinterpret_cast<float *>(base + p.off_ir);

    // peak and onset of every channel, straight onto the output words
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        DecayArgs A{};
        group_rows(din, c0, cn, &A.in, 4);
        A.cn = cn;
        A.L = L;
        A.peak = dpeak + c0;
        A.onset = donset + c0;
        return launch_decay_onset(A, s);
    });
    if (st) return st;
    // p.rows channels at a time: their spectra, then their (channel, band) rows in groups of p.rows
    for (uint32_t c0 = 0; c0 < C; c0 += p.rows) {
        const uint32_t cc = std::min(C - c0, p.rows);
        {
            BigFftArgs A{};
            if ((st = big_fft_args(f, cc, &A))) return st;
            A.L = L;
            A.in_aligned8 = group_rows(din, c0, cc, &A.in, 8);
            for (uint32_t j = 0; j < cc; ++j) A.out.p[j] = reinterpret_cast<float *>(X + (uint64_t)j * bins);
            if ((st = launch_big_rfft(A, s))) return st;
        }
        for (uint32_t q0 = 0; q0 < cc * B; q0 += p.rows) {
            const uint32_t nr = std::min(cc * B - q0, p.rows);
            DecayArgs D{};
            BigFftArgs A{};
            if ((st = big_fft_args(f, nr, &A))) return st;
            A.Lout = L;
            D.L = L, D.nrows = nr, D.bins = bins, D.X = X, D.Y = Y, D.Qd = (float)p.Qd;
            D.onset = donset, D.ir = ir, D.Lp = p.Lp, D.hop = p.hop, D.hops = p.hops;
            D.pre = reinterpret_cast<double *>(base + p.off_pre);
            for (uint32_t r = 0; r < nr; ++r) {
                const uint32_t j = (q0 + r) / B, b = (q0 + r) % B, row = (c0 + j) * B + b;
                D.xrow[r] = j;
                D.chan[r] = c0 + j;
                D.fscale[r] = (float)((double)sr / ((double)p.n * p.fm[b]));
                D.energy[r] = de[row];
                D.moment[r] = dm[row];
                A.in.p[r] = reinterpret_cast<const float *>(Y + (uint64_t)r * bins);
                A.out.p[r] = ir + (uint64_t)r * p.Lp;
            }
            if ((st = launch_decay_mask(D, s)) || (st = launch_big_irfft(A, s)) || (st = launch_decay_hops(D, s))) return st;
        }
    }
    return (st = stage.copy_back()) ? st : finish(ex);
}

int dsp_decay_derive(const double *energy, const double *moment, uint64_t L, uint64_t onset, uint32_t hop, uint32_t sr,
                     dsp_decay_result *res) {
    if (!energy || !res) return invalid("dsp_decay_derive: energy or res is NULL");
    if (hop == 0 || hop != decay_hop(sr)) return invalid("dsp_decay_derive: hop is not dsp_decay_plan's for this rate");
    if (onset > L) return invalid("dsp_decay_derive: onset > L");
    decay_derive(energy + 1, moment ? moment + 1 : nullptr, (L - onset) / hop, hop, sr, res);
    return DSP_OK;
}

}  // extern "C"
