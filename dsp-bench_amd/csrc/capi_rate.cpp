// capi_rate.cpp -- the Plugin-free row calls of rate and level
// (include/dspbench/dspbench.h): dsp_resample, dsp_loudness and dsp_limiter,
// with their plans.  They share the resampler's cached table, which is also the
// true-peak detector's.  As every row call does, each checks its arguments and
// its rows' layout before it looks at a device, holds its cached tables until
// its launches are enqueued, and walks its channels in groups of kMaxChannels.
#include "capi_impl.hpp"
#include "limiter_host.hpp"
#include "loudness_host.hpp"

namespace dspb {

int resample_plan_checked(uint32_t sr_in, uint32_t sr_out, uint64_t L, const dsp_resample_spec *spec,
                          ResamplePlan *plan) {
    const dsp_resample_spec def{64u, 14.769656459379492, 0.9475937167399596};
    if (!spec) spec = &def;
    return plan_checked(resample_plan, sr_in, sr_out, L, spec->zeros, spec->beta, spec->rolloff, plan);
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

// dsp_limiter_plan's two plans: the limiter's own, then (TRUE_PEAK at ovs > 1) the oversampler's
static int limiter_plans(uint32_t sr, uint64_t L, uint32_t C, const dsp_limiter_spec *spec,
                         const dsp_resample_spec *tp_spec, LimiterPlan *p, ResamplePlan *rp) {
    if (int st = plan_checked(limiter_plan, sr, L, C, spec, p)) return st;
    if (spec->flags & DSP_LIMITER_TRUE_PEAK) return resample_plan_checked(sr, sr * p->oversample, L, tp_spec, rp);
    return DSP_OK;
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
    // (kOutputsUnchecked: this call has never looked at its output rows among themselves)
    if (output_rows_overlap({Rows{in, C, L}}, {Rows{out, C, Lout}}, kOutputsUnchecked))
        return invalid("dsp_resample: output rows overlap input rows");
    RowCall rc(ex);
    if (rc.status) return rc.status;
    const std::vector<const float *> din = rc.stage.in_rows(in, C, L);
    const std::vector<float *> dout = rc.stage.out_rows(out, C, Lout);
    if (rc.stage.status) return rc.stage.status;
    if (p.up == 1 && p.down == 1) {  // the same rate: a copy, no filter
        for (uint32_t c = 0; c < C; ++c)
            DSPB_HIP(hipMemcpyAsync(dout[c], din[c], L * sizeof(float), hipMemcpyDeviceToDevice, rc.s));
        return rc.done();
    }
    ResampleArgs A = resample_args(p, L);
    DevTable table;  // held until the call's launches are enqueued
    if ((st = resample_cached_table(p, A, rc.dev, rc.s, &table))) return st;
    A.table = table.get();
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        ResampleArgs G = A;
        group_rows(din, c0, cn, &G.in, 16);
        G.out_aligned16 = group_rows(dout, c0, cn, &G.out, 16);
        return launch_resample(G, cn, rc.s);
    });
    return st ? st : rc.done();
}

int dsp_loudness_plan(uint32_t sr, uint64_t L, uint32_t *hop, uint64_t *hops, uint32_t *oversample, float kcoef[10],
                      uint64_t *scratch_bytes) {
    LoudnessPlan p;
    if (plan_checked(loudness_plan, sr, L, &p)) return DSP_ERR_UNSUPPORTED;  // (the rate or the length is out of range)
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
    if (plan_checked(loudness_plan, sr, L, &lp)) return DSP_ERR_UNSUPPORTED;  // (the rate or the length is out of range)
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
    if (L > 0) {  // (no samples: no device is looked at; the call's ending is its own synchronise)
        RowCall rc(ex);
        if (rc.status) return rc.status;
        const std::vector<const float *> din = rc.stage.in_rows(in, C, L);
        if (rc.stage.status) return rc.stage.status;
        DevTable ktab, ttab;  // held until the call's launches are enqueued
        // (an eleventh float: never a BIQUAD cascade's key, whose tables differ)
        std::vector<float> key(lp.kcoef, lp.kcoef + 10);
        key.push_back(0.f);
        st = hold_table(&DeviceRes::iir, key, rc.dev, s, "the K-weighting cascade's state-transition tables",
                        [&](std::vector<float> &h, CachedTable &) { loudness_tables(lp.kcoef, h); }, &ktab);
        if (st) return st;
        ResampleArgs R{};
        if (run_tp && (st = oversampler_table(rp, L, lp.oversample, rc.dev, s, &R, &ttab))) return st;
        float *scratch = nullptr;
        if ((st = get_scratch(rc.dev, s, lp.scratch_bytes, &scratch, kScratchLoudness))) return st;
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
    if (int st = limiter_plans(sr, L, C, spec, tp_spec, &p, &rp)) return st;
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
    if ((st = limiter_plans(sr, L, C, spec, tp_spec, &lp, &rp))) return st;
    if ((st = whole_rows_only(ex, "dsp_limiter"))) return st;
    if (L == 0) {  // nothing to read or write: the rows are not looked at
        if (res) res->min_gain = 1.0, res->limited = 0;
        return DSP_OK;
    }
    if ((st = check_rows("in", in, C)) || (st = check_rows("out", out, C))) return st;
    const uint32_t G = lp.groups;
    if (gain && (st = check_rows("gain", gain, G))) return st;
    if (detector && (st = check_rows("detector", detector, G))) return st;
    // (a row set the call does not have is empty; kInPlaceOk: out[c] == in[c], and only that, is allowed)
    if (output_rows_overlap({Rows{in, C, L}},
                            {Rows{out, C, L}, Rows{gain, gain ? G : 0, L}, Rows{detector, detector ? G : 0, L}},
                            kInPlaceOk))
        return invalid("dsp_limiter: rows overlap (only out[c] == in[c] is allowed)");
    if (res) {
        res->min_gain = 1.0;
        res->limited = 0;
        if ((st = refuse_sync_under_capture(stream_of(ex), "stream capture: dsp_limiter with a result returns host "
                                                           "values and synchronises its stream")))
            return st;
    }
    RowCall rc(ex);
    if (rc.status) return rc.status;
    Stage &stage = rc.stage;
    const hipStream_t s = rc.s;
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
    st = hold_table(&DeviceRes::limiter, {lp.rho, (float)lp.lookahead}, rc.dev, s,
                    "the limiter's release powers and attack window",
                    [&](std::vector<float> &h, CachedTable &) { limiter_table(lp, h); }, &ltab);
    if (st) return st;
    ResampleArgs R{};
    if (lp.oversample > 1 && (st = oversampler_table(rp, L, lp.oversample, rc.dev, s, &R, &ttab))) return st;
    float *scratch = nullptr;
    if ((st = get_scratch(rc.dev, s, lp.scratch_bytes, &scratch, kScratchLimiter))) return st;

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
    if (!res) return rc.done();
    // with a result the call reads the counts back and synchronises itself
    uint32_t w[4] = {0, 0, 0, 0};
    DSPB_HIP(hipMemcpyAsync(w, words, sizeof w, hipMemcpyDeviceToHost, s));
    if ((st = stage.copy_back())) return st;
    DSPB_HIP(hipStreamSynchronize(s));
    const uint32_t b = (w[0] & 0x80000000u) ? (w[0] & 0x7fffffffu) : ~w[0];
    float m;
    std::memcpy(&m, &b, 4);
    res->min_gain = (double)m;
    res->limited = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    return DSP_OK;
}

}  // extern "C"
