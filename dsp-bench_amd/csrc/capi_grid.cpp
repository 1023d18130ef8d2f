// capi_grid.cpp -- the Plugin-free row calls on the 8192-point grid
// (include/dspbench/dspbench.h): dsp_welch, dsp_stft / dsp_istft, dsp_pvoc /
// dsp_time_stretch and the pitch-shift plan.  They share the 8192-point
// twiddles and windows (get_tw, get_window) and the layout of a spectrum row.
// The rules of a row call are at the head of capi_rate.cpp.
#include "capi_impl.hpp"
#include "pvoc_host.hpp"
#include "stft_cx_host.hpp"
#include "welch_host.hpp"

namespace dspb {

static_assert(kWelchGroup == kMaxChannels, "welch_plan sizes the scratch for for_groups' channel groups");
static_assert(kStftCxGroup == kMaxChannels, "istft_plan sizes the scratch for for_groups' channel groups");
static_assert(kPvocGroup == kMaxChannels, "pvoc_plan sizes the scratch for for_groups' channel groups");

// spectrum rows (dsp_stft's outputs, dsp_istft's inputs, both of dsp_pvoc's): none NULL, each 8-byte aligned
static int spectrum_rows(const char *call, const float *const *rows, uint32_t C) {
    if (int st = check_rows("spec", rows, C)) return st;
    for (uint32_t c = 0; c < C; ++c)
        if (!aligned(rows[c], 8)) return invalid("%s: spec[%u] is not 8-byte aligned", call, c);
    return DSP_OK;
}
// a spectrum row's floats and extent: its last frame ends at 2 K, not at ld
constexpr uint64_t kDense = 2ull * kStftCxBins;
static uint64_t spectrum_span(uint64_t frames, uint64_t ld) { return (frames - 1) * ld + kDense; }

// pvoc_plan at the debug hook's chunk (DSP_DEBUG_PVOC_CHUNK)
static int pvoc_plan_here(uint64_t F, uint32_t C, const dsp_pvoc_spec *spec, PvocPlan *p, const char **why) {
    return pvoc_plan(F, C, spec, p, why, g_pvoc_chunk.load());
}

}  // namespace dspb

using namespace dspb;

extern "C" {

int dsp_welch_plan(uint64_t L, uint32_t C, int has_ref, const dsp_welch_spec *spec, uint64_t *frames, uint32_t *bins,
                   uint32_t *run, uint64_t *scratch_bytes, double *win_sum, double *win_sumsq) {
    WelchPlan p;
    if (int st = plan_checked(welch_plan, L, C, has_ref, spec, &p)) return st;
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
    if ((st = plan_checked(welch_plan, L, C, ref != nullptr, spec, &p))) return st;
    if ((st = whole_rows_only(ex, "dsp_welch"))) return st;
    if ((srr != nullptr) != (ref != nullptr) || (sxy != nullptr) != (ref != nullptr))
        return invalid("dsp_welch: srr and sxy go with ref (all three, or none)");
    if ((st = check_rows("in", in, C))) return st;
    // the float64 rows as float rows of twice the length, for the layout checks
    std::vector<const float *> fxx, fxy;
    if ((st = double_rows("dsp_welch", "sxx", sxx, C, &fxx)) || (ref && (st = double_rows("dsp_welch", "sxy", sxy, C, &fxy)))) return st;
    const float *frr = reinterpret_cast<const float *>(srr);
    if (ref && !aligned(srr, 8)) return invalid("dsp_welch: srr is not 8-byte aligned");
    const uint32_t nr = ref ? 1u : 0u;  // (without ref its three sets are empty)
    if (output_rows_overlap({Rows{in, C, L}, Rows{&ref, nr, L}},
                            {Rows{fxx.data(), C, 2ull * kWelchBins}, Rows{fxy.data(), ref ? C : 0u, 4ull * kWelchBins},
                             Rows{&frr, nr, 2ull * kWelchBins}}))
        return invalid("dsp_welch: an output row overlaps an input row or another output row");
    RowCall rc(ex);
    if (rc.status) return rc.status;
    const hipStream_t s = rc.s;
    const std::vector<const float *> din = rc.stage.in_rows(in, C, L);
    const float *dref = ref ? rc.stage.in(ref, L) : nullptr;
    std::vector<double *> dxx(C), dxy(C, nullptr);
    for (uint32_t c = 0; c < C; ++c) {
        dxx[c] = (double *)rc.stage.out_bytes(sxx[c], sizeof(double) * kWelchBins);
        if (ref) dxy[c] = (double *)rc.stage.out_bytes(sxy[c], sizeof(double) * 2 * kWelchBins);
    }
    double *drr = ref ? (double *)rc.stage.out_bytes(srr, sizeof(double) * kWelchBins) : nullptr;
    if (rc.stage.status) return rc.stage.status;

    WelchArgs A{};
    const float *win = nullptr;
    if ((st = get_tw(rc.dev, s, &A.tw)) || (st = get_window(rc.dev, s, p.window, kWelchN, kWelchN, &win))) return st;
    float *scratch = nullptr;
    if ((st = get_scratch(rc.dev, s, p.scratch_bytes, &scratch, kScratchWelch))) return st;
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
    return st ? st : rc.done();
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
    if (int st = plan_checked(stft_cx_plan, L, C, spec, &p)) return st;
    if (frames) *frames = p.frames;
    if (bins) *bins = kStftCxBins;
    if (min_ld) *min_ld = p.min_ld;
    return DSP_OK;
}

int dsp_stft(const float *const *in, uint32_t C, uint64_t L, float *const *spec, uint64_t ld, const dsp_stft_spec *sp,
             const dsp_exec *ex) {
    StftCxPlan p;
    int st;
    if ((st = plan_checked(stft_cx_plan, L, C, sp, &p))) return st;
    if ((st = plan_checked(stft_cx_check_ld, false, p.frames, ld))) return st;
    if ((st = whole_rows_only(ex, "dsp_stft"))) return st;
    if ((st = check_rows("in", in, C)) || (st = spectrum_rows("dsp_stft", spec, C))) return st;
    if (output_rows_overlap({Rows{in, C, L}}, {Rows{spec, C, spectrum_span(p.frames, ld)}}))
        return invalid("dsp_stft: an output row overlaps an input row or another output row");
    RowCall rc(ex);
    if (rc.status) return rc.status;
    const std::vector<const float *> din = rc.stage.in_rows(in, C, L);
    const std::vector<float *> dspec = rc.stage.out_framed_rows(spec, C, p.frames, kDense, ld);
    if (rc.stage.status) return rc.stage.status;

    StftCxArgs A{};
    const float *win = nullptr;
    if ((st = get_tw(rc.dev, rc.s, &A.tw)) || (st = get_window(rc.dev, rc.s, p.window, kStftCxN, kStftCxN, &win))) return st;
    A.win2 = reinterpret_cast<const v2f *>(win);
    A.H = p.H;
    A.ld = rc.stage.framed_ld(kDense, ld);
    A.f0 = 0;
    A.nf = p.frames;
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        StftCxArgs G = A;
        G.cn = cn;
        group_rows(din, c0, cn, &G.in, 4);
        group_rows(dspec, c0, cn, &G.spec, 8);
        return launch_stft_cx(G, rc.s);
    });
    return st ? st : rc.done();
}

int dsp_istft_plan(uint64_t F, uint32_t C, const dsp_istft_spec *spec, uint64_t *Lout, uint32_t *overlap,
                   uint32_t *chunk, uint64_t *scratch_bytes) {
    IstftPlan p;
    if (int st = plan_checked(istft_plan, F, C, spec, &p)) return st;
    if (Lout) *Lout = p.Lout_full;
    if (overlap) *overlap = p.overlap;
    if (chunk) *chunk = p.chunk;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return DSP_OK;
}

int dsp_istft(const float *const *spec, uint32_t C, uint64_t F, uint64_t ld, float *const *out, uint64_t Lout,
              const dsp_istft_spec *sp, const dsp_exec *ex) {
    IstftPlan p;
    int st;
    if ((st = plan_checked(istft_plan, F, C, sp, &p))) return st;
    if ((st = plan_checked(stft_cx_check_ld, true, F, ld))) return st;
    if ((st = plan_checked(istft_check_lout, p, Lout))) return st;
    if ((st = whole_rows_only(ex, "dsp_istft"))) return st;
    if ((st = spectrum_rows("dsp_istft", spec, C)) || (st = check_rows("out", out, C))) return st;
    const uint64_t span = spectrum_span(F, ld);
    if (output_rows_overlap({Rows{spec, C, span}}, {Rows{out, C, Lout}}))
        return invalid("dsp_istft: an output row overlaps an input row or another output row");
    RowCall rc(ex);
    if (rc.status) return rc.status;
    const hipStream_t s = rc.s;
    const std::vector<const float *> dspec = rc.stage.in_rows(spec, C, span);
    const std::vector<float *> dout = rc.stage.out_rows(out, C, Lout);
    if (rc.stage.status) return rc.stage.status;

    IstftArgs A{};
    if ((st = get_tw(rc.dev, s, &A.tw)) || (st = get_window(rc.dev, s, p.window, kStftCxN, kStftCxN, &A.win))) return st;
    if ((st = get_scratch(rc.dev, s, p.scratch_bytes, &A.S, kScratchIstft))) return st;
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
    return st ? st : rc.done();
}

int dsp_pvoc_plan(uint64_t F, uint32_t C, const dsp_pvoc_spec *spec, uint64_t *frames_out, uint32_t *chunk,
                  uint64_t *scratch_bytes) {
    PvocPlan p;
    if (int st = plan_checked(pvoc_plan_here, F, C, spec, &p)) return st;
    if (frames_out) *frames_out = p.frames_out;
    if (chunk) *chunk = p.chunk;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return DSP_OK;
}

int dsp_pvoc(const float *const *spec_in, uint32_t C, uint64_t F, uint64_t ld_in, float *const *spec_out,
             uint64_t ld_out, const dsp_pvoc_spec *sp, const dsp_exec *ex) {
    PvocPlan p;
    int st;
    if ((st = plan_checked(pvoc_plan_here, F, C, sp, &p))) return st;
    if ((st = plan_checked(pvoc_check_ld, F, ld_in))) return st;
    if ((st = plan_checked(pvoc_check_ld, p.frames_out, ld_out))) return st;
    if ((st = whole_rows_only(ex, "dsp_pvoc"))) return st;
    if ((st = spectrum_rows("dsp_pvoc", spec_in, C)) || (st = spectrum_rows("dsp_pvoc", spec_out, C))) return st;
    const uint64_t span_in = spectrum_span(F, ld_in);
    if (output_rows_overlap({Rows{spec_in, C, span_in}}, {Rows{spec_out, C, spectrum_span(p.frames_out, ld_out)}}))
        return invalid("dsp_pvoc: an output row overlaps an input row or another output row");
    RowCall rc(ex);
    if (rc.status) return rc.status;
    const std::vector<const float *> din = rc.stage.in_rows(spec_in, C, span_in);
    const std::vector<float *> dout = rc.stage.out_framed_rows(spec_out, C, p.frames_out, kDense, ld_out);
    if (rc.stage.status) return rc.stage.status;

    PvocArgs A{};
    float *scratch = nullptr;
    // (the A/B variant that stores every increment keeps them behind the sums)
    A.variant = g_pvoc_variant.load();
    const uint64_t inc_bytes = (A.variant & 4u) ? (uint64_t)p.rows * p.frames_out * kStftCxBins * sizeof(uint32_t) : 0;
    if ((st = get_scratch(rc.dev, rc.s, p.scratch_bytes + inc_bytes, &scratch, kScratchPvoc))) return st;
    A.S = reinterpret_cast<uint32_t *>(scratch);
    A.inc = inc_bytes ? A.S + p.scratch_bytes / sizeof(uint32_t) : nullptr;
    A.ld_in = ld_in;
    A.ld_out = rc.stage.framed_ld(kDense, ld_out);
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
        return launch_pvoc(G, rc.s);
    });
    return st ? st : rc.done();
}

int dsp_time_stretch_plan(uint64_t L, uint32_t C, const dsp_stretch_spec *spec, uint64_t *frames_in,
                          uint64_t *frames_out, uint64_t *Lout_full, uint64_t *Lout_default,
                          uint64_t *device_bytes) {
    StretchPlan p;
    if (int st = plan_checked(stretch_plan, L, C, spec, &p)) return st;
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
    int st;
    if ((st = plan_checked(stretch_plan, L, C, sp, &p))) return st;
    if (Lout == 0 || Lout > p.Lout_full) return invalid("dsp_time_stretch: needs 1 <= Lout <= N + (F' - 1) H");
    if ((st = whole_rows_only(ex, "dsp_time_stretch"))) return st;
    if ((st = check_rows("in", in, C)) || (st = check_rows("out", out, C))) return st;
    if (output_rows_overlap({Rows{in, C, L}}, {Rows{out, C, Lout}}))
        return invalid("dsp_time_stretch: an output row overlaps an input row or another output row");
    RowCall rc(ex);
    if (rc.status) return rc.status;
    if ((st = refuse_capture(rc.s, "dsp_time_stretch's pair of spectrograms (allocated per call)"))) return st;
    const std::vector<const float *> din = rc.stage.in_rows(in, C, L);
    const std::vector<float *> dout = rc.stage.out_rows(out, C, Lout);
    if (rc.stage.status) return rc.stage.status;
    StretchScratch sc;
    hipError_t me = hipMalloc(&sc.a, p.in_bytes);
    if (me == hipSuccess) me = hipMalloc(&sc.b, p.out_bytes);
    if (me != hipSuccess) {
        (void)hipGetLastError();  // the refusal is this call's answer, not a later launch's
        return hip_fail(me, "dsp_time_stretch: hipMalloc of the spectrograms");
    }
    // the three public calls on device rows, on the caller's stream
    dsp_exec dev{};
    dev.device = rc.dev;
    dev.stream = (void *)rc.s;
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
    if (!st) st = rc.stage.copy_back();
    // the spectrograms leave with the call: what was enqueued must have read them
    const hipError_t e = hipStreamSynchronize(rc.s);
    if (st) return st;
    DSPB_HIP(e);
    return finish(ex);
}

int dsp_pitch_shift_plan(uint64_t L, uint32_t C, double semitones, uint32_t H, int32_t window, uint32_t *p, uint32_t *q,
                         dsp_stretch_spec *stretch, uint64_t *padded, uint64_t *stretched, uint64_t *Lout) {
    PitchPlan pl;
    if (int st = plan_checked(pitch_plan, L, C, semitones, H, window, &pl)) return st;
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

int dsp_pitch_ratio(double semitones, uint32_t *p, uint32_t *q) { return plan_checked(pitch_ratio, semitones, p, q); }

}  // extern "C"
