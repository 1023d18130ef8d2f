// capi_bigfft.cpp -- the Plugin-free row calls on the large FFT
// (include/dspbench/dspbench.h, fft_big.hip): dsp_rfft / dsp_irfft,
// dsp_deconvolve, dsp_sweep and dsp_decay, with their plans.  They share a
// call's large-FFT context: the cached twiddle table of n and the stream's work
// buffers.  The rules of a row call are at the head of capi_rate.cpp.
#include "capi_impl.hpp"
#include "decay_host.hpp"
#include "sweep_host.hpp"

namespace dspb {

static_assert(kDecayGroup == kMaxChannels, "decay_plan sizes the scratch for launches of kMaxChannels rows");

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
    if (output_rows_overlap({Rows{in, C, Lin}}, {Rows{out, C, Lout}})) return invalid("%s", overlap_text);
    RowCall rc(ex);
    if (rc.status) return rc.status;
    const std::vector<float *> dout = rc.stage.out_rows(out, C, Lout);
    std::vector<const float *> din(C);
    for (uint32_t c = 0; c < C; ++c) din[c] = Lin ? rc.stage.in(in[c], Lin) : dout[c];
    if (rc.stage.status) return rc.stage.status;
    int st;
    BigFft f;
    if ((st = big_fft_open(n, std::min<uint32_t>(C, kMaxChannels) * rfft_scratch_bytes(n), rc.dev, rc.s, &f))) return st;
    st = for_groups(C, [&](uint32_t c0, uint32_t cn) {
        BigFftArgs A{};
        if (int e = big_fft_args(f, cn, &A)) return e;
        if (inverse) A.Lout = Lout;
        else A.L = Lin;
        A.in_aligned8 = group_rows(din, c0, cn, &A.in, 8);
        A.out_aligned8 = group_rows(dout, c0, cn, &A.out, 8);
        return inverse ? launch_big_irfft(A, rc.s) : launch_big_rfft(A, rc.s);
    });
    return st ? st : rc.done();
}

}  // namespace dspb

using namespace dspb;

extern "C" {

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
    return plan_checked(deconv_plan, Ly, Ls, C, n, scratch_bytes);
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
    if (output_rows_overlap({Rows{rec, C, Ly}, Rows{&ref, 1, Ls}}, {Rows{ir, C, ir_len}}))
        return invalid("dsp_deconvolve: ir rows overlap rec, ref or each other");
    RowCall rc(ex);
    if (rc.status) return rc.status;
    const hipStream_t s = rc.s;
    if ((st = refuse_sync_under_capture(s, "stream capture: dsp_deconvolve reads the excitation's maximum back and "
                                           "synchronises its stream")))
        return st;
    const std::vector<const float *> drec = rc.stage.in_rows(rec, C, Ly);
    const float *dref = rc.stage.in(ref, Ls);
    const std::vector<float *> dir = rc.stage.out_rows(ir, C, ir_len);
    if (rc.stage.status) return rc.stage.status;
    BigFft f;
    if ((st = big_fft_open(n, scratch_bytes, rc.dev, s, &f))) return st;
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
    return rc.done();
}

int dsp_sweep_plan(uint32_t sr, const dsp_sweep_spec *spec, uint64_t *L, double *rate) {
    SweepPlan p;
    if (plan_checked(sweep_plan, sr, spec, &p)) return DSP_ERR_INVALID;  // (every refusal is the spec's)
    if (L) *L = p.L;
    if (rate) *rate = p.rate;
    return DSP_OK;
}

int dsp_sweep(uint32_t sr, const dsp_sweep_spec *spec, float *out, uint64_t count) {
    SweepPlan p;
    if (plan_checked(sweep_plan, sr, spec, &p)) return DSP_ERR_INVALID;  // (every refusal is the spec's)
    if (count > p.L) return invalid("dsp_sweep: count %llu > L %llu", (unsigned long long)count, (unsigned long long)p.L);
    if (count && !out) return invalid("out is NULL");
    sweep_fill(sr, spec, p, out, count);
    return DSP_OK;
}

int dsp_sweep_harmonic_offset(uint32_t sr, const dsp_sweep_spec *spec, uint32_t order, double *samples) {
    SweepPlan p;
    if (plan_checked(sweep_plan, sr, spec, &p)) return DSP_ERR_INVALID;  // (every refusal is the spec's)
    if (order == 0) return invalid("dsp_sweep_harmonic_offset: order must be >= 1");
    if (samples) *samples = sweep_harmonic_offset(sr, p, order);
    return DSP_OK;
}

int dsp_decay_plan(uint64_t L, uint32_t C, uint32_t sr, const dsp_decay_spec *spec, uint32_t *n, uint32_t *P,
                   uint32_t *hop, uint32_t *bands, uint64_t *hops, uint64_t *scratch_bytes, double *fm) {
    DecayPlan p;
    if (int st = plan_checked(decay_plan, L, C, sr, spec, &p)) return st;
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
    if ((st = plan_checked(decay_plan, L, C, sr, spec, &p))) return st;
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
    const float *fp = peak, *fo = reinterpret_cast<const float *>(onset);
    if (output_rows_overlap({Rows{in, C, L}}, {Rows{fe.data(), R, 2 * p.hops}, Rows{fm.data(), moment ? R : 0u, 2 * p.hops},
                                               Rows{&fp, 1, C}, Rows{&fo, 1, 2ull * C}}))
        return invalid("dsp_decay: an output row overlaps an input row or another output row");
    RowCall rc(ex);
    if (rc.status) return rc.status;
    const hipStream_t s = rc.s;
    const std::vector<const float *> din = rc.stage.in_rows(in, C, L);
    float *dpeak = (float *)rc.stage.out_bytes(peak, sizeof(float) * C);
    unsigned long long *donset = (unsigned long long *)rc.stage.out_bytes(onset, sizeof(uint64_t) * C);
    std::vector<double *> de(R), dm(R, nullptr);
    for (uint32_t r = 0; r < R; ++r) {
        de[r] = (double *)rc.stage.out_bytes(energy[r], sizeof(double) * p.hops);
        if (moment) dm[r] = (double *)rc.stage.out_bytes(moment[r], sizeof(double) * p.hops);
    }
    if (rc.stage.status) return rc.stage.status;
    BigFft f;
    if ((st = big_fft_open(p.n, p.scratch_bytes, rc.dev, s, &f))) return st;
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
    return rc.done();
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
