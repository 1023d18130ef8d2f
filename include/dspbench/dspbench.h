/*
 * dspbench.h -- C ABI of the MI355X offline-render + spectrum path.
 *
 * libdspbench.so exports everything declared here plus every host service of
 * plugin_header.h.  Plain pointers and sizes only; no torch, no C++ types.
 *
 * What each entry point replaces in the reference (odecaux/DSP-Bench):
 *
 *   dsp_render_offline  render_audio called back to back with a fixed block
 *                       size until EOF (audio.cpp:13-175, block pump of
 *                       wasapi_audio.cpp:223-251).  The reference has no
 *                       offline renderer (README.md:16 TODO); semantics are
 *                       exactly those of SURVEY §3.1 (i)-(v), one-shot mode.
 *   dsp_stft_magnitude  windowing -> fft_forward -> pythagore_array per frame
 *                       (dsp.cpp:69-72, 74-103, 166-168) over frames of hop H.
 *   dsp_render_stft     the two above fused: render, keep the render, and
 *                       the spectrum of the rendered signal (headline path).
 *   dsp_ir_analysis     compute_IR (plugin.cpp:17-58) followed by
 *                       fft_perform_and_get_magnitude (dsp.cpp:53-66).
 *   dsp_fft_forward /   fft_forward / fft_reverse (dsp.cpp:74-132) with the
 *   dsp_fft_reverse     same split re/im layout and 1/sqrt(N) scaling.
 *
 * Plugin dispatch: a plugin reaches the GPU as a dsp_plugin.  For the stock
 * plugins whose audio_callback is a per-sample map the `kind` selects a
 * specialised kernel that reads the plugin's own parameter / state blob at
 * the struct offsets the plugin declares (gain_test: Parameters{float gain},
 * IR_test: Parameters{float gain; float step}, static_gain_plugin:
 * State{float gain}).  DSP_PLUGIN_GENERIC runs the plugin's own
 * audio_callback, compiled from its unchanged source to gfx950 code by the
 * module compiler (module.h), through the generic block driver.
 *
 * Errors: every entry point returns DSP_OK (0) or a negative dsp_status.
 * Nothing aborts; HIP errors are mapped to DSP_ERR_HIP and the HIP error
 * string is kept in dsp_last_error().
 */
#ifndef DSPBENCH_H
#define DSPBENCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): dsp_fir_method removed (DSP_EXEC_FIR_DIRECT in dsp_exec.flags
 * selects the direct form), the transport / gather-plan entry points and the
 * dsp_comm layout of shard.h, dsp_callback_facts and the fact-gated block
 * classes of module.h.  A binding written against 1 must not assume those. */
#define DSPBENCH_ABI_VERSION 3

enum dsp_status {
    DSP_OK = 0,
    DSP_ERR_INVALID = -1,     /* bad argument (null pointer, size, alignment) */
    DSP_ERR_HIP = -2,         /* a HIP runtime call failed */
    DSP_ERR_UNSUPPORTED = -3, /* valid request this build does not implement */
    DSP_ERR_NOMEM = -4,       /* device allocation failed */
    DSP_ERR_NO_DEVICE = -5    /* no gfx950 device visible */
};

/* Windows.  Symmetric convention w[n] = a - b cos(2 pi n / (N - 1)), the
 * convention of ippsWinHamming_32f (dsp.cpp:71). */
enum dsp_window {
    DSP_WIN_HAMMING = 0, /* 0.54 / 0.46: reference parity window */
    DSP_WIN_HANN = 1,    /* 0.5 / 0.5: benchmark window (BASELINE cfg 4) */
    DSP_WIN_RECT = 2
};

enum dsp_plugin_kind {
    DSP_PLUGIN_NOOP = 0,        /* test/no_op.cpp */
    DSP_PLUGIN_GAIN = 1,        /* build/gain_test.cpp: out *= params.gain (f32 @0) */
    DSP_PLUGIN_STATIC_GAIN = 2, /* test/static_gain_plugin.cpp: out *= state.gain (f32 @0) */
    DSP_PLUGIN_IR_RAMP = 3,     /* build/IR_test.cpp: out[s] = (float)g_s, g -= step (f32 @0, @4) */
    DSP_PLUGIN_FIR = 4,         /* build-defined cfg 3b: y[n] = sum_k taps[k] x[n-k], params = float taps[T],
                                   T <= 2048; state carries across blocks, so whole files only
                                   (sample_offset 0; shard by channel) */
    DSP_PLUGIN_BIQUAD = 5,      /* build-defined: a cascade of S = params_size / 20 (1..4) direct-form-I
                                   biquads, params = float {b0, b1, b2, a1, a2}[S], y = b0 x + b1 x1 +
                                   b2 x2 - a1 y1 - a2 y2 (plugins/biquad.cpp's section), zero initial
                                   state carried across blocks: whole files only (sample_offset 0;
                                   shard by channel).  Block-parallel (a state scan), fp32 within a
                                   bound of float64, not bit-exact with a serial chain; not in graphs */
    DSP_PLUGIN_CONV = 6,        /* build-defined: convolution with a long impulse response, FIR's
                                   semantics y[n] = sum_k taps[k] x[n-k] for params = float taps[T],
                                   1 <= T <= 2^20 (21.8 s at 48 kHz), finite; zero initial history
                                   carried across blocks: whole files only (sample_offset 0; shard
                                   by channel).  Uniform partitioned overlap-save on 8192-point
                                   frames (dsp_conv_plan); fp32 within a bound of float64.  Output
                                   rows must not overlap input rows (DSP_ERR_INVALID) */
    DSP_PLUGIN_GENERIC = 16     /* compiled audio_callback run on the GPU (module) */
};

typedef struct dsp_plugin {
    int32_t kind;          /* dsp_plugin_kind */
    uint32_t params_size;  /* bytes of the Parameters blob */
    const void *params;    /* host pointer to the Parameters blob */
    uint32_t state_size;   /* bytes of the State blob */
    void *state;           /* host pointer to the State blob */
    const void *module;    /* DSP_PLUGIN_GENERIC: dsp_module handle, else NULL */
} dsp_plugin;

/* Execution context (ref has none: single-threaded per audio thread). */
#define DSP_EXEC_HOST_BUFFERS 0x1u /* in/out/mag are host pointers: stage via HBM */
#define DSP_EXEC_SYNC 0x2u         /* synchronise the stream before returning */
#define DSP_EXEC_FIR_DIRECT 0x4u   /* DSP_PLUGIN_FIR: the direct form even when T <= 1025 (default:
                                      FFT overlap-save with 8192-point frames for T <= 1025, the
                                      direct form above) */
#define DSP_EXEC_NO_SPECIALIZE 0x8u /* DSP_PLUGIN_GENERIC: run the plugin's callback on every block.
                                      Default: a plugin whose callback the IR analysis proves to
                                      ignore its input (then one block, the same on every channel)
                                      or to scale it by one factor runs as that block tiled / that
                                      gain in the fused kernels (module.h dsp_callback_facts) */
#define DSP_EXEC_VERIFY_CLASS 0x10u /* DSP_PLUGIN_GENERIC rendered by a block class: afterwards run
                                      the callback on the first, the last and two more blocks of the
                                      call's own input and compare with the rendered rows bit for
                                      bit; on a mismatch render the call again with the callback on
                                      every block.  Reported through dsp_exec.result.  Costs a
                                      stream synchronisation (dsp_render_offline / dsp_render_stft).
                                      A call whose output rows overlap its input rows (in place)
                                      runs the callback on every block instead: the check and a
                                      re-render need the input after the render.  Honoured by
                                      dsp_render_offline and dsp_render_stft, and per chunk by the
                                      chunked (dsp_render_stft_host / _wav) and sharded drivers,
                                      whose result ORs their chunks' bits; dsp_render_loop with
                                      the flag runs the callback on every block (result 0) */
#define DSP_EXEC_SERIAL_STATE 0x20u /* DSP_PLUGIN_GENERIC whose callback writes its State: one chain
                                      of blocks in order on one lane, as the reference's audio thread
                                      runs them (default: speculative segments, module.h
                                      dsp_state_spec_info -- the same bits) */
#define DSP_EXEC_EVERY_FRAME 0x40u  /* dsp_render_stft, fused IR_test launch (DSP_PLUGIN_IR_RAMP, or a
                                      GENERIC plugin whose block class is one table): compute every
                                      frame's FFT.  Default: when the hop is a multiple of the block
                                      size (H % B == 0) every frame of the call holds the same
                                      samples, and a call long enough to fill the device computes
                                      the spectrum once per wave and stores it for a run of frames
                                      (DSP_RESULT_FRAME_REUSE) -- the same bits.  Outside stream
                                      capture that spectrum is kept per device between calls
                                      (DSP_RESULT_SPECTRUM_CACHE).  A GENERIC call with DSP_EXEC_VERIFY_CLASS computes
                                      every frame too */
/* the flags that choose how a call computes (not where its buffers live):
 * the chunked and sharded drivers pass them on to every chunk */
#define DSP_EXEC_METHOD_FLAGS                                                                    \
    (DSP_EXEC_FIR_DIRECT | DSP_EXEC_NO_SPECIALIZE | DSP_EXEC_VERIFY_CLASS | DSP_EXEC_SERIAL_STATE | \
     DSP_EXEC_EVERY_FRAME)

/* dsp_exec.result bits (written when result is not NULL) */
#define DSP_RESULT_CLASS 0x1u      /* a GENERIC plugin ran as its block class */
#define DSP_RESULT_VERIFIED 0x2u   /* DSP_EXEC_VERIFY_CLASS: the checked blocks matched */
#define DSP_RESULT_RERENDERED 0x4u /* DSP_EXEC_VERIFY_CLASS: a checked block differed; the call was
                                      rendered again with the callback on every block */
#define DSP_RESULT_FRAME_REUSE 0x8u /* dsp_render_stft: the fused launch computed one spectrum per
                                      run of frames (see DSP_EXEC_EVERY_FRAME); the chunked and
                                      sharded drivers OR it across their chunks */
#define DSP_RESULT_SPECTRUM_CACHE 0x10u /* dsp_render_stft, with DSP_RESULT_FRAME_REUSE: the one
                                      spectrum of the call came from the device's cache of spectrum
                                      rows (computed once per plugin block, window and block size,
                                      then kept between calls) and the launch only stored it -- the
                                      same bits.  Never under stream capture, DSP_EXEC_EVERY_FRAME
                                      or DSP_EXEC_VERIFY_CLASS */

typedef struct dsp_exec {
    int32_t device;         /* HIP device ordinal; -1 = current device */
    uint32_t flags;         /* DSP_EXEC_* */
    void *stream;           /* hipStream_t; NULL = the legacy default stream */
    uint64_t sample_offset; /* global index of in[c][0] (time-chunk shards);
                               must be a multiple of the block size B */
    uint32_t *result;       /* optional: DSP_RESULT_* of the call (NULL: not reported) */
} dsp_exec;

/* Number of frames of an STFT over L samples: L >= N ? (L - N) / H + 1 : 0. */
uint64_t dsp_stft_frame_count(uint64_t L, uint32_t N, uint32_t H);

/* DSP_PLUGIN_BIQUAD's plan for a cascade (host only, no device): *window =
 * the number of preceding 2048-sample tiles whose end state still reaches a
 * tile's entering state above 2^-48 (1..192: the render sums exactly those, in
 * a fixed order, and is bitwise reproducible run to run), or 0 for a cascade
 * that does not decay that fast (a chained look-back: within the same error
 * bound, not bitwise reproducible).  DSP_ERR_INVALID for a bad blob. */
int dsp_biquad_plan(const float *coef, uint32_t sections, uint32_t *window);

/* DSP_PLUGIN_CONV's plan (host only, no device): partitions of the filter,
 * frames of the call, and the device scratch bytes one channel group needs.
 * partitions = ceil(taps / 4096); frames = ceil(ceil(L / B) B / 4096);
 * scratch_bytes = 2 min(C, 16) frames 33792 (the input's and the output's
 * spectra; channel groups of 16 run one after another over the same scratch,
 * which the render keeps per stream).  Any out pointer may be NULL.
 * DSP_ERR_INVALID for taps = 0, taps > 2^20 or B = 0. */
int dsp_conv_plan(uint32_t taps, uint64_t L, uint32_t B, uint32_t C,
                  uint32_t *partitions, uint64_t *frames, uint64_t *scratch_bytes);

/* Sample-rate conversion: a polyphase Kaiser-windowed sinc, zero-phase.
 *
 * With g = gcd(sr_in, sr_out): up = sr_out / g, down = sr_in / g.  A quality
 * spec is zeros Z (zero crossings each side, 4..64), the Kaiser beta (0..20)
 * and rolloff (0.5..1); a NULL spec is Z = 64, beta = 14.769656459379492,
 * rolloff = 0.9475937167399596 ("kaiser best").
 *   rho = rolloff min(1, up / down), W = Z / rho, half = ceil(W),
 *   taps per phase Tp = 2 half,
 *   h(u) = rho sinc(rho u) I0(beta sqrt(1 - (u / W)^2)) / I0(beta) for |u| < W,
 *          0 otherwise (sinc(t) = sin(pi t) / (pi t)),
 *   table[phi][i] = (float)h(half - 1 - i + phi / up), phi < up, i < Tp
 *                   (float64, rounded once),
 *   Lout = ceil(L up / down),
 *   y[m] = sum_{i < Tp} table[phi][i] x[n0 - half + 1 + i], q = m down (64-bit),
 *          n0 = q / up, phi = q % up, x = 0 outside [0, L).
 * Output m sits at input time m down / up: no delay to compensate.  The sum's
 * order is the kernel's own (fp32, within a bound of float64; taps outside an
 * output's window enter as zero products, so samples must be finite).
 * sr_in == sr_out is a copy, bit for bit, with no filter.
 *
 * Refused with DSP_ERR_UNSUPPORTED: up > 4096, Tp > 8192, a table (up Tp
 * floats) above 8 MiB, L up >= 2^63.  Every pair of the standard rates 8000,
 * 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000,
 * 176400, 192000 plans at the default quality: none is refused (the largest
 * are 192000 -> 8000, Tp = 3242, and 192000 -> 11025, a 1.4 MB table;
 * tests/test_resample_plan.py checks the list against dsp_resample_plan). */
typedef struct dsp_resample_spec {
    uint32_t zeros;  /* 4..64 */
    double beta;     /* 0..20 */
    double rolloff;  /* 0.5..1 */
} dsp_resample_spec;

/* The plan of a conversion (host only, no device).  Any out pointer may be
 * NULL.  DSP_ERR_INVALID for a rate of 0 or a spec outside its ranges;
 * DSP_ERR_UNSUPPORTED as above. */
int dsp_resample_plan(uint32_t sr_in, uint32_t sr_out, uint64_t L, const dsp_resample_spec *spec,
                      uint32_t *up, uint32_t *down, uint32_t *taps_per_phase, uint64_t *Lout,
                      uint64_t *table_bytes);

/* The conversion's table[phi][i], up rows of Tp floats, as the device uses it
 * (host only).  count must be up Tp (DSP_ERR_INVALID otherwise). */
int dsp_resample_taps(uint32_t sr_in, uint32_t sr_out, const dsp_resample_spec *spec, float *table,
                      uint64_t count);

/* Converts C rows of L samples at sr_in into rows of Lout samples at sr_out
 * (Lout must equal the plan's).  Device rows, or host rows with
 * DSP_EXEC_HOST_BUFFERS.  Output rows must not overlap input rows and
 * ex->sample_offset must be 0 (DSP_ERR_INVALID).  L = 0 is DSP_OK and writes
 * nothing.  The device table is cached per device by (up, down, spec); a
 * stream being captured needs one eager call of the conversion first. */
int dsp_resample(const float *const *in, uint32_t C, uint64_t L, float *const *out, uint64_t Lout,
                 uint32_t sr_in, uint32_t sr_out, const dsp_resample_spec *spec, const dsp_exec *ex);

/* Programme loudness (ITU-R BS.1770-4 / EBU R128), loudness range (EBU Tech
 * 3342) and true peak of C rows of L samples at rate sr.
 *
 * Hop and blocks: hop = (sr + 5) / 10 samples (100 ms); hop j holds samples
 * [j hop, (j + 1) hop); hops = L / hop (a ragged tail takes no part in the
 * loudness, but it does in the peaks).  Momentary block i is hops i .. i + 3
 * (400 ms, 75 % overlap): blocks = hops >= 4 ? hops - 3 : 0.  Short-term
 * block i is hops i .. i + 29 (3 s).  8000 <= sr <= 384000; any other rate is
 * DSP_ERR_UNSUPPORTED.
 *
 * K-weighting: two direct-form-I sections {b0, b1, b2, a1, a2} with
 * DSP_PLUGIN_BIQUAD's equation, as a cascade, zero initial state; the
 * coefficients are computed in float64 and rounded once to float:
 *   stage 1: f0 = 1681.974450955533, G = 3.999843853973347 dB,
 *            Q = 0.7071752369554196, K = tan(pi f0 / sr), Vh = 10^(G / 20),
 *            Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2,
 *            b0 = (Vh + Vb K / Q + K^2) / a0, b1 = 2 (K^2 - Vh) / a0,
 *            b2 = (Vh - Vb K / Q + K^2) / a0,
 *            a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0
 *   stage 2: f0 = 38.13547087602444, Q = 0.5003270373238773,
 *            K = tan(pi f0 / sr), a0 = 1 + K / Q + K^2, b = {1, -2, 1},
 *            a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0
 * (at sr = 48000 these are BS.1770-4's table to every printed digit).
 * Samples must be finite.
 *
 * Hop energy: z[c][j] = sum over hop j of y_c[n]^2 (a double: the sum, not the
 * mean), y_c the K-weighted channel (fp32 on the device, within a bound of
 * float64; the same bits on every run).
 *
 * Gating (BS.1770-4), with weights G_c (NULL: 1 for every channel; a caller
 * passes 1.41 for surrounds and 0 for LFE):
 *   w_i = sum_c G_c (z[c][i] + .. + z[c][i + 3]) / (4 hop),
 *   l_i = -0.691 + 10 log10 w_i;
 *   absolute gate l_i > -70; relative gate l_i > -0.691 + 10 log10(mean of w
 *   over the absolute-gated blocks) - 10;
 *   integrated = -0.691 + 10 log10(mean of w over the blocks that pass both),
 *   -HUGE_VAL if none does.  momentary_max = max l_i; short_term_max the same
 *   over the 3 s blocks; both -HUGE_VAL where there is no block.
 * Range (EBU Tech 3342): the short-term loudness of every 3 s block (hop
 *   100 ms); keep those above -70, then those above (the mean power of the
 *   kept ones, in LUFS) - 20; sorted ascending s[0 .. n):
 *   range = s[(size_t)((n - 1) 0.95 + 0.5)] - s[(size_t)((n - 1) 0.10 + 0.5)],
 *   0 where n = 0.
 * Peaks: sample_peak = max over c, n of |x_c[n]|; true_peak = max over c, m of
 *   |y_c[m]|, y = dsp_resample's definition for sr -> ovs sr with the caller's
 *   dsp_resample_spec (NULL: the library default), ovs = 4 for sr < 88200,
 *   2 for sr < 176400, else 1 (then true_peak = sample_peak).  The oversampled
 *   signal is never stored. */
typedef struct dsp_loudness_result {
    double integrated;      /* LUFS */
    double range;           /* LU */
    double momentary_max;   /* LUFS */
    double short_term_max;  /* LUFS */
    double sample_peak;     /* linear */
    double true_peak;       /* linear; NaN without DSP_LOUDNESS_TRUE_PEAK */
    uint64_t blocks;        /* momentary blocks */
    uint64_t gated_blocks;  /* of them, those that pass both gates */
} dsp_loudness_result;

#define DSP_LOUDNESS_TRUE_PEAK 0x1u /* dsp_loudness flags: run the oversampled pass */

/* The plan of a measurement (host only, no device): hop, hops and oversample
 * as above, kcoef = the two sections' ten floats, scratch_bytes = the device
 * scratch one channel group of 16 takes (kept per stream).  Any out pointer
 * may be NULL.  DSP_ERR_UNSUPPORTED for a rate outside 8000..384000. */
int dsp_loudness_plan(uint32_t sr, uint64_t L, uint32_t *hop, uint64_t *hops, uint32_t *oversample,
                      float kcoef[10], uint64_t *scratch_bytes);

/* Gating, maxima and range from hop energies (host only): hop_energy is C rows
 * of `hops` doubles.  Fills integrated, range, momentary_max, short_term_max,
 * blocks and gated_blocks; leaves the peaks alone.  DSP_ERR_INVALID for C = 0,
 * hop = 0, a NULL row (with hops > 0) or a NULL res. */
int dsp_loudness_gate(const double *const *hop_energy, uint32_t C, uint64_t hops, uint32_t hop,
                      const float *weights, dsp_loudness_result *res);

/* Measures C rows of L samples: device rows, or host rows with
 * DSP_EXEC_HOST_BUFFERS.  hop_energy (optional): host rows, C of `hops`
 * doubles.  chan_peaks (optional): host double[2 C], sample then true peak per
 * channel (the true peak NaN without DSP_LOUDNESS_TRUE_PEAK).  *res is exactly
 * dsp_loudness_gate of the call's own hop energies, plus the peaks.  The call
 * returns host values: it synchronises its stream, and refuses a stream that
 * is being captured.  L = 0 or hops < 4 is DSP_OK with integrated -HUGE_VAL.
 * DSP_ERR_INVALID for C = 0, a NULL row, a NULL res or a non-zero
 * sample_offset; DSP_ERR_UNSUPPORTED for the rate. */
int dsp_loudness(const float *const *in, uint32_t C, uint64_t L, uint32_t sr, const float *weights,
                 uint32_t flags, const dsp_resample_spec *tp_spec, double *const *hop_energy,
                 double *chan_peaks, dsp_loudness_result *res, const dsp_exec *ex);

/* Look-ahead peak limiter, offline and zero-latency: C rows of L finite samples
 * at rate sr come out as C rows of L samples with |y| <= ceiling, no delay.
 *
 * Spec: ceiling c > 0 (linear, finite); lookahead A in samples, 0..1024;
 * release tau in samples, 0 (none) or 1..2^22; flags DSP_LIMITER_*.
 * Channels form link groups: one group of all C channels, or with
 * DSP_LIMITER_UNLINKED one group per channel.  Per group:
 *   1. detector   p[n] = max over the group's channels of |x_c[n]|; with
 *                 DSP_LIMITER_TRUE_PEAK of max(|x_c[n]|, max_{phi < ovs}
 *                 |u_c[ovs n + phi]|), u = dsp_resample's y for sr -> ovs sr
 *                 with the caller's dsp_resample_spec (NULL: the default), ovs
 *                 as in dsp_loudness (4 / 2 / 1; at 1 the flag changes
 *                 nothing).  The oversampled signal is never stored.
 *   2. needed     a[n] = p[n] > c ? 1 - c / p[n] : 0 (fp32, IEEE division);
 *                 a[n] = 0 for n >= L.
 *   3. hold       h[n] = max_{n <= j <= n + A} a[j].
 *   4. release    e[n] = max(h[n], rho e[n - 1]), e[-1] = 0,
 *                 rho = (float)exp(-1 / tau) (float64, rounded once), 0 for
 *                 tau = 0.
 *   5. attack     s[n] = sum_{k = 0..A} w[k] e[n - k], e[j] = 0 for j < 0,
 *                 w[k] = (float)(v_k / sum v), v_k = sin^2(pi (k + 1) / (A + 2))
 *                 (float64); A = 0: w = {1}.
 *   6. output     g[n] = 1 - s[n]; y_c[n] = min(max(x_c[n] g[n], -c), c).
 * Every e[j], j in [n - A, n], is >= a[n], so in exact arithmetic g[n] <=
 * c / p[n]: the clamp of step 6 absorbs rounding only, and makes |y| <= c hold
 * bit for bit.  Where max |x| <= c the call is the identity (g = 1.0f, y = x
 * bit for bit).  The device's e and s are fp32 within a bound of the float64
 * definition (the decays of step 4 are powers of rho rounded once, the sum of
 * step 5 runs k = 0..A in order); the same bits on every run, and for a
 * prefix of the rows the same bits wherever the definition's are the same.
 * With a true-peak detector the output's true peak is lowered to about the
 * ceiling, not guaranteed below it: the gain varies between samples. */
typedef struct dsp_limiter_spec {
    float ceiling;      /* linear, > 0 */
    uint32_t lookahead; /* samples, 0..1024 */
    double release;     /* samples: 0, or 1..2^22 */
    uint32_t flags;     /* DSP_LIMITER_* */
} dsp_limiter_spec;

#define DSP_LIMITER_UNLINKED 0x1u  /* one link group per channel */
#define DSP_LIMITER_TRUE_PEAK 0x2u /* the oversampled detector */

typedef struct dsp_limiter_result {
    double min_gain;  /* min over groups and n of g[n]; 1 for L = 0 */
    uint64_t limited; /* the number of (group, n) with g[n] < 1 */
} dsp_limiter_result;

/* The plan of a call (host only, no device): link groups, the detector's
 * oversampling, rho, the window w[0..A] (A + 1 floats) and the bytes of device
 * scratch the call takes (kept per stream).  Any out pointer may be NULL.
 * DSP_ERR_INVALID for C = 0, a NULL spec, a ceiling that is not finite and
 * positive, A > 1024, a release outside its range, unknown flags, or (with
 * DSP_LIMITER_TRUE_PEAK) a resample spec outside its ranges;
 * DSP_ERR_UNSUPPORTED with DSP_LIMITER_TRUE_PEAK for what dsp_loudness refuses
 * (a rate outside 8000..384000). */
int dsp_limiter_plan(uint32_t sr, uint64_t L, uint32_t C, const dsp_limiter_spec *spec,
                     const dsp_resample_spec *tp_spec, uint32_t *groups, uint32_t *oversample, float *rho,
                     float *window, uint64_t *scratch_bytes);

/* Limits C rows of L samples: device rows, or host rows with
 * DSP_EXEC_HOST_BUFFERS.  out[c] == in[c] (in place) is allowed; any other
 * overlap between out, in, gain and detector rows is DSP_ERR_INVALID.  gain and
 * detector (optional): one row of L floats per link group, g[n] and p[n].
 * ex->sample_offset must be 0.  L = 0 is DSP_OK and writes nothing.  Without
 * res the call is stream-ordered and does not synchronise; its device table is
 * cached per device, so a stream being captured needs one eager call of the
 * same shape first.  With res the call synchronises its stream and refuses a
 * stream that is being captured.  DSP_ERR_NO_DEVICE without a device. */
int dsp_limiter(const float *const *in, uint32_t C, uint64_t L, float *const *out, uint32_t sr,
                const dsp_limiter_spec *spec, const dsp_resample_spec *tp_spec, float *const *gain,
                float *const *detector, dsp_limiter_result *res, const dsp_exec *ex);

/* Large real FFT: n a power of two, 2^10 <= n <= 2^24.  in[c] holds L <= n
 * samples; the rest of the frame is zero and is never read from memory.
 * spec[c] holds n / 2 + 1 bins as interleaved (re, im) floats in natural order.
 *   forward  X[k] = sum_j x[j] e^{-2 pi i j k / n}   (unnormalised)
 *   inverse  x[j] = 1/n sum_k X[k] e^{+2 pi i j k / n}, the first Lout <= n
 *            samples written; bins 0 and n / 2 use only their real part.
 * This is numpy's rfft / irfft convention.  It is NOT dsp_fft_forward's
 * 1 / sqrt(n) in both directions, which stays as the reference-parity service
 * for n <= 8192.
 * Method: z[j] = x[2j] + i x[2j+1], an M = n / 2 point complex transform as 2..4
 * Stockham passes (the plan, a pure function of n: radices 64, 32 and 8,
 * largest first), then the real split.  Inter-pass twiddles come from a
 * two-level table W_n^K = hi[K >> 12] lo[K & 4095] computed in float64 and
 * rounded once, cached per device by n: a stream being captured needs one eager
 * call of the same n first.  No float atomics, a fixed summation order: the
 * same bits on every run, and channel c's bits do not depend on C.  Channel
 * groups of at most 16 run one after another over a scratch kept per stream.
 * ex->sample_offset must be 0; output rows must not overlap input rows
 * (DSP_ERR_INVALID); host rows with DSP_EXEC_HOST_BUFFERS; L = 0 gives a zero
 * spectrum.  DSP_ERR_NO_DEVICE without a device. */
/* The plan (host only, no device): the pass count, radix[0..passes) (the rest
 * 0; their product is n / 2) and the scratch bytes per channel.  Any out
 * pointer may be NULL.  DSP_ERR_INVALID for an n that is no power of two in
 * [2^10, 2^24]. */
int dsp_rfft_plan(uint32_t n, uint32_t *passes, uint32_t radix[4], uint64_t *scratch_bytes_per_channel);
int dsp_rfft(const float *const *in, uint32_t C, uint64_t L, uint32_t n, float *const *spec, const dsp_exec *ex);
int dsp_irfft(const float *const *spec, uint32_t C, uint32_t n, float *const *out, uint64_t Lout,
              const dsp_exec *ex);

/* Deconvolution by regularised spectral division: the impulse response between
 * an excitation ref (one row of Ls samples, used for every channel) and C
 * recordings rec[c] of Ly samples.  n = max(1024, the next power of two >=
 * max(Ly, Ls)); beyond 2^24 DSP_ERR_UNSUPPORTED.  With Y_c = rfft_n(rec[c]) and
 * S = rfft_n(ref):
 *   lambda   = (float)eps * max_k |S[k]|^2
 *   H_c[k]   = Y_c[k] conj(S[k]) / (|S[k]|^2 + lambda)
 *   h_c      = irfft_n(H_c)
 *   ir[c][i] = h_c[(i - pre) mod n],  i < ir_len,  pre <= ir_len <= n
 * so the first `pre` output samples are negative time: where the harmonic
 * responses of a swept-sine measurement land (dsp_sweep_harmonic_offset).
 * The maximum is an integer atomic max over the bit patterns of the
 * non-negative |S|^2 (order-preserving, deterministic); the division is one
 * pointwise launch between the transforms.  A spec of NULL is eps = 1e-6,
 * pre = 0.  DSP_ERR_INVALID for eps not finite or outside [1e-12, 1], Ly = 0,
 * Ls = 0, C = 0, pre > ir_len, ir_len > n, a ref whose spectrum is all zeros
 * (nothing is written), and any overlap of ir rows with rec, ref or each other.
 * The call reads the maximum back: it synchronises its stream once, and
 * refuses a stream that is being captured.  ex->sample_offset must be 0. */
typedef struct dsp_deconv_spec {
    double eps;   /* 1e-12 .. 1 */
    uint32_t pre; /* output samples of negative time */
} dsp_deconv_spec;

/* The plan (host only): n and the bytes of device scratch (kept per stream). */
int dsp_deconv_plan(uint64_t Ly, uint64_t Ls, uint32_t C, uint32_t *n, uint64_t *scratch_bytes);
int dsp_deconvolve(const float *const *rec, uint32_t C, uint64_t Ly, const float *ref, uint64_t Ls,
                   float *const *ir, uint64_t ir_len, const dsp_deconv_spec *spec, const dsp_exec *ex);

/* The excitation: an exponential sine sweep (Farina), host only, float64
 * rounded once.  With R = ln(f2 / f1), T = seconds, L = round(T sr):
 *   x[i] = amplitude sin(2 pi f1 T / R (e^{(i / sr) R / T} - 1)),  i < L
 * times a raised-cosine fade 0.5 - 0.5 cos(pi (i + 0.5) / fade) over `fade`
 * samples at each end.  Deconvolved by the sweep, the response of harmonic
 * order m sits T ln(m) / R seconds before the linear one.
 * DSP_ERR_INVALID unless 0 < f1 < f2 <= sr / 2, seconds > 0, 1 <= L <= 2^24,
 * 2 fade <= L and amplitude is finite; dsp_sweep also for count > L. */
typedef struct dsp_sweep_spec {
    double f1, f2, seconds, amplitude;
    uint32_t fade;
} dsp_sweep_spec;

int dsp_sweep_plan(uint32_t sr, const dsp_sweep_spec *spec, uint64_t *L, double *rate /* ln(f2/f1)/T */);
int dsp_sweep(uint32_t sr, const dsp_sweep_spec *spec, float *out, uint64_t count);
/* order >= 1; *samples = T ln(order) / R sr */
int dsp_sweep_harmonic_offset(uint32_t sr, const dsp_sweep_spec *spec, uint32_t order, double *samples);

/* Welch spectral estimates: the average spectrum of C rows of L samples and,
 * with a reference row, the cross-spectrum from which the transfer function
 * (H1) and the coherence follow -- the noise or programme-material measurement
 * beside the sweep's (dsp_deconvolve).
 *
 * N = 8192 only (any other N: DSP_ERR_UNSUPPORTED).  F = dsp_stft_frame_count(
 * L, N, H) frames with 1 <= H <= N, frame f over [f H, f H + N): no padding and
 * no detrend, a tail shorter than a frame is ignored.  w is DSP_WIN_HAMMING or
 * DSP_WIN_HANN, the symmetric table of dsp_stft_magnitude (not scipy's periodic
 * default).  With X_{c,f} = DFT_N(w in[c][f H ..)), unnormalised, K = 4097
 * bins, and R_f the same of the optional row ref (L samples, shared by every
 * channel as in dsp_deconvolve), the call returns raw sums as float64 rows:
 *   sxx[c][k]             = sum_f |X_{c,f}[k]|^2           C rows of K
 *   srr[k]                = sum_f |R_f[k]|^2               one row of K
 *   sxy[c][2k], [2k + 1]  = sum_f conj(R_f[k]) X_{c,f}[k]  C rows of 2 K, (re, im)
 * sxy has the sign of scipy.signal.csd(ref, in).  srr and sxy are written only
 * with a ref and must be NULL exactly when ref is NULL.
 * Summation order (part of the contract): the frames are cut into runs of `run`
 * consecutive frames, a constant of the plan; a run is summed in float32 in
 * frame order, the runs are added in float64 in run order.  No float atomics:
 * the same bits on every run, and channel c's bits do not depend on C.  When
 * in[c] holds the same samples as ref, the imaginary parts of sxy[c] are
 * exactly 0.  Accuracy: per row max_k |S - exact| <= 1.5e-6 max_k exact (for sxy
 * the scale is sqrt(max sxx max srr)) for finite samples; non-finite samples
 * give undefined sums.
 * Method: the frames are walked in chunks; a chunk's windowed transforms go to
 * a device scratch kept per stream, a second launch sums the runs, a third adds
 * them onto the output rows.  The scratch holds at most 64 MiB of spectra and
 * never more than 72 MiB in all, whatever L is.
 * DSP_ERR_INVALID for C = 0, F = 0 (L < N), H = 0 or H > N, an unknown window,
 * ex->sample_offset != 0, srr / sxy not matching ref, an output row that is
 * not 8-byte aligned, or any overlap of an output row with an input row or
 * another output row (nothing is written).  Host rows with
 * DSP_EXEC_HOST_BUFFERS.  Channel groups of at most 16 run one after another
 * over the scratch.  The window and twiddle tables are cached per device: a
 * stream being captured needs one eager call of the same shape first.
 * DSP_ERR_NO_DEVICE without a device. */
typedef struct dsp_welch_spec {
    uint32_t N;     /* 8192 */
    uint32_t H;     /* 1 .. N */
    int32_t window; /* DSP_WIN_HAMMING or DSP_WIN_HANN */
} dsp_welch_spec;   /* NULL: {8192, 4096, DSP_WIN_HANN} */

/* The plan (host only, no device): frames F, bins K, the run length, the bytes
 * of device scratch, and win_sum = sum w, win_sumsq = sum w^2 in float64 over
 * the float table the kernel reads.  Any out pointer may be NULL. */
int dsp_welch_plan(uint64_t L, uint32_t C, int has_ref, const dsp_welch_spec *spec, uint64_t *frames,
                   uint32_t *bins, uint32_t *run, uint64_t *scratch_bytes, double *win_sum, double *win_sumsq);
int dsp_welch(const float *const *in, uint32_t C, uint64_t L, const float *ref /* may be NULL */,
              double *const *sxx, double *srr, double *const *sxy, const dsp_welch_spec *spec, const dsp_exec *ex);

/* From the sums to the estimates (host only, float64); any output may be NULL,
 * srr and sxy may be NULL when H1 and coherence are.
 *   psd[c][k]       = g_k sxx[c][k] / (frames sr win_sumsq), g = 2 except at DC
 *                     and Nyquist (k = 0, bins - 1): one-sided, scipy's
 *                     scaling='density'.  DSP_WELCH_SPECTRUM divides by
 *                     frames win_sum^2 instead (scaling='spectrum').
 *   H1[c][2k], +1   = sxy[c][k] / srr[k]
 *   coherence[c][k] = |sxy[c][k]|^2 / (sxx[c][k] srr[k])
 * A bin whose denominator is 0 gives H1 = 0 and coherence = 0.
 * DSP_ERR_INVALID for C = 0, bins = 0, frames = 0, unknown flags, a NULL input
 * an output needs, or (for psd) a scale that is not finite and positive. */
#define DSP_WELCH_SPECTRUM 0x1u
int dsp_welch_derive(const double *const *sxx, const double *srr, const double *const *sxy, uint32_t C,
                     uint32_t bins, uint64_t frames, double sr, double win_sum, double win_sumsq, uint32_t flags,
                     double *const *psd, double *const *H1, double *const *coherence);

/* The complex STFT and its overlap-add inverse: the pair a spectral process
 * (a mask, a time-varying EQ, the phase vocoder dsp_pvoc below) stands between.
 * torch.stft(x,
 * 8192, H, window=w, center=False, return_complex=True) is dsp_stft's result
 * transposed to [bins][frames], with w the library's symmetric table.
 *
 * N = 8192 only (any other N: DSP_ERR_UNSUPPORTED).  w is DSP_WIN_HAMMING or
 * DSP_WIN_HANN, the symmetric float table of dsp_stft_magnitude and dsp_welch.
 * Frames are dsp_stft_frame_count(L, N, H)'s: frame f over [f H, f H + N), no
 * padding, no centring, a tail shorter than a frame is ignored.  K = 4097 bins.
 * Normalisation is numpy's (dsp_rfft's): unnormalised forward, 1 / N inverse.
 *
 * dsp_stft, 1 <= H <= N:
 *   spec[c][f ld + 2 k], [.. + 1] = (re, im) of
 *   X_{c,f}[k] = sum_j w[j] in[c][f H + j] e^(-2 pi i j k / N),  k <= 4096.
 * ld is in floats, even and >= 2 K = 8194 (the plan's min_ld); floats [2 K, ld)
 * of a frame are not written.  Rows of spec must be 8-byte aligned; input rows
 * need only be floats.  The imaginary parts of bins 0 and 4096 are written as
 * +0.  One launch, no scratch: one wavefront per (frame, row), each bin written
 * once from registers.  Accuracy: per frame max_k |X - exact| <= 1.1e-6 max_k
 * |exact| for finite samples.  The same bits on every run; channel c's bits do
 * not depend on C; scaling the samples by a power of two scales the result
 * exactly (underflow aside).
 *
 * dsp_istft, 512 <= H <= N (a smaller H: DSP_ERR_UNSUPPORTED), the
 * least-squares (Griffin-Lim) inverse with the same window for synthesis.  With
 * v_f = irfft_N(spec_f), bins 0 and 4096 taken by their real part only (as
 * dsp_irfft), and Lout_full = N + (F - 1) H:
 *   num[i] = sum_f w[i - f H] v_f[i - f H]     den[i] = sum_f w[i - f H]^2
 *   out[c][i] = den[i] < floor ? 0 : num[i] / den[i],   i < Lout <= Lout_full
 * over the frames f that cover i, at most overlap = ceil(N / H) <= 16 of them.
 * floor must be finite and in [1e-12, 1]; a Hann window's zero ends make den 0
 * at the first and last samples, which is what floor is for.
 * Summation order (part of the contract): w v_f is one float32 product; num
 * adds them in float32 in ascending frame order; den adds w^2 in float32 in the
 * same order, each step one fused multiply-add; the quotient is one correctly
 * rounded float32 division, den compared with floor rounded to float32.  No
 * float atomics: the same bits on every run, and channel c's bits do not depend
 * on C.  A sample whose exact den lies within a factor 2 of floor may come out
 * either way; everything else follows the rule.  Accuracy: per row
 * |out[i] - exact[i]| <= 1.1e-6 A[i] max_f max_j |v_f[j]| with the noise gain
 * A[i] = sum_f |w[i - f H]| / den[i], for finite spectra.
 * Method: the frames are walked in chunks of `chunk` frames; one launch
 * inverts a chunk's frames, one wavefront each, and writes w v_f to a device
 * scratch kept per stream; a second launch, one thread per output sample, sums
 * and divides.  A chunk's first launch also inverts again the up to overlap - 1
 * frames before the chunk that its samples still touch, so no sum straddles two
 * launches.  chunk is the largest count with min(C, 16) chunk 32 KiB <= 64 MiB.
 *
 * Both: DSP_ERR_INVALID (nothing written) for C = 0, no frame (L < N, F = 0),
 * H = 0 or H > N, an unknown window, a floor out of range, ld odd or < 8194,
 * Lout = 0 or Lout > Lout_full, ex->sample_offset != 0, a spectrum row that is
 * not 8-byte aligned, or any overlap of an output row with an input row or
 * another output row.  Host rows with DSP_EXEC_HOST_BUFFERS.  Channel groups of
 * at most 16 run one after another.  The window and twiddle tables are cached
 * per device: a stream being captured needs one eager call of the same shape
 * first.  DSP_ERR_NO_DEVICE without a device. */
typedef struct dsp_stft_spec {
    uint32_t N;     /* 8192 */
    uint32_t H;     /* 1 .. N */
    int32_t window; /* DSP_WIN_HAMMING or DSP_WIN_HANN */
} dsp_stft_spec;    /* NULL: {8192, 4096, DSP_WIN_HANN} */
typedef struct dsp_istft_spec {
    uint32_t N;     /* 8192 */
    uint32_t H;     /* 512 .. N */
    int32_t window; /* DSP_WIN_HAMMING or DSP_WIN_HANN */
    double floor;   /* 1e-12 .. 1 */
} dsp_istft_spec;   /* NULL: {8192, 4096, DSP_WIN_HANN, 1e-10} */

/* The plans (host only, no device).  Any out pointer may be NULL.
 * dsp_stft_plan: frames F, bins K = 4097, min_ld = 2 K floats.
 * dsp_istft_plan: Lout_full, overlap, chunk, and the bytes of device scratch:
 * min(C, 16) min(F, chunk + overlap - 1) frames of 32 KiB. */
int dsp_stft_plan(uint64_t L, uint32_t C, const dsp_stft_spec *spec, uint64_t *frames, uint32_t *bins,
                  uint64_t *min_ld);
int dsp_stft(const float *const *in, uint32_t C, uint64_t L, float *const *spec, uint64_t ld,
             const dsp_stft_spec *sp, const dsp_exec *ex);
int dsp_istft_plan(uint64_t F, uint32_t C, const dsp_istft_spec *spec, uint64_t *Lout, uint32_t *overlap,
                   uint32_t *chunk, uint64_t *scratch_bytes);
int dsp_istft(const float *const *spec, uint32_t C, uint64_t F, uint64_t ld, float *const *out, uint64_t Lout,
              const dsp_istft_spec *sp, const dsp_exec *ex);

/* The phase vocoder: the spectral process that changes a spectrogram's frame
 * count, and with dsp_stft before and dsp_istft after it a file's duration
 * (dsp_time_stretch) or, with dsp_resample after that, its pitch.
 *
 * dsp_pvoc.  spec_in[c] holds F frames and spec_out[c] F' frames in dsp_stft's
 * layout: K = 4097 (re, im) pairs per frame, ld_in and ld_out in floats, even
 * and >= 8194, rows 8-byte aligned; floats [2 K, ld_out) of an output frame are
 * not written.  rate is finite and in [1/8, 8]; above 1 the output is shorter.
 * Output frame t reads at s_t = fl64(t rate), one float64 product, and F' is
 * the number of t >= 0 with s_t < F (ceil(F / rate) up to that rounding; the
 * plan counts it exactly).  With f = floor(s_t), a = float32(s_t - f) and
 * Z[F] = Z[F + 1] = 0, per bin k <= 4096, all bins alike as complex values:
 *   mag_t       = (1 - a) |Z[f]| + a |Z[f + 1]|
 *   phase_0     = arg Z[0]
 *   phase_{t+1} = phase_t + arg(Z[f + 1] conj Z[f])        (mod one turn)
 *   Z'[t]       = mag_t (cos phase_t, sin phase_t)
 * with arg 0 = 0 (an increment is 0 where either bin is 0).  This is
 * librosa.phase_vocoder's recurrence: its expected advance cancels modulo a
 * turn, so no hop enters.
 * Arithmetic (part of the contract).  A phase is a 32-bit fixed-point fraction
 * of a turn.  The argument of an input bin is computed in float32 as turns in
 * [-1/2, 1/2] and rounded to nearest into that format, +1/2 and -1/2 being the
 * same word; an increment is the wrapping 32-bit difference of the two
 * arguments, and the phase their wrapping sum.  Integer addition is
 * associative, so the sum over t is cut into chunks of `chunk` output frames
 * and gives the same bits however it is cut: the same bits on every run,
 * channel c's bits do not depend on C, frame t's bits do not depend on how
 * many frames follow it, no float atomics, and no workgroup waits for
 * another.  |Z|, the interpolation, cos and sin are float32; scaling Z by a
 * power of two scales Z' exactly (overflow of |Z|^2 and underflow aside); an
 * all-zero spectrogram gives +0.  Accuracy against the same recurrence in
 * float64 on the same float32 input: per bin |Z'[t] - exact| <= 6.2e-7 sqrt(t + 1)
 * mag_t plus a float32 ulp of the frame's largest magnitude.
 * Method: three launches per channel group.  Per (chunk, 64 neighbouring bins)
 * the integer sum of the chunk's increments goes to a device scratch kept per
 * stream, [row][chunk][4097] uint32; one thread per (row, bin) turns the sums
 * into each chunk's starting phase; the third launch forms the increments
 * again, carries the phase and writes every output bin once.  chunk = 64.
 * DSP_ERR_INVALID (nothing written) for C = 0, F = 0, a NULL spec, a rate that
 * is not finite or outside [1/8, 8], an odd or short ld, a NULL or misaligned
 * row, ex->sample_offset != 0, or any overlap of an output row with an input
 * row or another output row; DSP_ERR_UNSUPPORTED for F > 2^48.  Host rows with
 * DSP_EXEC_HOST_BUFFERS.  Channel groups of at most 16 run one after another.
 * The scratch is made on first use: a stream being captured needs one eager
 * call of the same shape first.  DSP_ERR_NO_DEVICE without a device.
 *
 * dsp_time_stretch: dsp_stft(N, H, window), dsp_pvoc(rate), dsp_istft(N, H,
 * window, floor) over two dense device spectrograms of min(C, 16) rows
 * (frames_in and frames_out frames of 8194 floats; device_bytes is their sum:
 * about 5.5 GB per stereo hour and spectrogram at H = 2048).  They are
 * allocated for the call and freed after it, so this call synchronises its
 * stream and cannot be captured into a graph (DSP_ERR_INVALID on a capturing
 * stream); DSP_ERR_NOMEM when they cannot be had.  N = 8192; 512 <= H <= 8192
 * and the floor rule are dsp_istft's.  Lout_full = N + (F' - 1) H and
 * Lout_default = min(Lout_full, round(L / rate)); any 1 <= Lout <= Lout_full is
 * accepted.  What the three calls refuse, this one refuses with the same
 * status.  Output rows must not overlap input rows or each other.
 *
 * dsp_pitch_ratio (host only): the best p / q to 2^(semitones / 12) with p, q
 * <= 4096, by continued fractions (the nearest of the last convergent and the
 * last semiconvergent; the nearer to the reciprocal for an upward shift);
 * |semitones| <= 24, else DSP_ERR_INVALID.  A pitch shift by p / q is
 * dsp_time_stretch(rate = q / p) followed by dsp_resample(sr_in = p, sr_out =
 * q).  For the length to come back the stretch must deliver stretched =
 * floor(L p / q + 1 / 2) samples, and dsp_time_stretch of the L samples alone
 * ends short of that for an upward shift: its Lout_full is N + (F' - 1) H, about
 * (N - H)(1 / rate - 1) samples less, because the last input frame starts N - H
 * before the end.  So the input is first zero-padded: dsp_pitch_shift_plan
 * (host only) gives p, q, the stretch's spec (rate = q / p, N, H, window, floor
 * 1e-10), `padded` = the least max(L, 8192) + j H whose Lout_full reaches
 * `stretched`, `stretched` itself, and Lout = dsp_resample_plan(p, q,
 * stretched)'s length, within a sample of L (`stretched` is at least 1, so a
 * row shorter than q / (2 p) comes back up to q / p samples long).  The shift is
 * then: pad the rows
 * with zeros to `padded` samples, dsp_time_stretch(., padded, ., stretched,
 * stretch), dsp_resample(., stretched, ., Lout, p, q).  What
 * dsp_time_stretch_plan or dsp_resample_plan refuses, the plan refuses with the
 * same status; L = 0 is DSP_ERR_INVALID.  Any out pointer may be NULL. */
typedef struct dsp_pvoc_spec {
    double rate; /* 1/8 .. 8 */
} dsp_pvoc_spec;
typedef struct dsp_stretch_spec {
    double rate;    /* 1/8 .. 8 */
    uint32_t N;     /* 8192 */
    uint32_t H;     /* 512 .. N; 2048 is the usual choice */
    int32_t window; /* DSP_WIN_HAMMING or DSP_WIN_HANN */
    double floor;   /* 1e-12 .. 1; 1e-10 is the usual choice */
} dsp_stretch_spec;

/* The plans (host only, no device).  Any out pointer may be NULL.
 * dsp_pvoc_plan: F', chunk, and the bytes of device scratch: min(C, 16)
 * ceil(F' / chunk) rows of 4097 uint32. */
int dsp_pvoc_plan(uint64_t F, uint32_t C, const dsp_pvoc_spec *spec, uint64_t *frames_out, uint32_t *chunk,
                  uint64_t *scratch_bytes);
int dsp_pvoc(const float *const *spec_in, uint32_t C, uint64_t F, uint64_t ld_in, float *const *spec_out,
             uint64_t ld_out, const dsp_pvoc_spec *spec, const dsp_exec *ex);
int dsp_time_stretch_plan(uint64_t L, uint32_t C, const dsp_stretch_spec *spec, uint64_t *frames_in,
                          uint64_t *frames_out, uint64_t *Lout_full, uint64_t *Lout_default,
                          uint64_t *device_bytes);
int dsp_time_stretch(const float *const *in, uint32_t C, uint64_t L, float *const *out, uint64_t Lout,
                     const dsp_stretch_spec *spec, const dsp_exec *ex);
int dsp_pitch_ratio(double semitones, uint32_t *p, uint32_t *q);
int dsp_pitch_shift_plan(uint64_t L, uint32_t C, double semitones, uint32_t H, int32_t window, uint32_t *p, uint32_t *q,
                         dsp_stretch_spec *stretch, uint64_t *padded, uint64_t *stretched, uint64_t *Lout);

/* Room-acoustic decay analysis (ISO 3382) of C impulse responses of L samples:
 * what an impulse response (dsp_deconvolve) is measured for.  dsp_decay returns
 * per (channel, band) the energy of the band-filtered response in short hops
 * from the channel's onset, as raw float64 sums; dsp_decay_derive (host only)
 * turns one such row into reverberation times, clarity, definition and centre
 * time.
 *
 * Bands.  G = 10^0.3, fraction b = 1 (octave) or 3 (third-octave), band index k
 * has the mid frequency fm = 1000 G^(k / b) Hz.  The spec names k_lo..k_hi, at
 * most 32 bands (octave -5..4: 31.6 Hz..16 kHz; third-octave -16..13: 25 Hz..
 * 20 kHz).  A band whose upper edge fm G^(1 / (2 b)) exceeds sr / 2 is
 * DSP_ERR_INVALID.
 * Filter.  Zero phase, applied in the frequency domain: bin frequency f is
 * multiplied by g(f) = 1 / sqrt(1 + (Qd (f / fm - fm / f))^6), g(0) = 0, with
 * Qr = 1 / (G^(1 / (2 b)) - G^(-1 / (2 b))) and Qd = (pi / 6) / sin(pi / 6) Qr:
 * the magnitude of the sixth-order Butterworth band filter of IEC 61260 /
 * ANSI S1.11.  Zero phase means the filter rings symmetrically: a little band
 * energy lies before the onset (entry 0 below), and ISO 3382's caveat that a
 * band of width B resolves a decay time T only for B T > 16 applies.  g is
 * computed per bin in float32 with correctly rounded division and square root.
 * Transform.  y_{c,b} = irfft_n(g_b rfft_n(in[c]))[0..L) with n the smallest
 * power of two >= max(1024, L + P), P = ceil(8 sr Qr / fm_lo) for the lowest
 * band (8 / its bandwidth): the response's slowest pole decays as
 * e^(-pi B t / 2), so what wraps around into [0, L) is below -100 dB.
 * n > 2^24 is DSP_ERR_UNSUPPORTED.
 * Onset, per channel, on the unfiltered row: peak = max |in[c]|, thr = peak *
 * 0.1f (one float32 product), onset = the first i with |in[c][i]| >= thr (ISO
 * 3382's -20 dB rule).  Both are exact.  A silent row: peak 0, onset 0, every
 * energy 0.
 * Hop.  sr % 100 != 0 is DSP_ERR_UNSUPPORTED; hop = the largest divisor of
 * sr / 100 that is <= sr / 1000 (48000: 48, 44100: 21, 96000: 96, 88200: 63,
 * 32000: 32), so 10, 50 and 80 ms are whole hops.  Hop j of channel c covers
 * [onset_c + j hop, min(L, onset_c + (j + 1) hop)).
 * Output.  peak[c] and onset[c]; energy[c bands + b], rows of hops =
 * ceil(L / hop) + 1 float64: entry 0 = sum y^2 over i < onset, entry 1 + j =
 * sum y^2 over hop j, the rest 0.  moment (may be NULL), the same layout:
 * sum (i - onset) y^2, in samples.
 * Summation order (part of the contract): y^2 is one float32 product, taken to
 * float64.  A hop's samples i = 0 .. are dealt to 16 float64 accumulators, i to
 * accumulator i mod 16, each added in sample order; the 16 are then added as a
 * tree, a_q += a_{q ^ 8}, then ^ 4, ^ 2, ^ 1.  Entry 0: the samples before the
 * onset are cut into pieces of hop samples from sample 0, each summed as a hop;
 * the pieces p are dealt to 64 accumulators, p to accumulator p mod 64, added in
 * piece order, and the 64 are added as the same tree from ^ 32 down.  So a row
 * is a function of hop and the band-filtered samples alone: no float atomics,
 * the same bits on every run, and (channel, band)'s bits do not depend on C,
 * the number of bands or the group size.  Accuracy: per row max_j |e - exact|
 * <= 3.5e-6 max_j exact for finite samples; non-finite samples give undefined
 * sums and onset.
 * Method: an integer atomic max over |x| bit patterns and an integer atomic min
 * over indices (no float atomics) for peak and onset; dsp_rfft's passes for the
 * channels; per group of (channel, band) rows a mask launch, dsp_irfft's passes
 * and the hop reduction, which reads the onset on the device: the call does not
 * synchronise its stream.  The scratch is kept per stream; the rows of a group
 * are capped at 256 MiB of it (16 rows at most, one at least: 320 MiB at
 * n = 2^24), see dsp_decay_plan.
 * DSP_ERR_INVALID for C = 0, L = 0, ex->sample_offset != 0, a bad spec, a
 * float64 row that is not 8-byte aligned, or any overlap of an output row with
 * an input row or another output row (nothing is written).  Host rows with
 * DSP_EXEC_HOST_BUFFERS.  The twiddle table is cached per device: a stream being
 * captured needs one eager call of the same n first.  DSP_ERR_NO_DEVICE without
 * a device. */
typedef struct dsp_decay_spec {
    uint32_t fraction; /* 1 or 3 */
    int32_t k_lo, k_hi;
} dsp_decay_spec;      /* NULL: {1, -5, 4} */

/* The plan (host only, no device).  Any out pointer may be NULL; fm holds 32. */
int dsp_decay_plan(uint64_t L, uint32_t C, uint32_t sr, const dsp_decay_spec *spec, uint32_t *n, uint32_t *P,
                   uint32_t *hop, uint32_t *bands, uint64_t *hops, uint64_t *scratch_bytes, double *fm);
int dsp_decay(const float *const *in, uint32_t C, uint64_t L, uint32_t sr, const dsp_decay_spec *spec, float *peak,
              uint64_t *onset, double *const *energy, double *const *moment /* may be NULL */, const dsp_exec *ex);

/* From one energy row to the room-acoustic figures (host only, float64).
 * e_j = energy[1 + j] for the F = (L - onset) / hop full hops (a partial last
 * hop is ignored); W = (sr / 100) / hop hops are 10 ms.
 *   noise N      the mean of the last max(1, F / 10) of the e_j
 *   inr          10 log10(max_k mean(e[k .. k + W)) / N) dB; +inf when N = 0
 *   truncation   k_t: the first k at or after the loudest window with
 *                mean(e[k .. k + W)) <= 10^0.3 N, else the start of the noise tail
 *   EDC_k = sum_{j = k}^{k_t - 1} e_j, L_k = 10 log10(EDC_k / EDC_0) at t_k = k hop / sr
 *   edt, t20, t30   -60 / slope of the least-squares line of L_k against t_k from
 *                the first k with L_k <= hi to the last with L_k >= lo, (hi, lo) =
 *                (0, -10), (-5, -25), (-5, -35), in seconds.  Valid with inr >=
 *                20 / 35 / 45 dB and at least 3 points; else NaN and the flag bit
 *   c50, c80     10 log10(early / late) dB, split at 0.05 sr / hop and 0.08 sr /
 *                hop hops, late summed up to k_t;  d50 = early / (early + late)
 *   ts           sum moment / sum e over j < k_t, in seconds; NaN without a
 *                moment row
 * No noise compensation is done (Lundeby's method is out of scope).  A silent
 * row (every e_j = 0) sets DSP_DECAY_SILENT, one with F < W DSP_DECAY_SHORT;
 * both leave every value NaN.  DSP_ERR_INVALID for a NULL energy or res,
 * onset > L, or a rate and hop other than dsp_decay_plan's. */
#define DSP_DECAY_SILENT 0x1u
#define DSP_DECAY_EDT_INVALID 0x2u
#define DSP_DECAY_T20_INVALID 0x4u
#define DSP_DECAY_T30_INVALID 0x8u
#define DSP_DECAY_SHORT 0x10u
typedef struct dsp_decay_result {
    double edt, t20, t30;       /* seconds */
    double c50, c80;            /* dB */
    double d50;                 /* 0..1 */
    double ts;                  /* seconds */
    double inr;                 /* dB */
    uint32_t flags;             /* DSP_DECAY_* */
    uint32_t truncation;        /* k_t, in hops from the onset */
    uint32_t reserved[2];
} dsp_decay_result;
int dsp_decay_derive(const double *energy, const double *moment /* may be NULL */, uint64_t L, uint64_t onset,
                     uint32_t hop, uint32_t sr, dsp_decay_result *res);

/* Test hooks (not for production use).
 * DSP_DEBUG_BIQUAD_SPIN_LIMIT (set): the sleeps a DSP_PLUGIN_BIQUAD look-back
 *   waits for a preceding tile's words before it gives up (value ~0 restores
 *   the default); a launch in which a wave gave up is rendered again, on the
 *   same stream before the call's later work, as one serial chain per channel
 *   (within the same bound).  0 gives up wherever a word is not there at the
 *   first look.
 * DSP_DEBUG_BIQUAD_REPAIRS (get): launches on the current device rendered
 *   again that way since the last get (read it after the renders finished).
 * DSP_DEBUG_FRAME_RUN (set / get): frames per wave of the frame reuse (see
 *   DSP_EXEC_EVERY_FRAME) wherever it is valid, whatever the call's length
 *   (1..65535; 1 = every frame; 0 restores the launch's own choice).
 *   Process-wide: for tests and A/B runs.  A set value keeps the call on the
 *   reuse launch: it then takes no cached spectrum row.
 * DSP_DEBUG_SPECTRUM_CACHE (set / get): the cached spectrum row of the fused
 *   IR_test launch (DSP_RESULT_SPECTRUM_CACHE).  0: the library's own choice
 *   (calls long enough for frame reuse); 1: wherever the row is valid, whatever
 *   the call's length; 2: never (every call takes the reuse launch).
 * DSP_DEBUG_ROW_RUN (set / get): frames per wave of the store-only launch that
 *   serves a cached row (1..65535; 0 restores the default).
 * DSP_DEBUG_ROW_PACE (set / get): the pacing of that launch, nap | waves << 8:
 *   a wave sleeps `nap` units (0..16) between its hop stores and its row
 *   stores, and a compute unit holds `waves` (3..9) of them at once; with
 *   1 << 16 the row's lifetime event is recorded after the launch and not as
 *   the launch's own completion.  0 restores the default; the bytes written
 *   are the same for every value.  All three process-wide: for tests and A/B
 *   runs.
 * DSP_DEBUG_PVOC_CHUNK (set / get): output frames per chunk of dsp_pvoc and of
 *   dsp_pvoc_plan (8..4096; 0 restores 64).  The output's bits do not depend on it.
 * DSP_DEBUG_PVOC_VARIANT (set / get): the A/B variants of dsp_pvoc's kernels, a
 *   sum of 1 (an increment is one argument of the product Z[f + 1] conj Z[f]
 *   instead of the difference of two argument words), 2 (cos and sin by the
 *   hardware's turn-based instructions) and 4 (the first launch stores every
 *   increment in min(C, 16) F' 4097 more uint32 of scratch and the third reads
 *   them back).  0 restores the product; 1 and 2 change the output within the
 *   documented accuracy, 4 does not change it.  Both process-wide: for
 *   tools/ab_pvoc.py. */
enum {
    DSP_DEBUG_BIQUAD_SPIN_LIMIT = 1,
    DSP_DEBUG_BIQUAD_REPAIRS = 2,
    DSP_DEBUG_FRAME_RUN = 3,
    DSP_DEBUG_SPECTRUM_CACHE = 4,
    DSP_DEBUG_ROW_RUN = 5,
    DSP_DEBUG_ROW_PACE = 6,
    DSP_DEBUG_PVOC_CHUNK = 7,
    DSP_DEBUG_PVOC_VARIANT = 8
};
int dsp_debug_set(int what, uint64_t value);
int dsp_debug_get(int what, uint64_t *value);

/* Offline render, one-shot:
 *   nblocks = ceil(L / B); out[c] holds nblocks * B floats.
 *   Block b: out = file[cursor .. cursor+B) for c < in_channels, zero past
 *   EOF and for c >= in_channels, then audio_callback(out, C, B, sr).
 * in[c] (c < in_channels) hold L floats.  in_channels may be 0 (silence). */
int dsp_render_offline(const float *const *in, uint32_t in_channels, uint64_t L,
                       float *const *out, uint32_t C, uint32_t B, float sr,
                       const dsp_plugin *plugin, const dsp_exec *ex);

/* Offline render, loop mode (render_audio with audio_file_loop set,
 * audio.cpp:100-132): the file wraps -- block b, sample s reads file sample
 * (cursor + b B + s) mod L for c < min(in_channels, C); other channels are
 * zero (audio.cpp:138-141); then audio_callback in place.  Renders nblocks
 * blocks into out[c] (nblocks B floats) and returns the next read cursor,
 * (cursor + nblocks B) mod L, in *cursor_out (may be NULL).  L == 0 with a
 * file is DSP_ERR_INVALID (the reference spins forever, audio.cpp:104).
 * Device buffers only. */
int dsp_render_loop(const float *const *in, uint32_t in_channels, uint64_t L, uint64_t cursor,
                    float *const *out, uint32_t C, uint32_t B, uint64_t nblocks, float sr,
                    const dsp_plugin *plugin, uint64_t *cursor_out, const dsp_exec *ex);

/* STFT magnitude over C planar channels of L samples:
 *   F = dsp_stft_frame_count(L, N, H); mag[c][f * ld + k] = |X_f[k]| / sqrt(N)
 *   for k < K, X_f = DFT_N(w * in[c][f*H .. f*H + N)).
 * K <= N/2 + 1 for real input (K = N/2 + 1 = 4097 at N = 8192), or K = N
 * for the reference's all-bins layout (dsp.cpp:65; mirror |X[N-k]| = |X[k]|).
 * N = 8192 runs the CDNA4 wave-per-frame kernel; other powers of two <= 8192
 * run the generic LDS kernel.
 * Accuracy, here and in dsp_render_stft: per frame max_k |mag - exact| <=
 * 1e-6 max_k(exact) + 2^-61.  The absolute term is the quiet-frame floor: the
 * 8192-point kernels take the root of re^2 + im^2 (of a quarter of it at the
 * self-paired bin N / 4) with the hardware instruction, which reads a denormal
 * argument as zero, so a magnitude below 2^-62 may be stored as 0 (2^-61
 * leaves a factor of two).  It matters only to frames whose peak is below
 * about 2^-41; samples must be finite for the magnitudes to be defined. */
int dsp_stft_magnitude(const float *const *in, uint32_t C, uint64_t L, uint32_t N,
                       uint32_t H, int32_t window, uint32_t K, float *const *mag,
                       uint64_t ld, const dsp_exec *ex);

/* Render + STFT of the render, fused when the plugin is a per-sample map
 * (NOOP / GAIN / STATIC_GAIN / IR_RAMP) and N = 8192, H % B == 0.
 * Output = dsp_render_offline's out + dsp_stft_magnitude(out, ..., nblocks*B). */
int dsp_render_stft(const float *const *in, uint32_t in_channels, uint64_t L,
                    float *const *out, uint32_t C, uint32_t B, float sr,
                    const dsp_plugin *plugin, uint32_t N, uint32_t H,
                    int32_t window, uint32_t K, float *const *mag, uint64_t ld,
                    const dsp_exec *ex);

/* End to end from host memory: dsp_render_stft (mag != NULL) or
 * dsp_render_offline (mag == NULL) of host rows in[c] (L samples) into host
 * rows out[c] (ceil(L / B) B floats) and mag[c] (F rows of stride ld),
 * streamed through HBM in time chunks of about `chunk` samples (0: one
 * chunk): the upload of chunk t + 1 and the download of chunk t - 1 overlap
 * chunk t's compute (three HIP streams, two device slots).  Pinned host
 * buffers (hipHostMalloc / hipHostRegister) are DMA'd directly, pageable ones
 * staged through pinned slots.  Results equal the device-buffer call bit for
 * bit (lcm(B, H)-aligned chunks with an N - H halo); FIR and GENERIC plugins
 * run as one chunk.  Returns when the host rows are written.  ex->stream is
 * the compute stream. */
int dsp_render_stft_host(const float *const *in, uint32_t in_channels, uint64_t L, float *const *out, uint32_t C,
                         uint32_t B, float sr, const dsp_plugin *plugin, uint32_t N, uint32_t H, int32_t window,
                         uint32_t K, float *const *mag, uint64_t ld, uint64_t chunk, const dsp_exec *ex);

/* IR analysis: ir_out[c][0..ir_len) = audio_callback(delta) for every
 * channel (plugin.cpp:27-54), then mag[0 .. 4*ir_len) = |FFT_{4 ir_len}(
 * hamming(ir_len) * ir_out[0], zero padded)| / sqrt(4 ir_len) (dsp.cpp:53-66).
 * ir_len = 2048 in the reference (hardcoded_values.h:27). */
int dsp_ir_analysis(const dsp_plugin *plugin, uint32_t C, float sr, uint32_t ir_len,
                    float *const *ir_out, float *mag, const dsp_exec *ex);

/* Complex FFT services (dsp.cpp:74-132): n a power of two <= 8192.
 * forward: re + i*im = DFT(in + 0i) / sqrt(n)
 * reverse: out = Re(IDFT(re + i*im)) / sqrt(n) */
int dsp_fft_forward(const float *in, float *re, float *im, uint32_t n,
                    const dsp_exec *ex);
int dsp_fft_reverse(const float *re, const float *im, float *out, uint32_t n,
                    const dsp_exec *ex);

/* Elementwise services on device buffers (dsp.cpp:171-181, 208-210, 248-250). */
int dsp_gain(const float *in, float *out, float gain, uint64_t n, const dsp_exec *ex);
int dsp_copy(const float *in, float *out, uint64_t n, const dsp_exec *ex);
int dsp_set(float value, float *out, uint64_t n, const dsp_exec *ex);
int dsp_magnitude(const float *re, const float *im, float *out, uint64_t n,
                  const dsp_exec *ex);

/* Display reductions for long-file overviews.
 * minmax: the IR / waveform view's per-pixel extremes (opengl.h:877-890):
 *   vmax[p] = max(-1, max x[s]), vmin[p] = min(+1, min x[s]) over the
 *   samples s with s * pixels / n == p (the reference's initial values; the
 *   index product is 64-bit here, the reference's u32 product wraps).
 * spectrogram: out[p * K + k] = max of mag[f * ld + k] over the frames f
 *   with f * pixels / F == p (0 for an empty column). */
int dsp_minmax_decimate(const float *x, uint64_t n, uint32_t pixels, float *vmax, float *vmin,
                        const dsp_exec *ex);
int dsp_spectrogram_decimate(const float *mag, uint64_t F, uint32_t K, uint64_t ld,
                             uint32_t pixels, float *out, const dsp_exec *ex);

/* Kernel timing: when enabled, every launch of the dominant kernel of
 * dsp_render_stft / dsp_stft_magnitude (the 8192-point wave-per-frame kernel)
 * is bracketed by HIP events on its stream.  dsp_kernel_timing() waits for
 * them, returns the summed duration, the launch count and the algorithmic
 * bytes of those launches, and clears the record.  Enabling
 * creates a stock of events for the current device, and read-out events are
 * reused, so the timed launches do not pay for event creation. */
void dsp_kernel_timing_enable(int on);
int dsp_kernel_timing(double *total_ms, uint64_t *launches, uint64_t *bytes);

/* The 8192-point kernel and its options are fixed at build time.  The A/B
 * and ablation instantiations live in a separate tools build (`make ab`:
 * build/ab/libdspbench_ab.so, which adds dsp_stft_pk_ab_options()); this
 * library has no process-wide kernel selection. */


/* Diagnostics. */
int dsp_abi_version(void);
const char *dsp_status_string(int status);
const char *dsp_last_error(void);
int dsp_device_count(void);

#ifdef __cplusplus
}
#endif

#endif /* DSPBENCH_H */
