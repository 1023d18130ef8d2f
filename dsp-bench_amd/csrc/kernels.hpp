// kernels.hpp -- kernel argument blocks and launchers shared by the HIP
// translation units and the C ABI (capi.cpp, capi_render.cpp, capi_signal.cpp).
#pragma once
#include "common.hpp"
#include "host_tables.hpp"  // kConvHop, kConvSpec4

struct dsp_module;  // include/dspbench/module.h

namespace dspb {

typedef float v2f __attribute__((ext_vector_type(2)));

struct RenderArgs {
    ChanIn in;
    uint32_t in_ch;
    uint64_t L;      // file samples available from in[c][0]
    ChanOut out;
    uint64_t start;  // first local sample to render
    uint64_t end;    // one past the last (nblocks * B)
    SampleMap map;
    uint64_t goff;   // global index of local sample 0
};

struct Stft8kArgs {
    ChanIn in;           // signal (memory source) or WAV file (fused)
    uint32_t in_ch;      // channels present in `in`
    uint64_t L;          // valid samples in in[c] (file length when fused)
    ChanOut out;         // fused: render output
    ChanOut mag;         // magnitudes, row f at mag[c] + f * ld
    uint64_t F;          // frames per channel
    uint32_t H;          // hop
    uint32_t K;          // bins stored (<= 4097, or 8192 = mirrored all-bins)
    uint64_t ld;         // row stride of mag
    uint32_t valid;      // samples of a frame that exist (8192, or IR length)
    const v2f *win2;     // window as 4096 float2 (w[2m], w[2m+1]), zero past valid
    const v2f *tw;       // T8192[k] = exp(-2 pi i k / 8192), k < 8192
    float scale;         // 1 / sqrt(8192)
    SampleMap map;       // fused render map
    uint64_t goff;       // global sample index of in[c][0] / out[c][0]
    uint64_t *stamps;    // diagnostic builds only (-DDSPB_STAMPS): per-frame phase clocks
    const float4 *wbase; // computed-window variants: (cos, sin) of theta (2 lane), theta (2 lane + 1)
    float wa, wb;        // window w = wa - wb cos(theta n), pre-scaled
    uint64_t tail_end;   // > F H: waves F .. render [F H, tail_end) too (stft_pk PER path), else 0
    // stft_pk PER path, frame reuse (H % B == 0: every frame of the call has the
    // same samples): a wave owns `run` consecutive frames of a channel, computes
    // the spectrum once and stores it `run` times.  0 / 1: one frame per wave.
    // The caller sets run (stft8192_pk_frame_run); the launch sets run_waves.
    uint32_t run;
    uint64_t run_waves;  // ceil(F / run): the waves past them render the tail
};

struct GenericFftArgs {
    // input: either split complex (re, im[may be null]) or real frames
    const float *re_in;
    const float *im_in;
    ChanIn sig;          // real frames: signal channels (STFT / IR)
    uint64_t frame_hop;  // samples between frames
    uint32_t valid;      // samples per frame that exist (zero beyond)
    const float *win;    // window (n floats, may be null)
    uint32_t n, log2n;
    int dir;             // -1 forward, +1 inverse
    const v2f *tw;       // T8192
    float scale;
    // output: split complex, real part only, or magnitude rows
    float *re_out;
    float *im_out;
    ChanOut mag;
    uint32_t K;
    uint64_t ld;
    int mode;  // 0: complex->complex, 1: complex->real part, 2: frames->mag
};

int launch_ramp_table(float *table, uint32_t B, float gain, float step, hipStream_t s);
int launch_render(const RenderArgs &A, uint32_t C, bool vec, hipStream_t s);
int launch_render_wrap(const RenderArgs &A, uint32_t C, uint64_t cursor, hipStream_t s);
int module_render(::dsp_module *m, const void *params, uint32_t params_size, const float *const *in,
                  uint32_t in_ch, uint64_t L, float *const *out, uint32_t C, uint32_t B, float sr,
                  uint64_t goff, hipStream_t s, uint32_t flags);
int module_callback_once(::dsp_module *m, const void *params, uint32_t params_size, float *const *bufs, uint32_t C,
                         uint32_t B, float sr, hipStream_t s);
int module_ir(::dsp_module *m, const void *params, uint32_t params_size, float *const *bufs, uint32_t C,
              uint32_t n, float sr, hipStream_t s);
// a stateless plugin's block class for (Parameters, C, B, sr), probed once
// through its own callback and cached in the module (module.cpp)
enum { kSpecNone = 0, kSpecTable = 1, kSpecGain = 2, kSpecGainTable = 3 };
struct ModuleSpec {
    int kind = kSpecNone;
    float gain = 1.f;             // kSpecGain: y = gain x
    const float *table = nullptr; // kSpecTable: the block every block renders (B floats, every channel);
                                  // kSpecGainTable: C rows of B gains, y = x * G[c][position]
    // kSpecTable: the block is an f64 ramp rounded to f32, table[i] =
    // (float)fma(-i, rs, rg0) for every i < B, checked bit for bit on the host
    // (the fused kernels then evaluate it instead of loading the table)
    bool affine = false;
    double rg0 = 0.0, rs = 0.0;
    void *use = nullptr;  // kSpecTable: the hold on the table, released by module_spec_done
};
int module_specialize(::dsp_module *m, const void *params, uint32_t params_size, uint32_t C, uint32_t B, float sr,
                      hipStream_t s, ModuleSpec *out);
// after the launches that read a table class's block (ModuleSpec::use)
int module_spec_done(::dsp_module *m, void *use, hipStream_t s);
void spec_reap(::dsp_module *m);
size_t module_spec_retired(::dsp_module *m);  // tables evicted and not yet freed
struct FirFftArgs {
    ChanIn in;           // input channels
    uint32_t in_ch;
    uint64_t L;          // input samples (zero past)
    ChanOut out;         // render rows, Ly samples
    uint64_t Ly;
    uint64_t F;          // frames = ceil(Ly / 7168)
    const float *H;      // FFT(taps)/16384, lane-major pairs (fir_fft.hip)
    v2f h2048;           // H[2048]
    const v2f *tw;       // T8192 + lane-major stage twiddles (capi.cpp get_tw)
    uint32_t nout;       // fir_pair_kernel: output channels in `out` (set by launch_fir_pair)
};
int launch_fir_fft(const FirFftArgs &A, uint32_t C, hipStream_t s);
// two channels per frame as one complex signal, 4096-point frames, hop 3072
// (C even; F = ceil(Ly / kPairHop); H = SampleMap::pairH; h2048 unused)
constexpr uint32_t kPairHop = 3072;
int launch_fir_pair(const FirFftArgs &A, uint32_t C, hipStream_t s);
int launch_fir(const float *x, uint64_t L, float *y, uint64_t Ly, const float *h8, uint32_t T8,
               bool y_aligned16, hipStream_t s);
// DSP_PLUGIN_CONV (conv_fdl.hip): partitioned overlap-save, 8192-point real
// frames of hop kConvHop, one launch_conv per channel group: forward
// transforms into X, the multiply-accumulate over partitions into Y, inverse
// transforms into the render rows
struct ConvArgs {
    ChanIn in;           // input channels
    uint32_t in_ch;
    uint64_t L;          // input samples (zero past)
    ChanOut out;         // render rows, Ly samples
    uint64_t Ly;
    uint64_t F;          // frames = ceil(Ly / kConvHop)
    const float4 *H;     // `parts` spectra of kConvSpec4 float4 (host_tables.cpp conv_table)
    uint32_t parts;      // partitions = ceil(T / kConvHop)
    float4 *X, *Y;       // scratch: [channel][frame] spectra of the input and of the output
    const v2f *tw;       // T8192 + lane-major stage twiddles (capi.cpp get_tw)
};
int launch_conv(const ConvArgs &A, uint32_t C, hipStream_t s);
// dsp_resample (resample.hip): one launch converts C <= 16 channels.  up,
// down, half, Tp are the plan's (host_tables.hpp ResamplePlan);
// resample_blocking derives the rest from them, and `table` holds
// resample_device_table's layout for that blocking
struct ResampleArgs {
    ChanIn in;
    ChanOut out;
    uint64_t L, Lout;
    const float *table;
    uint32_t up, down, half, Tp;
    uint32_t phase;          // 1: resample_phase_kernel<R>; 0: resample_direct_kernel
    uint32_t R, S;           // phases per group; steps of a group's sweep (a multiple of 4)
    uint32_t JC;             // 64-period chunks per tile
    uint32_t a, hreg;        // down = odd << a; floats per LDS region of the staged input
    uint32_t xspan, xfloats; // staged inputs per tile; floats of LDS they take
    uint32_t lds_bytes;
    uint32_t out_aligned16;  // every output row is 16-byte aligned
};
void resample_blocking(ResampleArgs *A);
uint64_t resample_device_floats(const ResampleArgs &A);
void resample_device_table(const ResampleArgs &A, const float *plain, float *out);
int launch_resample(const ResampleArgs &A, uint32_t C, hipStream_t s);
// DSP_PLUGIN_BIQUAD (iir.hip): one launch renders C <= 16 channels of Ly
// samples from zero state; tiles of 64 lanes x biquad_lane_samples() samples
struct BiquadArgs {
    ChanIn in;
    uint32_t in_ch;
    uint64_t L;            // file samples (zero past)
    ChanOut out;
    uint64_t Ly;           // rendered samples per channel
    uint32_t C;            // channels of this launch
    uint64_t ntiles_ch;    // biquad_tiles(Ly)
    const float *coef;     // 5 S floats (b0 b1 b2 a1 a2 per section)
    const float *Q;        // 65 D x D: M^(T l)
    const float *P;        // 257 D x D: M^(64 T k)
    uint32_t window;       // W: S_in from the W previous tiles' aggregates (0: inclusive look-back)
    uint64_t *aggw, *inclw;  // per tile, nch D words: epoch << 32 | float bits (aggregate, inclusive)
    uint64_t epoch;        // distinct per launch on one workspace (32 bits used)
    uint32_t spin_limit;   // sleeps a look-back waits before it gives up
    uint32_t *err;         // the stream's workspace word: a wave that gave up writes the epoch
    uint32_t *repairs;     // host-mapped: launches biquad_repair_kernel rendered again (diagnostic)
    uint32_t in_aligned16, out_aligned16;
};
uint64_t biquad_tiles(uint64_t Ly);
uint32_t biquad_lane_samples();
// nch = 2: one wavefront per tile of a channel pair (C even), packed math
int launch_biquad(const BiquadArgs &A, uint32_t sections, uint32_t nch, hipStream_t s);
// dsp_loudness (loudness.hip): one channel group (<= 16 rows) per call of each
// launcher.  Scratch rows are the group's (loudness_host.hpp
// loudness_scratch_bytes): z[16][hops], peaks[32], part[16][tiles][4].
struct LoudnessArgs {
    ChanIn in;
    uint64_t L;            // samples per row
    uint32_t first, count; // rows [first, first + count) of the group in this launch
    uint64_t tiles;        // ceil(L / 2048)
    uint32_t hop;
    uint64_t hops;
    const float *coef;     // loudness_tables: 10 of 20 floats,
    const float *Q;        // 65 4 x 4: M^(T l) in the scan's coordinates,
    const float *P;        // 2 4 x 4: I, M^(64 T)
    uint32_t window;       // warm-up tiles before a wave's run (the cascade's look-back)
    uint32_t run;          // tiles a wave measures
    float *part;           // per (row, tile): 4 hop partials, the tile's first hop first
    double *z;             // per (row, hop): the hop energy
    uint32_t *peaks;       // [16] sample peaks, [16] true peaks: the bits of max |.|
    uint32_t in_aligned16;
};
// partial sums + sample peaks (nch = 2: one wavefront per channel pair, count even)
int launch_loudness_kweight(const LoudnessArgs &A, uint32_t nch, hipStream_t s);
// z[row][j] from the partials, rows [0, rows)
int launch_loudness_finish(const LoudnessArgs &A, uint32_t rows, hipStream_t s);
// max |y| of the rows at ovs x the rate; table = resample_device_table's layout
// for up = ovs, down = 1 ([step][phase], `steps` a multiple of 4)
int launch_loudness_truepeak(const LoudnessArgs &A, uint32_t rows, uint32_t ovs, const float *table,
                             uint32_t steps, uint32_t half, hipStream_t s);
// dsp_limiter (limiter.hip): one launch of each pass serves `ngroups` link
// groups of `nch` rows each (ngroups nch <= 16): group j is rows [j nch,
// (j + 1) nch) of in / out and row j of the scratch, of gain and of det.
struct LimiterArgs {
    ChanIn in;
    ChanOut out;
    ChanOut gain, det;     // per group; NULL: not asked for
    uint64_t L;
    uint64_t tiles;        // ceil(L / 2048); scratch rows hold tiles 2048 floats
    uint32_t ngroups, nch;
    uint32_t A;            // lookahead
    uint32_t wpad;         // window entries of the table, a multiple of 8
    float c;               // ceiling
    const float *tab;      // limiter_host.hpp limiter_table
    float *h;              // [ngroups][tiles 2048]
    float *pmax;           // [tiles 2048]: a linked group's p over its earlier launches (or NULL)
    uint32_t pmode;        // pass 1: 0 whole (p, hold, E); 1 p of these rows to pmax; 2 the same, max with pmax
    uint32_t use_pmax;     // pass 1, pmode 0: p is combined with pmax
    float *E, *carry;      // [ngroups][tiles]
    uint32_t *words;       // [0] min g as an ordered key, [2..3] the count (64 bits); NULL: not counted
    const float *tp;       // the oversampler's table [step][phase] (or NULL)
    uint32_t steps, half;
    uint32_t in_aligned16, out_aligned16, gain_aligned16;
};
int launch_limiter_detect(const LimiterArgs &A, uint32_t ovs, hipStream_t s);
int launch_limiter_carry(const LimiterArgs &A, hipStream_t s);
int launch_limiter_apply(const LimiterArgs &A, hipStream_t s);
// dsp_rfft / dsp_irfft / dsp_deconvolve (fft_big.hip): `nch` <= 16 channels per
// launch, channel j's work buffers at buf0 / buf1 + j M (M = n / 2 complex).
struct BigFftArgs {
    uint32_t n, nch;
    uint32_t passes, radix[4];   // host_tables.hpp rfft_plan
    const v2f *tw;               // rfft_twiddles(n): lo, then hi
    v2f *buf0, *buf1;            // [nch][M] each
    ChanIn in;                   // forward: real rows of L samples; inverse: spectra of M + 1 bins
    ChanOut out;                 // forward: spectra of M + 1 bins; inverse: real rows of Lout samples
    uint64_t L, Lout;
    uint32_t rot;                // inverse: sample i of the transform is written at (i + rot) mod n
    uint32_t in_aligned8, out_aligned8;
};
// the forward transform of nch rows: pack + passes + real split
int launch_big_rfft(const BigFftArgs &A, hipStream_t s);
// the inverse: inverse split + passes + unpack, scaled by 1 / n
int launch_big_irfft(const BigFftArgs &A, hipStream_t s);
// *word = max(*word, the bits of max_k |S[k]|^2) over `bins` bins (an integer atomic max; zero the word first)
int launch_deconv_max(const v2f *S, uint32_t bins, uint32_t *word, hipStream_t s);
// Y_j[k] = Y_j[k] conj(S[k]) / (|S[k]|^2 + eps *word) for j < nch spectra of `bins` bins at Y + j bins
int launch_deconv_divide(v2f *Y, const v2f *S, uint32_t bins, uint32_t nch, float eps, const uint32_t *word,
                         hipStream_t s);
// dsp_welch (welch.hip): one chunk of frames of one channel group per call:
// forward transforms into S, the run sums into the partials, the runs added in
// float64 onto the output rows (welch_host.hpp has the constants and the layout)
struct WelchArgs {
    ChanIn in;             // cn channel rows
    const float *ref;      // the reference row (row cn of the launches), or NULL
    uint32_t cn, has_ref;
    uint64_t f0;           // the chunk's first frame
    uint32_t nf;           // its frames, <= chunk
    uint32_t H;
    uint32_t chunk;        // frames per row of S
    uint32_t runs_cap;     // runs per row of the partials: chunk / kWelchRun
    const v2f *win2;       // the window as 4096 float2 (w[2m], w[2m+1])
    const v2f *tw;         // T8192 + lane-major stage twiddles (capi.cpp get_tw)
    float4 *S;             // [cn + has_ref][chunk] spectra of kWelchSpec4 float4
    v2f *pxx;              // [cn][runs_cap][kWelchSpec4]
    float4 *pxy;           // [cn][runs_cap][kWelchSpec4] (re, re, im, im)
    v2f *prr;              // [runs_cap][kWelchSpec4]
    double *sxx[kMaxChannels];  // output rows: 4097 doubles,
    double *sxy[kMaxChannels];  // 4097 (re, im) pairs (has_ref),
    double *srr;           // 4097 doubles (has_ref; NULL: a later channel group, not written again)
    uint32_t first;        // the call's first chunk: the sums start from zero
};
int launch_welch_chunk(const WelchArgs &A, hipStream_t s);
// dsp_stft (stft_cx.hip): the frames [f0, f0 + nf) of one channel group, one
// wavefront per (frame, row), every bin stored once in natural order
struct StftCxArgs {
    ChanIn in;             // cn channel rows
    ChanOut spec;          // cn spectrum rows, 8-byte aligned: frame f at spec[c] + f ld
    uint32_t cn;
    uint64_t f0, nf;
    uint32_t H;
    uint64_t ld;           // floats, even, >= 8194
    const v2f *win2;       // the window as 4096 float2 (w[2m], w[2m+1])
    const v2f *tw;         // T8192 + lane-major stage twiddles (capi.cpp get_tw)
};
int launch_stft_cx(const StftCxArgs &A, hipStream_t s);
// dsp_istft (stft_cx.hip): one chunk of one channel group (stft_cx_host.hpp
// istft_chunk): the frames [fa, fa + ns) inverted and windowed into the slots
// [0, ns) of the scratch, then the samples [i0, i1) summed, divided and stored
struct IstftArgs {
    ChanIn spec;           // cn spectrum rows, 8-byte aligned
    ChanOut out;           // cn output rows
    uint32_t cn;
    uint64_t ld;
    uint32_t H;
    uint64_t F;            // frames of the call
    uint64_t fa;           // the frame in slot 0
    uint32_t ns;           // slots filled, <= slots
    uint32_t slots;        // slots per row of S
    uint64_t i0, i1;       // the samples this chunk owns
    uint32_t t0, n;        // set by the launch: i0 - fa H, and i1 - i0
    float floor;
    const v2f *win2;       // the window as 4096 float2, and
    const float *win;      // the same table as 8192 floats
    const v2f *tw;
    float *S;              // [cn][slots][8192] w v_f
};
int launch_istft_chunk(const IstftArgs &A, hipStream_t s);
// dsp_pvoc (pvoc.hip): one channel group, all of its chunks (pvoc_host.hpp
// PvocPlan): the chunks' phase sums, their carries, then the output frames
struct PvocArgs {
    ChanIn in;             // cn spectrum rows of F frames, 8-byte aligned
    ChanOut out;           // cn spectrum rows of frames_out frames, 8-byte aligned
    uint32_t cn;
    uint64_t ld_in, ld_out;  // floats, even, >= 8194
    uint64_t F, frames_out;
    double rate;
    uint32_t chunk;        // output frames per chunk
    uint64_t chunks;       // ceil(frames_out / chunk)
    uint64_t c0;           // set by the launch: its first chunk
    uint32_t *S;           // [cn][chunks][4097]
    uint32_t variant;      // 0: the product; else the A/B bits of DSP_DEBUG_PVOC_VARIANT (pvoc.hip)
    uint32_t *inc;         // variant bit 4 only: [cn][frames_out][4097] increments
};
int launch_pvoc(const PvocArgs &A, hipStream_t s);
// dsp_decay (decay.hip): peak and onset of a channel group; the band masks of
// a group of (channel, band) rows; the rows' hop sums (decay_host.hpp has the
// scratch layout)
struct DecayArgs {
    ChanIn in;                  // onset: cn unfiltered rows
    uint32_t cn;
    uint64_t L;
    float *peak;                // onset: the group's first channel
    unsigned long long *onset;  // onset: the group's first channel; hops: the call's channel 0
    uint32_t nrows;             // mask, hops: rows of this group
    uint32_t bins;              // n / 2 + 1
    const v2f *X;               // channel spectra, [..][bins]
    v2f *Y;                     // [nrows][bins] band spectra
    uint32_t xrow[kMaxChannels];   // a row's spectrum in X
    uint32_t chan[kMaxChannels];   // a row's channel of the call
    float fscale[kMaxChannels];    // sr / (n fm): bin k lies at f / fm = k fscale
    float Qd;
    const float *ir;            // [nrows][Lp] band-filtered rows
    uint64_t Lp;
    double *energy[kMaxChannels];  // output rows of `hops`
    double *moment[kMaxChannels];  // or NULL
    double *pre;                // [nrows][2][hops] sums of the pieces before the onset: energy, moment
    uint32_t hop;
    uint64_t hops;
};
int launch_decay_onset(const DecayArgs &A, hipStream_t s);
int launch_decay_mask(const DecayArgs &A, hipStream_t s);
int launch_decay_hops(const DecayArgs &A, hipStream_t s);
int launch_minmax(const float *x, uint64_t n, uint32_t P, float *vmax, float *vmin, hipStream_t s);
int launch_spectro(const float *mag, uint64_t F, uint32_t K, uint64_t ld, uint32_t P, float *out,
                   hipStream_t s);
int launch_wav_decode(const uint8_t *payload, uint32_t C, uint16_t bits, bool is_float, uint64_t frame0,
                      uint64_t frames, const ChanOut &out, bool out_aligned16, hipStream_t s);
int launch_wav_encode(uint8_t *payload, uint32_t C, uint16_t bits, bool is_float, uint64_t frames,
                      const ChanOut &in, hipStream_t s);
bool stft8192_pk_per_path(const Stft8kArgs &A, bool fused);
// frames per wave of the PER path's frame reuse for a launch of C channels
// (Stft8kArgs::run): 1 when the frames differ (H % B != 0), the call is not on
// the PER path or it is too short to fill the device; `forced` > 0 (test hook)
// replaces the default wherever reuse is valid
uint32_t stft8192_pk_frame_run(const Stft8kArgs &A, bool fused, uint32_t C, uint32_t forced);
int stft_pk_ab_options();  // A/B option bits of this thread: 0 unless the tools build (stft_pk_ab.hip) set them
int launch_stft8192_pk(const Stft8kArgs &A, uint32_t C, bool fused, int opt, hipStream_t s);
// the PER path with H % B == 0 from a cached spectrum row (4097 magnitudes in
// bin order): the hops and the rows of every frame, A.run frames per wave, no FFT
// pace: nap | waves << 8 (| kRowPaceRecord, which the host side reads); done: may be null
constexpr uint32_t kRowPaceMaxNap = 16, kRowPaceMinWaves = 3, kRowPaceRecord = 1u << 16;
bool row_pace_valid(uint32_t pace);
int launch_stft8192_rows(const Stft8kArgs &A, uint32_t C, const float *row, uint32_t pace, hipEvent_t done,
                         hipStream_t s);
int launch_fft_generic(const GenericFftArgs &A, uint64_t transforms, uint32_t C, hipStream_t s);
int launch_gain(const float *in, float *out, float g, uint64_t n, hipStream_t s);
int launch_set(float v, float *out, uint64_t n, hipStream_t s);
int launch_copy(const float *in, float *out, uint64_t n, hipStream_t s, bool *done);
int launch_upload(float *dst, const float *src, uint64_t n, hipStream_t s);
int launch_impulse(const ChanOut &buf, uint32_t C, uint32_t n, hipStream_t s);
int launch_magnitude(const float *re, const float *im, float *out, uint64_t n, hipStream_t s);

}  // namespace dspb
