// dspbench_render -- the offline-render command line: a C++ host that drives
// the GPU path through the C ABI only (include/dspbench/*.h), the way the
// reference's host would ("called from: the build's
// offline-render CLI").
//
//   WAV file -> dsp_wav_parse -> payload to HBM -> dsp_wav_decode (planar)
//   -> dsp_render_offline / dsp_render_stft through a plugin -> dsp_wav_encode
//   -> output WAV (+ optional magnitude spectra as raw float32).
//
// It replaces the reference's load (wav_reader.h:57-205, audio.h:66-121),
// render loop (audio.cpp:13-175, pumped by wasapi_audio.cpp:223-251) and the
// analysis FFT (dsp.cpp:53-103) for a whole file, offline.
//
//   dspbench_render IN.wav OUT.wav [options]
//     --plugin NAME     gain_test (default) | IR_test | no_op | static_gain |
//                       PATH.cpp (any reference-style plugin source, compiled
//                       for gfx950 at run time: DSP_PLUGIN_GENERIC)
//     --convolve IR.wav convolve with an impulse response (DSP_PLUGIN_CONV): the
//                       first channel of IR.wav (1..2^20 frames, decoded like the
//                       input) is the taps for every device channel.  Not with
//                       --plugin
//     --gain G          gain_test / static_gain gain (0.2 / 0.1)
//     --ir G,STEP       IR_test parameters (0.9,0.002)
//     --block B         block size (512)
//     --bits 16|24|32|float   output sample format (default: the input's)
//     --stft FILE       also write the Hann 8192 / 4096 STFT magnitudes of the
//                       render: header "DSPMAG1\0", u32 C, u32 K, u64 F, then
//                       C x F x K float32
//     --device N        GPU ordinal (0; with --world: LOCAL_RANK if set, else the rank)
//     --device-channels C   render into C device channels, as the reference's
//                       device does (always 2, wasapi_audio.cpp:432-433): file
//                       channels past C are dropped, missing ones render from
//                       zeros (audio.cpp:65-81, 138-141).  Default: the file's.
//     --device-rate R   the sample rate handed to the plugin and written to the
//                       output header (the reference ignores the WAV's own rate,
//                       wav_reader.h:7-14).  Default: the file's.
//     --rate R          convert the input from its header's rate to R on the GPU
//                       before the render (dsp_resample, default quality); R is
//                       the rate handed to the plugin and written to the output
//                       header.  With --convolve the impulse response is
//                       converted from its own header's rate to R and scaled by
//                       ir_rate / R (the filter's DC gain is kept); it must still
//                       be <= 2^20 taps.  Not with --device-rate, --loop or
//                       --comm-id
//     --stretch RATE    make the render 1 / RATE times as long at the same pitch
//                       (dsp_time_stretch: STFT, phase vocoder, inverse STFT at hop
//                       --stretch-hop, default 2048; 0.125 <= RATE <= 8; the render
//                       must hold one 8192-point frame), before --normalize, --limit
//                       and the encode.  Prints one JSON line {"stretch": {rate, p,
//                       q, hop, frames_in, frames_out, samples_in,
//                       samples_stretched, samples_out}}
//     --pitch SEMITONES shift the render's pitch by p / q ~ 2^(SEMITONES / 12)
//                       (dsp_pitch_ratio, |SEMITONES| <= 24) at its length: the
//                       render, zero-padded by whole hops as far as needed, is
//                       stretched at rate q / p to floor(frames p / q + 1 / 2) samples and
//                       converted from p to q (dsp_resample); samples_out is within
//                       one of samples_in.  The same JSON line.  Neither goes with
//                       the other, with --deconvolve, --transfer, --decay, --stft,
//                       --loop or the multi-GPU modes
//     --loudness        measure the render (its written frames, every output
//                       channel at weight 1: dsp_loudness with the true peak)
//                       and print one JSON line with the result to stdout
//     --normalize LUFS  measure, then scale the render by g = (float)10^((LUFS -
//                       integrated) / 20) before the encode; a render that
//                       measures -inf is an error
//     --true-peak-ceiling DBTP   with --normalize: lower g so that true_peak g
//                       <= 10^(DBTP / 20): the whole programme is turned down
//                       until its loudest peak fits, unless --limit is given
//     --limit           with --normalize and --true-peak-ceiling: g is not
//                       lowered; the render is scaled by g and then limited in
//                       place (dsp_limiter at the ceiling, true-peak detector,
//                       channels linked), so only the milliseconds around each
//                       peak are turned down.  The result's true peak is measured
//                       again and what is left above the ceiling is removed by a
//                       scalar gain, reported as residual_gain.  Prints the JSON
//                       line, with "limiter": {min_gain, limited, residual_gain}
//     --limit-lookahead MS   the limiter's lookahead (1.5; at most 1024 samples)
//     --limit-release MS     its release time constant (100; 0: none)
//                       None of these with --loop or the multi-GPU modes.
//                       --stft's magnitudes are those of the render before this
//                       gain (the fused render + STFT)
//     --deconvolve REF.wav   swept-sine measurement: IN.wav is the recording, the
//                       first channel of REF.wav the excitation; OUT.wav is the
//                       impulse response, one channel per input channel
//                       (dsp_deconvolve), float unless --bits says otherwise.
//                       Prints one JSON line: n, eps, pre, ir_length and each
//                       channel's peak {index, value}.  IN and REF must have the
//                       same rate.  Not with --plugin, --convolve, --loop,
//                       --stft, --rate, --loudness, --normalize or the multi-GPU
//                       modes
//     --deconv-eps E    the regularisation, 1e-12..1 (1e-6)
//     --deconv-pre N    output samples of negative time (0): where a sweep's
//                       harmonic responses land
//     --ir-length N     samples written (min(n, 2^20): usable by --convolve)
//     --psd OUT.csv     also write the average spectrum of the written render
//                       (dsp_welch, Hann 8192 / 4096, one-sided density): a
//                       header line, then per bin its frequency in Hz and each
//                       channel's 10 log10(PSD), dB re full scale^2 / Hz.  Prints
//                       one JSON line {"psd": {frames, bins, hop, channels:
//                       [{peak_hz, peak_db, power_db}]}}.  A render shorter than
//                       one frame is an error.  Not with --deconvolve, --loop or
//                       the multi-GPU modes
//     --decay OUT.csv   with --deconvolve: the room-acoustic figures of the impulse
//                       response that run writes (dsp_decay, dsp_decay_derive;
//                       its negative-time samples fall before the onset): a
//                       header line, then per channel and band the mid
//                       frequency in Hz, EDT, T20, T30 in seconds, C50, C80 in
//                       dB, D50, Ts in ms and the INR in dB; a value that is not
//                       valid is an empty cell.  Prints one JSON line {"decay":
//                       {n, hop, bands, fraction, channels: [{onset,
//                       peak_dbfs}]}}.  Not with --plugin, --convolve, --loop,
//                       --stft, --psd, --transfer, --rate or the multi-GPU modes
//     --decay-bands octave|third   31.6 Hz..16 kHz octaves (default) or 25 Hz..
//                       20 kHz third-octaves, without the bands above rate / 2
//     --loop NBLOCKS    loop mode (audio.cpp:100-132): NBLOCKS blocks from a
//                       file that wraps around (no --stft)
//   multi-GPU (cfg 5, shard.h): one process per GPU, channels sharded one
//   run per rank, the render + STFT gathered to rank 0 over RCCL (needs --stft)
//     --world W --rank R    W processes, this one's rank (default: WORLD_SIZE /
//                       RANK from the environment when --comm-id is given)
//     --comm-id FILE    rendezvous file: rank 0 writes the RCCL id and the run
//                       id, the others wait for a file carrying their run id;
//                       rank 0 removes it once every rank has joined
//     --run-id STR      this launch's id (default: DSPB_RUN_ID, else
//                       TORCHELASTIC_RUN_ID, else none: then a file older than
//                       this process's start is taken as stale and ignored)
//     --chunk S         pipeline chunk in samples (default 16 Mi)
//
// dspbench_render --sweep F1:F2:SECONDS[:RATE[:BITS]] OUT.wav
//   writes the exponential sine sweep of dsp_sweep (F1..F2 Hz over SECONDS, at
//   RATE, default 48000, as BITS 16|24|32|float, default float; amplitude 0.5
//   with 10 ms fades) as a mono WAV: the excitation of a measurement that
//   --deconvolve evaluates.  Host only: no device is opened.
//
// dspbench_render REC.wav OUT.csv --transfer REF.wav
//   the transfer function from the first channel of REF.wav to each channel of
//   REC.wav (dsp_welch with a reference, Hann 8192 / 4096; dsp_welch_derive):
//   OUT.csv holds a header line, then per bin its frequency in Hz and per
//   channel |H1| in dB, H1's phase in radians and the coherence.  Prints one
//   JSON line {"transfer": {frames, bins, hop, channels: [{mean_coherence,
//   min_coherence, gain_db}]}}.  Nothing is resampled or aligned: files of
//   different rates or lengths, or shorter than one frame, are refused.
//
// dspbench_render IR.wav --decay OUT.csv [--decay-bands octave|third]
//   the same analysis of an impulse response that is already a file: the CSV
//   and the JSON line of --decay above.
//
// options.cpp reads the command line, device.hpp owns what lives on the device,
// wavio.cpp is the one WAV loader and the one writer; here are the five modes.
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <ctime>

#include "dspbench/shard.h"
#include "options.hpp"
#include "wavio.hpp"

namespace {

constexpr uint32_t N = 8192, H = 4096, K = N / 2 + 1;  // --stft: Hann 8192 / 4096

// rank 0 writes the RCCL id and the run id to `path` (atomically: a temp
// file renamed); the other ranks wait up to two minutes for a file carrying
// their run id -- or, without one, a file written after they started -- so a
// file a previous launch left behind is never read
bool exchange_comm_id(const std::string &path, uint32_t rank, const std::string &run_id, time_t started,
                      unsigned char *id) {
    if (rank == 0) {
        if (dsp_comm_unique_id(id)) return false;
        const std::string tmp = path + ".tmp";
        FILE *f = std::fopen(tmp.c_str(), "wb");
        if (!f) return false;
        const bool ok = std::fwrite(id, 1, DSP_COMM_ID_BYTES, f) == DSP_COMM_ID_BYTES &&
                        std::fwrite(run_id.data(), 1, run_id.size(), f) == run_id.size();
        std::fclose(f);
        return ok && std::rename(tmp.c_str(), path.c_str()) == 0;
    }
    std::vector<unsigned char> buf(DSP_COMM_ID_BYTES + run_id.size() + 1);
    int tries = 1200;  // two minutes; DSPB_COMM_WAIT_S shortens it (tests)
    if (const char *w = std::getenv("DSPB_COMM_WAIT_S")) tries = std::max(1, std::atoi(w) * 10);
    for (int i = 0; i < tries; ++i, usleep(100000)) {
        struct stat sb;
        if (stat(path.c_str(), &sb) != 0) continue;
        if (run_id.empty() && sb.st_mtime < started) continue;  // stale: before this launch
        FILE *f = std::fopen(path.c_str(), "rb");
        if (!f) continue;
        const size_t n = std::fread(buf.data(), 1, buf.size(), f);
        std::fclose(f);
        if (n != DSP_COMM_ID_BYTES + run_id.size()) continue;  // another launch's run id (or a partial file)
        if (std::memcmp(buf.data() + DSP_COMM_ID_BYTES, run_id.data(), run_id.size()) != 0) continue;
        std::memcpy(id, buf.data(), DSP_COMM_ID_BYTES);
        return true;
    }
    return false;
}

// a double as a JSON number (Python's json reads the three non-finite tokens)
std::string json_num(double v) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v < 0 ? "-Infinity" : "Infinity";
    char b[40];
    std::snprintf(b, sizeof b, "%.17g", v);
    return b;
}

// ---- --sweep: the excitation as a mono WAV, host only ------------------------
int run_sweep(const Options &o) {
    dsp_sweep_spec sp{};
    sp.amplitude = 0.5, sp.f1 = o.sweep_f1, sp.f2 = o.sweep_f2, sp.seconds = o.sweep_seconds;
    const unsigned rate = o.sweep_rate;
    uint64_t L = 0;
    int st = dsp_sweep_plan(rate, &sp, &L, nullptr);
    if (st) return fail("dsp_sweep_plan", st);
    sp.fade = (uint32_t)std::min<uint64_t>(rate / 100, L / 2);  // 10 ms at each end
    std::vector<float> x(L);
    if ((st = dsp_sweep(rate, &sp, x.data(), L))) return fail("dsp_sweep", st);
    const Format f = resolve_bits(o.sweep_bits, {});
    const size_t bps = f.bits / 8u;
    WavOut w;
    if (int e = wav_header(w, f, 1, rate, L)) return e;
    for (uint64_t i = 0; i < L; ++i) {  // dsp_wav_encode's rounding, on the host
        uint32_t code;
        if (f.fmt == DSP_WAV_FORMAT_FLOAT) std::memcpy(&code, &x[i], 4);
        else if (f.bits == 32) {
            const double r = std::min(std::max(std::rint((double)x[i] * 2147483648.0), -2147483648.0), 2147483647.0);
            code = (uint32_t)(int32_t)r;
        } else {
            const float S = f.bits == 16 ? 32768.f : 8388608.f;
            code = (uint32_t)(int32_t)std::fmin(std::fmax(std::rint(x[i] * S), -S), S - 1.f);
        }
        for (size_t b = 0; b < bps; ++b) w.bytes[w.hdr + i * bps + b] = (unsigned char)(code >> (8 * b));
    }
    if (int e = write_file(o.out_path.c_str(), {{w.bytes.data(), w.size}})) return e;
    std::printf("dspbench_render: sweep %g..%g Hz, %llu frames @ %u Hz -> %s (%s)\n", sp.f1, sp.f2,
                (unsigned long long)L, rate, o.out_path.c_str(), o.sweep_bits.c_str());
    return 0;
}

// the input file, for both device modes: refused before the device is opened
int load_input(const Options &o, Device &dev, Wav &in) {
    return load_wav(o.in_path.c_str(), "", [&](const dsp_wav_info &i) {
        const uint32_t C = o.dev_channels ? o.dev_channels : i.channels;
        if (i.channels == 0 || i.channels > 16 || C == 0 || C > 16) {
            std::fprintf(stderr, "dspbench_render: %u file / %u device channels (1..16 supported)\n", i.channels, C);
            return 1;
        }
        return 0;
    }, dev, in);
}

// ---- --decay: ISO 3382 figures of device rows (impulse responses) -----------
int write_decay(const Options &o, float *const *rows, uint32_t C, uint64_t L, uint32_t rate, Device &dev) {
    dsp_decay_spec sp = o.decay_bands == "third" ? dsp_decay_spec{3u, -16, 13} : dsp_decay_spec{1u, -5, 4};
    // without the bands whose upper edge lies above rate / 2
    while (sp.k_hi > sp.k_lo && 1000.0 * std::pow(10.0, 0.3 * (sp.k_hi + 0.5) / sp.fraction) > 0.5 * rate) --sp.k_hi;
    uint32_t n = 0, hop = 0, B = 0;
    uint64_t hops = 0;
    double fm[32];
    int st = dsp_decay_plan(L, C, rate, &sp, &n, nullptr, &hop, &B, &hops, nullptr, fm);
    if (st) return fail("dsp_decay_plan", st);
    const size_t R = (size_t)C * B, row = hops;
    DevBuf buf;  // [2][R][hops] float64, then the onsets and the peaks
    HIPCK(hipMalloc(&buf.h, 2 * R * row * sizeof(double) + C * (sizeof(uint64_t) + sizeof(float))));
    double *de = (double *)buf.h, *dm = de + R * row;
    uint64_t *donset = (uint64_t *)(dm + R * row);
    float *dpeak = (float *)(donset + C);
    std::vector<double *> pe(R), pm(R);
    for (size_t r = 0; r < R; ++r) pe[r] = de + r * row, pm[r] = dm + r * row;
    if ((st = dsp_decay(rows, C, L, rate, &sp, dpeak, donset, pe.data(), pm.data(), &dev.ex))) return fail("dsp_decay", st);
    std::vector<double> h(2 * R * row);
    std::vector<uint64_t> onset(C);
    std::vector<float> peak(C);
    HIPCK(hipMemcpyAsync(h.data(), de, h.size() * sizeof(double), hipMemcpyDeviceToHost, dev.stream.h));
    HIPCK(hipMemcpyAsync(onset.data(), donset, C * sizeof(uint64_t), hipMemcpyDeviceToHost, dev.stream.h));
    HIPCK(hipMemcpyAsync(peak.data(), dpeak, C * sizeof(float), hipMemcpyDeviceToHost, dev.stream.h));
    HIPCK(hipStreamSynchronize(dev.stream.h));
    std::string csv = "channel,fm_hz,edt_s,t20_s,t30_s,c50_db,c80_db,d50,ts_ms,inr_db\n";
    std::string j = "{\"decay\": {\"n\": " + std::to_string(n) + ", \"hop\": " + std::to_string(hop) + ", \"bands\": " +
                    std::to_string(B) + ", \"fraction\": " + std::to_string(sp.fraction) + ", \"channels\": [";
    char b[48];
    for (uint32_t c = 0; c < C; ++c) {
        j += std::string(c ? ", " : "") + "{\"onset\": " + std::to_string(onset[c]) + ", \"peak_dbfs\": " +
             json_num(20.0 * std::log10((double)peak[c])) + "}";
        for (uint32_t k = 0; k < B; ++k) {
            const size_t r = (size_t)c * B + k;
            dsp_decay_result res;
            if ((st = dsp_decay_derive(&h[r * row], &h[(R + r) * row], L, onset[c], hop, rate, &res)))
                return fail("dsp_decay_derive", st);
            std::snprintf(b, sizeof b, "%u,%.9g", c, fm[k]);
            csv += b;
            const double v[8] = {res.edt, res.t20, res.t30, res.c50, res.c80, res.d50, 1e3 * res.ts, res.inr};
            for (double x : v) {
                if (std::isnan(x)) b[0] = ',', b[1] = 0;  // not valid: an empty cell
                else std::snprintf(b, sizeof b, ",%.9g", x);
                csv += b;
            }
            csv += "\n";
        }
    }
    if (int e = write_file(o.decay_path.c_str(), {{csv.data(), csv.size()}})) return e;
    std::printf("%s]}}\n", j.c_str());
    return 0;
}

// ---- IR.wav --decay OUT.csv: the analysis of a file ---------------------------
int run_decay(const Options &o) {
    Device dev(o.device);
    Wav in;
    if (int e = load_input(o, dev, in)) return e;
    if (in.info.frames == 0) {
        std::fprintf(stderr, "dspbench_render: --decay: %s is empty\n", o.in_path.c_str());
        return 1;
    }
    if (int e = write_decay(o, in.rows.ptr.data(), in.info.channels, in.info.frames, in.info.sample_rate, dev)) return e;
    std::printf("dspbench_render: %s: %u ch x %llu frames @ %u Hz, decay analysis -> %s, %.1f ms end to end\n",
                o.in_path.c_str(), in.info.channels, (unsigned long long)in.info.frames, in.info.sample_rate,
                o.decay_path.c_str(), dev.ms());
    return 0;
}

// ---- --deconvolve: the recording deconvolved by REF's first channel ---------
int run_deconvolve(const Options &o) {
    Device dev(o.device);
    Wav in, ref;
    if (int e = load_input(o, dev, in)) return e;
    const uint32_t Cf = in.info.channels, rate = in.info.sample_rate;
    const uint64_t L = in.info.frames;
    const char *ref_path = o.deconv_path.c_str();
    if (int e = load_wav(ref_path, " (excitation)", [&](const dsp_wav_info &ri) {
            if (ri.sample_rate != rate) {
                std::fprintf(stderr, "dspbench_render: --deconvolve: %s is at %u Hz, %s at %u Hz\n", ref_path,
                             ri.sample_rate, o.in_path.c_str(), rate);
                return 1;
            }
            if (ri.frames == 0 || L == 0 || ri.channels == 0 || ri.channels > 16) {
                std::fprintf(stderr, "dspbench_render: --deconvolve: an empty recording or excitation\n");
                return 1;
            }
            return 0;
        }, dev, ref))
        return e;
    uint32_t n = 0;
    int st = dsp_deconv_plan(L, ref.info.frames, Cf, &n, nullptr);
    if (st) return fail("dsp_deconv_plan", st);
    const uint64_t irl = o.ir_length ? o.ir_length : std::min<uint64_t>(n, 1u << 20);
    if (irl > n || o.deconv_pre > irl) {
        std::fprintf(stderr, "dspbench_render: --deconvolve: needs --deconv-pre <= --ir-length <= n = %u\n", n);
        return 2;
    }
    Rows ir;
    HIPCK(ir.alloc(Cf, irl));
    dsp_deconv_spec ds{};
    ds.eps = o.deconv_eps;
    ds.pre = (uint32_t)o.deconv_pre;
    if ((st = dsp_deconvolve(in.rows.ptr.data(), Cf, L, ref.rows.ptr[0], ref.info.frames, ir.ptr.data(), irl, &ds, &dev.ex)))
        return fail("dsp_deconvolve", st);
    WavOut w;
    if (int e = queue_wav(ir, Cf, irl, rate, resolve_bits(o.bits, {DSP_WAV_FORMAT_FLOAT, 32}), dev, w)) return e;
    std::vector<float> h(irl);
    std::string j = "{\"n\": " + std::to_string(n) + ", \"eps\": " + json_num(o.deconv_eps) + ", \"pre\": " +
                    std::to_string(o.deconv_pre) + ", \"ir_length\": " + std::to_string(irl) + ", \"peaks\": [";
    for (uint32_t c = 0; c < Cf; ++c) {  // each channel's peak
        HIPCK(hipMemcpyAsync(h.data(), ir.ptr[c], irl * sizeof(float), hipMemcpyDeviceToHost, dev.stream.h));
        HIPCK(hipStreamSynchronize(dev.stream.h));
        uint64_t at = 0;
        for (uint64_t i = 1; i < irl; ++i)
            if (std::fabs(h[i]) > std::fabs(h[at])) at = i;
        j += std::string(c ? ", " : "") + "{\"index\": " + std::to_string(at) + ", \"value\": " +
             json_num((double)h[at]) + "}";
    }
    std::printf("%s]}\n", j.c_str());
    if (int e = write_file(o.out_path.c_str(), {{w.bytes.data(), w.size}})) return e;
    if (!o.decay_path.empty())  // of the rows the file holds (before its sample format)
        if (int e = write_decay(o, ir.ptr.data(), Cf, irl, rate, dev)) return e;
    std::printf("dspbench_render: %s deconvolved by %s: %u ch x %llu frames @ %u Hz -> %s (n = %u), %.1f ms end to end\n",
                o.in_path.c_str(), ref_path, Cf, (unsigned long long)irl, rate, o.out_path.c_str(), n, dev.ms());
    return 0;
}

// ---- --psd / --transfer: Welch sums of device rows, on the host ---------------
struct WelchSums {
    uint64_t frames = 0;
    double win_sum = 0.0, win_sumsq = 0.0;
    std::vector<double> sxx, srr, sxy;  // [C][K], [K], [C][2 K]
};

// dsp_welch (Hann 8192 / 4096) of C rows of L samples, with the row ref when there is one
int welch_sums(float *const *rows, uint32_t C, uint64_t L, const float *ref, Device &dev, WelchSums &w) {
    int st = dsp_welch_plan(L, C, ref != nullptr, nullptr, &w.frames, nullptr, nullptr, nullptr, &w.win_sum, &w.win_sumsq);
    if (st) return fail("dsp_welch_plan", st);
    const size_t per = (size_t)K * (ref ? 3 : 1);  // doubles per channel: sxx, then sxy
    DevBuf buf;
    HIPCK(hipMalloc(&buf.h, ((size_t)C * per + K) * sizeof(double)));
    double *base = (double *)buf.h, *drr = base + (size_t)C * per;
    std::vector<double *> dxx(C), dxy(C);
    for (uint32_t c = 0; c < C; ++c) dxx[c] = base + c * per, dxy[c] = dxx[c] + K;
    if ((st = dsp_welch(rows, C, L, ref, dxx.data(), ref ? drr : nullptr, ref ? dxy.data() : nullptr, nullptr, &dev.ex)))
        return fail("dsp_welch", st);
    std::vector<double> host((size_t)C * per + K);
    HIPCK(hipMemcpyAsync(host.data(), base, host.size() * sizeof(double), hipMemcpyDeviceToHost, dev.stream.h));
    HIPCK(hipStreamSynchronize(dev.stream.h));
    w.sxx.resize((size_t)C * K);
    if (ref) w.sxy.resize((size_t)C * 2 * K), w.srr.assign(host.end() - K, host.end());
    for (uint32_t c = 0; c < C; ++c) {
        std::copy_n(host.begin() + c * per, K, w.sxx.begin() + (size_t)c * K);
        if (ref) std::copy_n(host.begin() + c * per + K, 2 * K, w.sxy.begin() + (size_t)c * 2 * K);
    }
    return 0;
}

// row pointers into a [C][n] vector
std::vector<double *> row_table(std::vector<double> &v, uint32_t C, size_t n) {
    std::vector<double *> t(C);
    for (uint32_t c = 0; c < C; ++c) t[c] = v.data() + c * n;
    return t;
}

// a CSV: the header line, then per bin its frequency and `cols` values
int write_csv(const char *path, const std::string &header, uint32_t rate, const std::vector<std::vector<double>> &cols) {
    std::string s = header + "\n";
    char b[48];
    for (uint32_t k = 0; k < K; ++k) {
        std::snprintf(b, sizeof b, "%.9g", (double)k * (double)rate / (double)N);
        s += b;
        for (const auto &col : cols) std::snprintf(b, sizeof b, ",%.9g", col[k]), s += b;
        s += "\n";
    }
    return write_file(path, {{s.data(), s.size()}});
}

// --psd: the average spectrum of rows (the render) as dB re full scale^2 / Hz, and its JSON line
int write_psd(const Options &o, float *const *rows, uint32_t C, uint64_t L, uint32_t rate, Device &dev) {
    WelchSums w;
    if (int e = welch_sums(rows, C, L, nullptr, dev, w)) return e;
    std::vector<double> psd((size_t)C * K);
    const std::vector<double *> xx = row_table(w.sxx, C, K), pp = row_table(psd, C, K);
    int st = dsp_welch_derive(xx.data(), nullptr, nullptr, C, K, w.frames, (double)rate, w.win_sum, w.win_sumsq, 0,
                              pp.data(), nullptr, nullptr);
    if (st) return fail("dsp_welch_derive", st);
    std::string header = "hz", j = "{\"psd\": {\"frames\": " + std::to_string(w.frames) + ", \"bins\": " +
                                   std::to_string(K) + ", \"hop\": " + std::to_string(H) + ", \"channels\": [";
    std::vector<std::vector<double>> cols(C, std::vector<double>(K));
    for (uint32_t c = 0; c < C; ++c) {
        header += ",ch" + std::to_string(c) + "_db";
        uint32_t at = 0;
        double power = 0.0;  // the integral of the density: the mean square of the windowed signal
        for (uint32_t k = 0; k < K; ++k) {
            const double v = pp[c][k];
            cols[c][k] = 10.0 * std::log10(v);
            power += v * (double)rate / (double)N;
            if (v > pp[c][at]) at = k;
        }
        j += std::string(c ? ", " : "") + "{\"peak_hz\": " + json_num((double)at * rate / N) + ", \"peak_db\": " +
             json_num(cols[c][at]) + ", \"power_db\": " + json_num(10.0 * std::log10(power)) + "}";
    }
    if (int e = write_csv(o.psd_path.c_str(), header, rate, cols)) return e;
    std::printf("%s]}}\n", j.c_str());
    return 0;
}

// ---- --transfer: H1 and coherence from REF's first channel to the recording ---
int run_transfer(const Options &o) {
    Device dev(o.device);
    Wav in, ref;
    if (int e = load_wav(o.in_path.c_str(), "", [&](const dsp_wav_info &i) {
            if (i.channels == 0 || i.channels > 16) {
                std::fprintf(stderr, "dspbench_render: %u file channels (1..16 supported)\n", i.channels);
                return 1;
            }
            if (i.frames < N) {
                std::fprintf(stderr, "dspbench_render: --transfer: %s has %llu frames, fewer than one %u-point frame\n",
                             o.in_path.c_str(), (unsigned long long)i.frames, N);
                return 1;
            }
            return 0;
        }, dev, in))
        return e;
    const uint32_t C = in.info.channels, rate = in.info.sample_rate;
    const uint64_t L = in.info.frames;
    const char *ref_path = o.transfer_path.c_str();
    if (int e = load_wav(ref_path, " (reference)", [&](const dsp_wav_info &ri) {
            if (ri.sample_rate != rate) {
                std::fprintf(stderr, "dspbench_render: --transfer: %s is at %u Hz, %s at %u Hz\n", ref_path, ri.sample_rate,
                             o.in_path.c_str(), rate);
                return 1;
            }
            if (ri.frames != L || ri.channels == 0 || ri.channels > 16) {
                std::fprintf(stderr, "dspbench_render: --transfer: %s has %llu frames, %s %llu (nothing is resampled or "
                                     "aligned)\n", ref_path, (unsigned long long)ri.frames, o.in_path.c_str(),
                             (unsigned long long)L);
                return 1;
            }
            return 0;
        }, dev, ref))
        return e;
    WelchSums w;
    if (int e = welch_sums(in.rows.ptr.data(), C, L, ref.rows.ptr[0], dev, w)) return e;
    std::vector<double> h1((size_t)C * 2 * K), coh((size_t)C * K);
    const std::vector<double *> xx = row_table(w.sxx, C, K), xy = row_table(w.sxy, C, 2 * K), hh = row_table(h1, C, 2 * K),
                                cc = row_table(coh, C, K);
    int st = dsp_welch_derive(xx.data(), w.srr.data(), xy.data(), C, K, w.frames, (double)rate, w.win_sum, w.win_sumsq, 0,
                              nullptr, hh.data(), cc.data());
    if (st) return fail("dsp_welch_derive", st);
    std::string header = "hz", j = "{\"transfer\": {\"frames\": " + std::to_string(w.frames) + ", \"bins\": " +
                                   std::to_string(K) + ", \"hop\": " + std::to_string(H) + ", \"channels\": [";
    std::vector<std::vector<double>> cols;
    double rr = 0.0;
    for (uint32_t k = 0; k < K; ++k) rr += w.srr[k];
    for (uint32_t c = 0; c < C; ++c) {
        const std::string n = "ch" + std::to_string(c);
        header += "," + n + "_h1_db," + n + "_phase_rad," + n + "_coherence";
        std::vector<double> db(K), ph(K), g(cc[c], cc[c] + K);
        double mean = 0.0, low = 1.0, power = 0.0;
        for (uint32_t k = 0; k < K; ++k) {
            const double re = hh[c][2 * k], im = hh[c][2 * k + 1];
            db[k] = 20.0 * std::log10(std::hypot(re, im));
            ph[k] = std::atan2(im, re);
            mean += g[k] / K, low = std::min(low, g[k]), power += xx[c][k];
        }
        j += std::string(c ? ", " : "") + "{\"mean_coherence\": " + json_num(mean) + ", \"min_coherence\": " + json_num(low) +
             ", \"gain_db\": " + json_num(10.0 * std::log10(power / rr)) + "}";
        cols.push_back(std::move(db)), cols.push_back(std::move(ph)), cols.push_back(std::move(g));
    }
    if (int e = write_csv(o.out_path.c_str(), header, rate, cols)) return e;
    std::printf("%s]}}\n", j.c_str());
    std::printf("dspbench_render: %s against %s: %u ch x %llu frames @ %u Hz, %llu Welch frames -> %s, %.1f ms end to end\n",
                o.in_path.c_str(), ref_path, C, (unsigned long long)L, rate, (unsigned long long)w.frames,
                o.out_path.c_str(), dev.ms());
    return 0;
}

// ---- the render: what its stages hand on ------------------------------------
struct Render {
    const Options &o;
    Device dev;
    Wav in;
    uint32_t Cf = 0, C = 0, Cin = 0, rate = 0;  // the file's channels, the device's, channels_to_write (audio.cpp:66)
    uint64_t L = 0, nblocks = 0, Lr = 0, F = 0;  // input frames (--rate: converted), blocks, frames and STFT frames rendered
    Rows out, mag;
    dsp_plugin p{};
    float pv[2] = {0.f, 0.f};
    Module mod;
    std::vector<unsigned char> gparams;
    std::vector<float> taps;
    Event e0, e1;
    dsp_comm *comm = nullptr;
    explicit Render(const Options &opt) : o(opt), dev(opt.device) {}
};

// --convolve: the IR file's first channel as the taps, at the render's rate
int load_taps(Render &r) {
    const Options &o = r.o;
    const char *path = o.conv_path.c_str();
    Wav ir;
    if (int e = load_wav(path, " (impulse response)", [&](const dsp_wav_info &ii) {
            if (ii.frames == 0 || ii.frames > (1u << 20) || ii.channels == 0 || ii.channels > 16) {
                std::fprintf(stderr, "dspbench_render: %s: %llu frames, %u channels (1..2^20 frames, 1..16 channels)\n",
                             path, (unsigned long long)ii.frames, ii.channels);
                return 1;
            }
            return 0;
        }, r.dev, ir))
        return e;
    uint64_t ntaps = ir.info.frames;
    float tap_scale = 1.f;
    if (o.rate && o.rate != ir.info.sample_rate) {  // --rate: the response at the render's rate, DC gain kept
        if (int e = resample_rows(ir.rows, 1, ntaps, ir.info.sample_rate, o.rate, " (impulse response)", [&](uint64_t n) {
                if (n == 0 || n > (1u << 20)) {
                    std::fprintf(stderr, "dspbench_render: %s: %llu taps at %u Hz (1..2^20 supported)\n", path,
                                 (unsigned long long)n, o.rate);
                    return 1;
                }
                return 0;
            }, r.dev))
            return e;
        tap_scale = (float)((double)ir.info.sample_rate / (double)o.rate);
    }
    r.taps.resize(ntaps);
    HIPCK(hipMemcpyAsync(r.taps.data(), ir.rows.ptr[0], ntaps * sizeof(float), hipMemcpyDeviceToHost, r.dev.stream.h));
    HIPCK(hipStreamSynchronize(r.dev.stream.h));
    if (tap_scale != 1.f)
        for (float &t : r.taps) t *= tap_scale;
    return 0;
}

// a plugin source file: compile for gfx950, load, defaults, state
int load_module(Render &r) {
    const char *path = r.o.plugin.c_str();
    std::vector<unsigned char> src;
    if (!read_file(path, src)) {
        std::fprintf(stderr, "dspbench_render: cannot read plugin %s\n", path);
        return 1;
    }
    src.push_back(0);
    void *code = nullptr;
    uint64_t code_size = 0;
    std::vector<char> log(1 << 16);
    int st = dsp_module_compile((const char *)src.data(), path, &code, &code_size, log.data(), log.size());
    if (st) {
        std::fprintf(stderr, "%s\n", log.data());
        return fail("dsp_module_compile", st);
    }
    st = dsp_module_load(code, code_size, r.dev.device, &r.mod.h);
    dsp_module_free_code(code);
    if (st) return fail("dsp_module_load", st);
    uint32_t ps = 0, ss = 0;
    int stateless = 0;
    if ((st = dsp_module_sizes(r.mod.h, &ps, &ss, &stateless))) return fail("dsp_module_sizes", st);
    r.gparams.resize(ps ? ps : 1);
    if ((st = dsp_module_default_parameters(r.mod.h, r.gparams.data()))) return fail("dsp_module_default_parameters", st);
    if ((st = dsp_module_initialize_state(r.mod.h, r.gparams.data(), r.C, (float)r.rate, 16u << 20)))
        return fail("dsp_module_initialize_state", st);
    r.p.kind = DSP_PLUGIN_GENERIC, r.p.params = r.gparams.data(), r.p.params_size = ps, r.p.module = r.mod.h;
    return 0;
}

int make_plugin(Render &r) {
    const Options &o = r.o;
    dsp_plugin &p = r.p;
    float *pv = r.pv;
    if (!o.conv_path.empty()) {
        if (int e = load_taps(r)) return e;
        p.kind = DSP_PLUGIN_CONV, p.params = r.taps.data(), p.params_size = (uint32_t)(r.taps.size() * sizeof(float));
    } else if (o.plugin == "gain_test") {
        pv[0] = o.gain >= 0.f ? o.gain : 0.2f;  // build/gain_test.cpp:23
        p.kind = DSP_PLUGIN_GAIN, p.params = pv, p.params_size = 4;
    } else if (o.plugin == "static_gain") {
        pv[0] = o.gain >= 0.f ? o.gain : 0.1f;  // test/static_gain_plugin.cpp:22
        p.kind = DSP_PLUGIN_STATIC_GAIN, p.state = pv, p.state_size = 4;
    } else if (o.plugin == "IR_test") {
        pv[0] = o.ir_gain, pv[1] = o.ir_step;  // build/IR_test.cpp:24
        p.kind = DSP_PLUGIN_IR_RAMP, p.params = pv, p.params_size = 8;
    } else if (o.plugin == "no_op") {
        p.kind = DSP_PLUGIN_NOOP;
    } else {
        return load_module(r);
    }
    return 0;
}

// cfg 5: this rank renders + STFTs its run of channels, rank 0 gathers every
// channel (out / mag hold the whole file there)
int render_sharded(Render &r) {
    const Options &o = r.o;
    const bool root = o.rank == 0;
    dsp_shard sh{};
    int st = dsp_shard_plan(r.L, r.C, o.world, o.rank, o.block, N, H, DSP_SHARD_CHANNELS, 1, &sh);
    if (st) return fail("dsp_shard_plan", st);
    Rows lown, lmag;  // this rank's run: renders (the root's are rows of r.out) and spectra
    if (!root) HIPCK(lown.alloc(sh.channels, r.Lr));
    HIPCK(lmag.alloc(sh.channels, (r.F ? r.F : 1) * K));
    if (root) HIPCK(r.mag.alloc(r.C, (r.F ? r.F : 1) * K));
    std::vector<float *> lout(sh.channels);
    std::vector<const float *> lin;
    for (uint32_t j = 0; j < sh.channels; ++j) {
        const uint32_t c = sh.chan0 + j;
        if (c < r.Cin) lin.push_back(r.in.rows.ptr[c]);
        lout[j] = root ? r.out.ptr[c] : lown.ptr[j];
    }
    st = dsp_render_stft_sharded(lin.data(), (uint32_t)lin.size(), r.L, lout.data(), lmag.ptr.data(), K, r.C, o.block,
                                 (float)r.rate, &r.p, N, H, DSP_WIN_HANN, K, &sh, o.chunk, r.comm, 0,
                                 root ? r.out.ptr.data() : nullptr, root ? r.mag.ptr.data() : nullptr, &r.dev.ex);
    if (st) return fail("dsp_render_stft_sharded", st);
    HIPCK(hipStreamSynchronize(r.dev.stream.h));
    return 0;
}

// the render (+ STFT) between the two events, as one of sharded / loop / stft / offline
int render(Render &r, time_t started) {
    const Options &o = r.o;
    const float sr = (float)r.rate;
    const uint32_t B = o.block;
    float *const *in = r.in.rows.ptr.data(), *const *out = r.out.ptr.data();
    hipStream_t s = r.dev.stream.h;
    r.F = o.stft_path.empty() ? 0 : dsp_stft_frame_count(r.Lr, N, H);
    HIPCK(hipEventCreate(&r.e0.h));
    HIPCK(hipEventCreate(&r.e1.h));
    int st = 0;
    if (o.multi()) {
        unsigned char id[DSP_COMM_ID_BYTES];
        if (!exchange_comm_id(o.comm_path, o.rank, o.run_id, started, id)) {
            std::fprintf(stderr, "dspbench_render: rank %u: no communicator id at %s\n", o.rank, o.comm_path.c_str());
            return 1;
        }
        if ((st = dsp_comm_init(id, o.world, o.rank, r.dev.device, &r.comm))) return fail("dsp_comm_init", st);
        // every rank has joined (the init is collective): the id is spent
        if (o.rank == 0) (void)std::remove(o.comm_path.c_str());
    }
    HIPCK(hipEventRecord(r.e0.h, s));
    if (o.multi()) {
        if (int e = render_sharded(r)) return e;
    } else if (o.loop_blocks) {
        uint64_t cursor = 0;
        if ((st = dsp_render_loop(in, r.Cin, r.L, 0, out, r.C, B, r.nblocks, sr, &r.p, &cursor, &r.dev.ex)))
            return fail("dsp_render_loop", st);
    } else if (r.F > 0) {
        HIPCK(r.mag.alloc(r.C, r.F * K));
        st = dsp_render_stft(in, r.Cin, r.L, out, r.C, B, sr, &r.p, N, H, DSP_WIN_HANN, K, r.mag.ptr.data(), K, &r.dev.ex);
        if (st) return fail("dsp_render_stft", st);
    } else {
        if ((st = dsp_render_offline(in, r.Cin, r.L, out, r.C, B, sr, &r.p, &r.dev.ex))) return fail("dsp_render_offline", st);
    }
    HIPCK(hipEventRecord(r.e1.h, s));
    return 0;
}

// --stretch RATE / --pitch SEMITONES: the render made 1 / RATE times as long at its pitch
// (dsp_time_stretch), or shifted by p / q ~ 2^(SEMITONES / 12) at its length: stretched at rate
// q / p and converted from p to q (dsp_resample) by dsp_pitch_shift_plan's lengths: the render
// zero-padded by whole hops until the stretch reaches floor(Lr p / q + 1 / 2) samples.  One JSON line tells the figures.
int stretch(Render &r) {
    const Options &o = r.o;
    hipStream_t s = r.dev.stream.h;
    uint32_t p = 1, q = 1;
    int st;
    dsp_stretch_spec sp{o.stretch_rate, N, o.stretch_hop, DSP_WIN_HANN, 1e-10};
    const uint64_t L0 = r.Lr;
    uint64_t Lin = L0, fin = 0, fout = 0, Lout = 0;
    if (o.pitch && (st = dsp_pitch_shift_plan(L0, r.C, o.pitch_semitones, o.stretch_hop, DSP_WIN_HANN, &p, &q, &sp, &Lin,
                                              &Lout, nullptr)))
        return fail("dsp_pitch_shift_plan", st);
    if ((st = dsp_time_stretch_plan(Lin, r.C, &sp, &fin, &fout, nullptr, o.pitch ? nullptr : &Lout, nullptr)))
        return fail("dsp_time_stretch_plan", st);
    const double rate = sp.rate;
    if (Lin > L0) {  // the render, then silence
        Rows padded;
        HIPCK(padded.alloc(r.C, Lin));
        for (uint32_t c = 0; c < r.C; ++c) {
            HIPCK(hipMemcpyAsync(padded.ptr[c], r.out.ptr[c], L0 * sizeof(float), hipMemcpyDeviceToDevice, s));
            HIPCK(hipMemsetAsync(padded.ptr[c] + L0, 0, (Lin - L0) * sizeof(float), s));
        }
        HIPCK(hipStreamSynchronize(s));
        for (uint32_t c = 0; c < r.C; ++c) r.out.replace(c, std::move(padded.own[c]));
    }
    Rows now;
    HIPCK(now.alloc(r.C, Lout));
    if ((st = dsp_time_stretch(r.out.ptr.data(), r.C, Lin, now.ptr.data(), Lout, &sp, &r.dev.ex)))
        return fail("dsp_time_stretch", st);
    HIPCK(hipStreamSynchronize(s));
    for (uint32_t c = 0; c < r.C; ++c) r.out.replace(c, std::move(now.own[c]));
    r.Lr = Lout;
    if (o.pitch)
        if (int e = resample_rows(r.out, r.C, r.Lr, p, q, " (--pitch)", [](uint64_t) { return 0; }, r.dev)) return e;
    std::printf("{\"stretch\": {\"rate\": %s, \"p\": %u, \"q\": %u, \"hop\": %u, \"frames_in\": %llu, "
                "\"frames_out\": %llu, \"samples_in\": %llu, \"samples_stretched\": %llu, \"samples_out\": %llu}}\n",
                json_num(rate).c_str(), p, q, o.stretch_hop, (unsigned long long)fin, (unsigned long long)fout,
                (unsigned long long)L0, (unsigned long long)Lout, (unsigned long long)r.Lr);
    return 0;
}

std::string loudness_json(const Options &o, const dsp_loudness_result &lr, float g, const dsp_limiter_result &lim,
                          float residual) {
    std::string j = "{\"integrated\": " + json_num(lr.integrated) + ", \"range\": " + json_num(lr.range) +
                    ", \"momentary_max\": " + json_num(lr.momentary_max) + ", \"short_term_max\": " +
                    json_num(lr.short_term_max) + ", \"sample_peak\": " + json_num(lr.sample_peak) +
                    ", \"true_peak\": " + json_num(lr.true_peak) + ", \"blocks\": " + std::to_string(lr.blocks) +
                    ", \"gated_blocks\": " + std::to_string(lr.gated_blocks);
    if (o.normalize) j += ", \"gain\": " + json_num((double)g);
    if (o.limit)
        j += ", \"limiter\": {\"min_gain\": " + json_num(lim.min_gain) + ", \"limited\": " + std::to_string(lim.limited) +
             ", \"residual_gain\": " + json_num((double)residual) + "}";
    return j + "}";
}

// --loudness / --normalize: the loudness of the render, and the gain to a target level
int level(Render &r) {
    const Options &o = r.o;
    float *const *out = r.out.ptr.data();
    auto measure = [&](dsp_loudness_result &lr) {
        return dsp_loudness(out, r.C, r.Lr, r.rate, nullptr, DSP_LOUDNESS_TRUE_PEAK, nullptr, nullptr, nullptr, &lr, &r.dev.ex);
    };
    // the largest gain <= g0 that keeps `peak` at or below the ceiling
    auto fit = [&](double peak, float g0) {
        const double limit = std::pow(10.0, o.ceiling_dbtp / 20.0);
        if (peak * (double)g0 > limit) {
            g0 = (float)(limit / peak);
            while (g0 > 0.f && peak * (double)g0 > limit) g0 = std::nextafterf(g0, 0.f);
        }
        return g0;
    };
    auto scale = [&](float by) {
        for (uint32_t c = 0; c < r.C; ++c)
            if (int e = dsp_gain(out[c], out[c], by, r.Lr, &r.dev.ex)) return e;
        return 0;
    };
    dsp_loudness_result lr{};
    int st = measure(lr);
    if (st) return fail("dsp_loudness", st);
    float g = 1.f, residual = 1.f;
    dsp_limiter_result lim{};
    if (o.normalize) {
        if (!std::isfinite(lr.integrated)) {
            std::fprintf(stderr, "dspbench_render: --normalize: the render's integrated loudness is %s "
                                 "(no block passes the gates)\n", json_num(lr.integrated).c_str());
            return 1;
        }
        g = (float)std::pow(10.0, (o.norm_lufs - lr.integrated) / 20.0);
        if (o.ceiling && !o.limit) g = fit(lr.true_peak, g);
        if ((st = scale(g))) return fail("dsp_gain", st);
    }
    if (o.normalize && o.limit) {
        // the level stays: the limiter turns down the peaks, then a scalar gain takes what is
        // left of the true peak above the ceiling (the limiter's gain moves between samples)
        dsp_limiter_spec ls{};
        ls.ceiling = (float)std::pow(10.0, o.ceiling_dbtp / 20.0);
        const double la = std::floor(o.limit_lookahead_ms * 1e-3 * (double)r.rate + 0.5);
        ls.lookahead = (uint32_t)(la < 1024.0 ? la : 1024.0);
        ls.release = o.limit_release_ms * 1e-3 * (double)r.rate;
        if (ls.release > 0.0 && ls.release < 1.0) ls.release = 1.0;
        ls.flags = DSP_LIMITER_TRUE_PEAK;
        if ((st = dsp_limiter(out, r.C, r.Lr, out, r.rate, &ls, nullptr, nullptr, nullptr, &lim, &r.dev.ex)))
            return fail("dsp_limiter", st);
        dsp_loudness_result after{};
        if ((st = measure(after))) return fail("dsp_loudness", st);
        residual = fit(after.true_peak, 1.f);
        if (residual != 1.f && (st = scale(residual))) return fail("dsp_gain", st);
    }
    if (o.loudness || o.limit) std::printf("%s\n", loudness_json(o, lr, g, lim, residual).c_str());
    return 0;
}

// encode the render and write it, with the spectra (header "DSPMAG1\0", u32 C, u32 K, u64 F)
int write_outputs(Render &r) {
    const Options &o = r.o;
    const uint64_t F = r.F;
    hipStream_t s = r.dev.stream.h;
    const Format f = resolve_bits(o.bits, {r.in.info.format, r.in.info.bits_per_sample});
    WavOut w;
    if (int e = queue_wav(r.out, r.C, r.Lr, r.rate, f, r.dev, w)) return e;
    std::vector<float> mag((size_t)r.C * F * K);
    float *const *dmag = r.mag.ptr.data();
    for (uint32_t c = 0; F > 0 && c < r.C; ++c)
        HIPCK(hipMemcpyAsync(mag.data() + (size_t)c * F * K, dmag[c], F * K * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    float render_ms = 0.f;
    HIPCK(hipEventElapsedTime(&render_ms, r.e0.h, r.e1.h));
    if (int e = write_file(o.out_path.c_str(), {{w.bytes.data(), w.size}})) return e;
    const uint32_t ck[2] = {r.C, K};
    if (F > 0)
        if (int e = write_file(o.stft_path.c_str(), {{"DSPMAG1", 8}, {ck, 8}, {&F, 8}, {mag.data(), mag.size() * 4}}))
            return e;
    std::printf("dspbench_render: %s: %u ch x %llu frames @ %u Hz -> %s (%s %u-bit, %llu blocks of %u)%s; "
                "render %.3f ms on the GPU, %.1f ms end to end\n",
                o.in_path.c_str(), r.C, (unsigned long long)r.L, r.rate, o.out_path.c_str(),
                f.fmt == DSP_WAV_FORMAT_FLOAT ? "float" : "PCM", f.bits, (unsigned long long)r.nblocks, o.block,
                F ? (" + STFT " + std::to_string(F) + " frames x " + std::to_string(K) + " bins").c_str() : "",
                render_ms, r.dev.ms());
    return 0;
}

// a rank other than 0 of the multi-GPU mode: only the root writes
int finish_rank(Render &r) {
    HIPCK(hipStreamSynchronize(r.dev.stream.h));
    float ms = 0.f;
    HIPCK(hipEventElapsedTime(&ms, r.e0.h, r.e1.h));
    std::printf("dspbench_render: rank %u of %u: channels rendered and gathered to rank 0 in %.3f ms\n", r.o.rank,
                r.o.world, ms);
    dsp_comm_destroy(r.comm);
    return 0;
}

// ---- the render modes: load, plugin, render, level, write -------------------
int run_render(const Options &o, time_t started) {
    Render r(o);
    if (int e = load_input(o, r.dev, r.in)) return e;
    const dsp_wav_info &info = r.in.info;
    r.Cf = info.channels;
    r.C = o.dev_channels ? o.dev_channels : r.Cf;
    r.Cin = std::min(r.Cf, r.C);
    r.rate = o.rate ? o.rate : o.dev_rate ? o.dev_rate : info.sample_rate;
    r.L = info.frames;
    if (o.rate && o.rate != info.sample_rate)  // --rate: the file at the new rate replaces the decoded one
        if (int e = resample_rows(r.in.rows, r.Cf, r.L, info.sample_rate, o.rate, "", [](uint64_t) { return 0; }, r.dev))
            return e;
    r.nblocks = o.loop_blocks ? o.loop_blocks : (r.L + o.block - 1) / o.block;
    r.Lr = r.nblocks * o.block;
    if (!o.psd_path.empty() && r.Lr < N) {
        std::fprintf(stderr, "dspbench_render: --psd: the render has %llu frames, fewer than one %u-point frame\n",
                     (unsigned long long)r.Lr, N);
        return 1;
    }
    HIPCK(r.out.alloc(r.C, r.Lr));
    r.mag.ptr.assign(r.C, nullptr);  // (--loop computes no spectra: with --stft their copy fails, as it always has)
    if (int e = make_plugin(r)) return e;
    if (int e = render(r, started)) return e;
    if (o.multi() && o.rank != 0) return finish_rank(r);
    if (o.stretches())  // before the levels and the encode: they see what is written
        if (int e = stretch(r)) return e;
    if (o.loudness || o.normalize)
        if (int e = level(r)) return e;
    if (int e = write_outputs(r)) return e;
    if (!o.psd_path.empty())  // of what was written: after --normalize and --limit
        if (int e = write_psd(o, r.out.ptr.data(), r.C, r.Lr, r.rate, r.dev)) return e;
    if (r.comm) dsp_comm_destroy(r.comm);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const time_t started = std::time(nullptr) - 2;  // (mtime has one-second resolution)
    Env env;
    env.dspb_run_id = std::getenv("DSPB_RUN_ID"), env.torchelastic_run_id = std::getenv("TORCHELASTIC_RUN_ID");
    env.world_size = std::getenv("WORLD_SIZE"), env.rank = std::getenv("RANK"), env.local_rank = std::getenv("LOCAL_RANK");
    const Parsed p = parse_options(argc, argv, env);
    if (p.status) {
        if (p.message) std::fputs(p.message, stderr);
        if (p.usage) std::fputs(usage_text(), stderr);
        return p.status;
    }
    switch (p.opt.mode) {
    case Options::SWEEP: return run_sweep(p.opt);
    case Options::DECONVOLVE: return run_deconvolve(p.opt);
    case Options::TRANSFER: return run_transfer(p.opt);
    case Options::DECAY: return run_decay(p.opt);
    default: return run_render(p.opt, started);
    }
}
