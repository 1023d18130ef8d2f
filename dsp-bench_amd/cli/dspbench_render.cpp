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
#include <hip/hip_runtime.h>

#include <sys/stat.h>
#include <unistd.h>

#include <ctime>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dspbench/dspbench.h"
#include "dspbench/module.h"
#include "dspbench/shard.h"
#include "dspbench/wav.h"

namespace {

int fail(const char *what, int st) {
    std::fprintf(stderr, "dspbench_render: %s: %s (%s)\n", what, dsp_status_string(st), dsp_last_error());
    return 1;
}

#define HIPCK(x)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            std::fprintf(stderr, "dspbench_render: %s: %s\n", #x, hipGetErrorString(e_)); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

bool read_file(const char *path, std::vector<unsigned char> &out) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n : 0);
    const bool ok = n >= 0 && std::fread(out.data(), 1, out.size(), f) == out.size();
    std::fclose(f);
    return ok;
}

void usage() {
    std::fprintf(stderr,
                 "usage: dspbench_render IN.wav OUT.wav [--plugin gain_test|IR_test|no_op|static_gain|PATH.cpp]\n"
                 "       [--convolve IR.wav] [--gain G] [--ir G,STEP] [--block B] [--bits 16|24|32|float] [--stft MAG.f32]"
                 " [--device N]\n"
                 "       [--device-channels C] [--device-rate R] [--rate R] [--loop NBLOCKS]\n"
                 "       [--loudness] [--normalize LUFS [--true-peak-ceiling DBTP [--limit]]]\n"
                 "       [--limit-lookahead MS] [--limit-release MS]\n"
                 "       [--deconvolve REF.wav [--deconv-eps E] [--deconv-pre N] [--ir-length N]]\n"
                 "       [--world W --rank R --comm-id FILE [--run-id STR] [--chunk SAMPLES]]\n"
                 "       dspbench_render --sweep F1:F2:SECONDS[:RATE[:BITS]] OUT.wav\n");
}

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

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// --sweep SPEC OUT.wav (either order): the excitation as a mono WAV, host only
int write_sweep(const char *spec_arg, const char *out_path) {
    dsp_sweep_spec sp{};
    sp.amplitude = 0.5;
    unsigned rate = 48000;
    char bits_s[8] = "float", tail = 0;
    const int got = std::sscanf(spec_arg, "%lf:%lf:%lf:%u:%7[a-z0-9]%c", &sp.f1, &sp.f2, &sp.seconds, &rate, bits_s, &tail);
    const std::string bs = bits_s;
    if (got < 3 || got > 5 || (bs != "float" && bs != "16" && bs != "24" && bs != "32")) {
        usage();
        return 2;
    }
    uint64_t L = 0;
    sp.fade = 0;
    int st = dsp_sweep_plan(rate, &sp, &L, nullptr);
    if (st) return fail("dsp_sweep_plan", st);
    sp.fade = (uint32_t)std::min<uint64_t>(rate / 100, L / 2);  // 10 ms at each end
    std::vector<float> x(L);
    if ((st = dsp_sweep(rate, &sp, x.data(), L))) return fail("dsp_sweep", st);
    const uint16_t fmt = bs == "float" ? DSP_WAV_FORMAT_FLOAT : DSP_WAV_FORMAT_PCM;
    const uint16_t bits = bs == "float" ? 32 : (uint16_t)std::atoi(bits_s);
    const size_t bps = bits / 8u;
    std::vector<unsigned char> out(64 + L * bps);
    const int hdr = dsp_wav_write_header(out.data(), out.size(), fmt, 1, rate, bits, L);
    if (hdr < 0) return fail("dsp_wav_write_header", hdr);
    for (uint64_t i = 0; i < L; ++i) {  // dsp_wav_encode's rounding, on the host
        uint32_t w;
        if (fmt == DSP_WAV_FORMAT_FLOAT) std::memcpy(&w, &x[i], 4);
        else if (bits == 32) {
            const double r = std::min(std::max(std::rint((double)x[i] * 2147483648.0), -2147483648.0), 2147483647.0);
            w = (uint32_t)(int32_t)r;
        } else {
            const float S = bits == 16 ? 32768.f : 8388608.f;
            w = (uint32_t)(int32_t)std::fmin(std::fmax(std::rint(x[i] * S), -S), S - 1.f);
        }
        for (size_t b = 0; b < bps; ++b) out[hdr + i * bps + b] = (unsigned char)(w >> (8 * b));
    }
    FILE *f = std::fopen(out_path, "wb");
    if (!f || std::fwrite(out.data(), 1, hdr + L * bps, f) != hdr + L * bps) {
        std::fprintf(stderr, "dspbench_render: cannot write %s\n", out_path);
        return 1;
    }
    std::fclose(f);
    std::printf("dspbench_render: sweep %g..%g Hz, %llu frames @ %u Hz -> %s (%s)\n", sp.f1, sp.f2,
                (unsigned long long)L, rate, out_path, bits_s);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i)
        if (std::string(argv[i]) == "--sweep") {  // its value and one positional argument, nothing else
            if (argc != 4 || i > 2) {
                usage();
                return 2;
            }
            return write_sweep(argv[i + 1], argv[i == 1 ? 3 : 1]);
        }
    if (argc < 3) {
        usage();
        return 2;
    }
    const char *in_path = argv[1], *out_path = argv[2];
    std::string plugin = "gain_test", stft_path, bits_opt, conv_path, deconv_path;
    double deconv_eps = 1e-6;
    uint64_t deconv_pre = 0, ir_length = 0;
    bool have_plugin = false;
    float gain = -1.f, ir_gain = 0.9f, ir_step = 0.002f;
    uint32_t B = 512;
    int device = -1;
    uint32_t dev_channels = 0, dev_rate = 0, conv_rate = 0, world = 0, rank = 0;
    uint64_t loop_blocks = 0, chunk = 16ull << 20;
    bool have_rank = false;
    bool want_loudness = false, want_normalize = false, want_ceiling = false;
    bool want_limit = false;
    double norm_lufs = 0.0, ceiling_dbtp = 0.0, limit_lookahead_ms = 1.5, limit_release_ms = 100.0;
    std::string comm_path, run_id;
    const time_t started = std::time(nullptr) - 2;  // (mtime has one-second resolution)
    if (const char *e = std::getenv("DSPB_RUN_ID")) run_id = e;
    else if (const char *e2 = std::getenv("TORCHELASTIC_RUN_ID")) run_id = e2;
    for (int i = 3; i < argc; i += 2) {  // every option but --loudness and --limit takes one value
        const std::string a = argv[i];
        if (a == "--loudness" || a == "--limit") {
            (a == "--limit" ? want_limit : want_loudness) = true;
            --i;
            continue;
        }
        const char *v = i + 1 < argc ? argv[i + 1] : nullptr;
        if (!v) {
            usage();
            return 2;
        }
        if (a == "--plugin") plugin = v, have_plugin = true;
        else if (a == "--convolve") conv_path = v;
        else if (a == "--deconvolve") deconv_path = v;
        else if (a == "--deconv-eps") deconv_eps = std::strtod(v, nullptr);
        else if (a == "--deconv-pre") deconv_pre = std::strtoull(v, nullptr, 10);
        else if (a == "--ir-length") {
            ir_length = std::strtoull(v, nullptr, 10);
            if (ir_length == 0) {
                usage();
                return 2;
            }
        }
        else if (a == "--gain") gain = std::strtof(v, nullptr);
        else if (a == "--ir") {
            if (std::sscanf(v, "%f,%f", &ir_gain, &ir_step) != 2) {
                usage();
                return 2;
            }
        } else if (a == "--block") B = (uint32_t)std::strtoul(v, nullptr, 10);
        else if (a == "--bits") bits_opt = v;
        else if (a == "--stft") stft_path = v;
        else if (a == "--device") device = std::atoi(v);
        else if (a == "--device-channels") dev_channels = (uint32_t)std::strtoul(v, nullptr, 10);
        else if (a == "--device-rate") dev_rate = (uint32_t)std::strtoul(v, nullptr, 10);
        else if (a == "--rate") {
            conv_rate = (uint32_t)std::strtoul(v, nullptr, 10);
            if (conv_rate == 0) {
                usage();
                return 2;
            }
        } else if (a == "--normalize" || a == "--true-peak-ceiling" || a == "--limit-lookahead" ||
                   a == "--limit-release") {
            char *end = nullptr;
            const double val = std::strtod(v, &end);
            if (end == v || *end) {  // not a number
                usage();
                return 2;
            }
            if (a == "--normalize") norm_lufs = val, want_normalize = true;
            else if (a == "--true-peak-ceiling") ceiling_dbtp = val, want_ceiling = true;
            else if (a == "--limit-lookahead") limit_lookahead_ms = val;
            else limit_release_ms = val;
        }
        else if (a == "--loop") loop_blocks = std::strtoull(v, nullptr, 10);
        else if (a == "--world") world = (uint32_t)std::strtoul(v, nullptr, 10);
        else if (a == "--rank") rank = (uint32_t)std::strtoul(v, nullptr, 10), have_rank = true;
        else if (a == "--comm-id") comm_path = v;
        else if (a == "--run-id") run_id = v;
        else if (a == "--chunk") chunk = std::strtoull(v, nullptr, 10);
        else {
            usage();
            return 2;
        }
    }
    if (B == 0) {
        usage();
        return 2;
    }
    if (have_plugin && !conv_path.empty()) {
        std::fprintf(stderr, "dspbench_render: --convolve and --plugin exclude each other\n");
        return 2;
    }
    const bool multi = !comm_path.empty();
    if (!deconv_path.empty() && (have_plugin || !conv_path.empty() || loop_blocks || multi || world || conv_rate ||
                                 !stft_path.empty() || want_loudness || want_normalize || want_ceiling || want_limit)) {
        std::fprintf(stderr, "dspbench_render: --deconvolve excludes --plugin, --convolve, --loop, --stft, --rate, "
                             "--loudness, --normalize and the multi-GPU modes\n");
        usage();
        return 2;
    }
    if (deconv_path.empty() && (deconv_pre || ir_length || deconv_eps != 1e-6)) {
        std::fprintf(stderr, "dspbench_render: --deconv-eps, --deconv-pre and --ir-length need --deconvolve\n");
        usage();
        return 2;
    }
    if (conv_rate && (dev_rate || loop_blocks || multi || world)) {
        std::fprintf(stderr, "dspbench_render: --rate excludes --device-rate, --loop and the multi-GPU modes\n");
        usage();
        return 2;
    }
    if ((want_loudness || want_normalize || want_ceiling || want_limit) && (loop_blocks || multi || world)) {
        std::fprintf(stderr, "dspbench_render: --loudness, --normalize, --true-peak-ceiling and --limit exclude --loop "
                             "and the multi-GPU modes\n");
        usage();
        return 2;
    }
    if (want_ceiling && !want_normalize) {
        std::fprintf(stderr, "dspbench_render: --true-peak-ceiling needs --normalize\n");
        usage();
        return 2;
    }
    if (want_limit && !(want_normalize && want_ceiling)) {
        std::fprintf(stderr, "dspbench_render: --limit needs --normalize and --true-peak-ceiling\n");
        usage();
        return 2;
    }
    if (want_limit && !(limit_lookahead_ms >= 0.0 && limit_release_ms >= 0.0)) {
        usage();
        return 2;
    }
    if ((want_normalize && !std::isfinite(norm_lufs)) || (want_ceiling && !std::isfinite(ceiling_dbtp))) {
        usage();
        return 2;
    }
    if (multi) {  // torchrun-style environment when not given explicitly
        const char *ew = std::getenv("WORLD_SIZE"), *er = std::getenv("RANK");
        if (!world) world = ew ? (uint32_t)std::atoi(ew) : 1;
        if (!have_rank) rank = er ? (uint32_t)std::atoi(er) : 0;
        if (device < 0) {
            const char *lr = std::getenv("LOCAL_RANK");
            device = lr ? std::atoi(lr) : (int)rank;
        }
        if (world == 0 || rank >= world || stft_path.empty() || loop_blocks) {
            std::fprintf(stderr, "dspbench_render: --comm-id needs --stft, rank < world and no --loop\n");
            return 2;
        }
    }
    if (device < 0) device = 0;

    // ---- load + parse (wav_reader.h:57-205) --------------------------------
    std::vector<unsigned char> file;
    if (!read_file(in_path, file)) {
        std::fprintf(stderr, "dspbench_render: cannot read %s\n", in_path);
        return 1;
    }
    dsp_wav_info info{};
    int st = dsp_wav_parse(file.data(), file.size(), &info);
    if (st) return fail("dsp_wav_parse", st);
    const uint32_t Cf = info.channels;                // the file's channels
    const uint32_t C = dev_channels ? dev_channels : Cf;  // the device's (the render's)
    const uint32_t Cin = Cf < C ? Cf : C;             // channels_to_write (audio.cpp:66)
    const uint32_t rate = conv_rate ? conv_rate : dev_rate ? dev_rate : info.sample_rate;
    uint64_t L = info.frames;  // (--rate: the converted length from the conversion on)
    if (Cf == 0 || Cf > 16 || C == 0 || C > 16) {
        std::fprintf(stderr, "dspbench_render: %u file / %u device channels (1..16 supported)\n", Cf, C);
        return 1;
    }
    std::vector<unsigned char> payload(info.data_bytes);
    for (uint64_t c = 0, o = 0; c < info.n_data_chunks; ++c) {  // the data chunks, concatenated
        std::memcpy(payload.data() + o, file.data() + info.data_offset[c], info.data_size[c]);
        o += info.data_size[c];
    }
    file.clear();
    file.shrink_to_fit();

    HIPCK(hipSetDevice(device));
    hipStream_t s;
    HIPCK(hipStreamCreate(&s));
    dsp_exec ex{};
    ex.device = device;
    ex.stream = s;

    // ---- payload -> HBM, decode to planar float (audio.h:66-121) ----------
    const auto t0 = std::chrono::steady_clock::now();
    void *d_pay = nullptr;
    HIPCK(hipMalloc(&d_pay, payload.size() + 16));
    HIPCK(hipMemcpyAsync(d_pay, payload.data(), payload.size(), hipMemcpyHostToDevice, s));
    std::vector<float *> din(Cf), dout(C);
    for (uint32_t c = 0; c < Cf; ++c) HIPCK(hipMalloc(&din[c], (L ? L : 1) * sizeof(float)));
    if ((st = dsp_wav_decode(d_pay, &info, 0, L, din.data(), &ex))) return fail("dsp_wav_decode", st);
    if (conv_rate && conv_rate != info.sample_rate) {  // --rate: the file at the new rate replaces the decoded one
        uint64_t Ln = 0;
        if ((st = dsp_resample_plan(info.sample_rate, conv_rate, L, nullptr, nullptr, nullptr, nullptr, &Ln, nullptr)))
            return fail("dsp_resample_plan", st);
        std::vector<float *> dnew(Cf);
        for (uint32_t c = 0; c < Cf; ++c) HIPCK(hipMalloc(&dnew[c], (Ln ? Ln : 1) * sizeof(float)));
        if ((st = dsp_resample(din.data(), Cf, L, dnew.data(), Ln, info.sample_rate, conv_rate, nullptr, &ex)))
            return fail("dsp_resample", st);
        HIPCK(hipStreamSynchronize(s));
        for (uint32_t c = 0; c < Cf; ++c) {
            HIPCK(hipFree(din[c]));
            din[c] = dnew[c];
        }
        L = Ln;
    }
    if (!deconv_path.empty()) {
        // ---- swept-sine measurement: the recording deconvolved by REF's first channel ----
        std::vector<unsigned char> rf;
        if (!read_file(deconv_path.c_str(), rf)) {
            std::fprintf(stderr, "dspbench_render: cannot read %s\n", deconv_path.c_str());
            return 1;
        }
        dsp_wav_info ri{};
        if ((st = dsp_wav_parse(rf.data(), rf.size(), &ri))) return fail("dsp_wav_parse (excitation)", st);
        if (ri.sample_rate != info.sample_rate) {
            std::fprintf(stderr, "dspbench_render: --deconvolve: %s is at %u Hz, %s at %u Hz\n", deconv_path.c_str(),
                         ri.sample_rate, in_path, info.sample_rate);
            return 1;
        }
        if (ri.frames == 0 || L == 0 || ri.channels == 0 || ri.channels > 16) {
            std::fprintf(stderr, "dspbench_render: --deconvolve: an empty recording or excitation\n");
            return 1;
        }
        std::vector<unsigned char> rp(ri.data_bytes);
        for (uint64_t c = 0, o = 0; c < ri.n_data_chunks; ++c) {
            std::memcpy(rp.data() + o, rf.data() + ri.data_offset[c], ri.data_size[c]);
            o += ri.data_size[c];
        }
        void *d_ref = nullptr;
        HIPCK(hipMalloc(&d_ref, rp.size() + 16));
        HIPCK(hipMemcpyAsync(d_ref, rp.data(), rp.size(), hipMemcpyHostToDevice, s));
        std::vector<float *> dref(ri.channels);
        for (uint32_t c = 0; c < ri.channels; ++c) HIPCK(hipMalloc(&dref[c], ri.frames * sizeof(float)));
        if ((st = dsp_wav_decode(d_ref, &ri, 0, ri.frames, dref.data(), &ex))) return fail("dsp_wav_decode", st);
        uint32_t n = 0;
        if ((st = dsp_deconv_plan(L, ri.frames, Cf, &n, nullptr))) return fail("dsp_deconv_plan", st);
        const uint64_t irl = ir_length ? ir_length : std::min<uint64_t>(n, 1u << 20);
        if (irl > n || deconv_pre > irl) {
            std::fprintf(stderr, "dspbench_render: --deconvolve: needs --deconv-pre <= --ir-length <= n = %u\n", n);
            return 2;
        }
        std::vector<float *> dir(Cf);
        for (uint32_t c = 0; c < Cf; ++c) HIPCK(hipMalloc(&dir[c], irl * sizeof(float)));
        dsp_deconv_spec ds{};
        ds.eps = deconv_eps;
        ds.pre = (uint32_t)deconv_pre;
        if ((st = dsp_deconvolve(din.data(), Cf, L, dref[0], ri.frames, dir.data(), irl, &ds, &ex)))
            return fail("dsp_deconvolve", st);
        uint16_t fmt = DSP_WAV_FORMAT_FLOAT, bits = 32;
        if (!bits_opt.empty() && bits_opt != "float") fmt = DSP_WAV_FORMAT_PCM, bits = (uint16_t)std::atoi(bits_opt.c_str());
        const uint64_t out_bytes = irl * Cf * (bits / 8u);
        void *d_opay = nullptr;
        HIPCK(hipMalloc(&d_opay, out_bytes + 16));
        if ((st = dsp_wav_encode(dir.data(), Cf, irl, fmt, bits, d_opay, &ex))) return fail("dsp_wav_encode", st);
        std::vector<unsigned char> out(64 + out_bytes);
        const int hdr = dsp_wav_write_header(out.data(), out.size(), fmt, (uint16_t)Cf, info.sample_rate, bits, irl);
        if (hdr < 0) return fail("dsp_wav_write_header", hdr);
        HIPCK(hipMemcpyAsync(out.data() + hdr, d_opay, out_bytes, hipMemcpyDeviceToHost, s));
        std::vector<float> h(irl);
        std::string j = "{\"n\": " + std::to_string(n) + ", \"eps\": " + json_num(deconv_eps) + ", \"pre\": " +
                        std::to_string(deconv_pre) + ", \"ir_length\": " + std::to_string(irl) + ", \"peaks\": [";
        for (uint32_t c = 0; c < Cf; ++c) {  // each channel's peak
            HIPCK(hipMemcpyAsync(h.data(), dir[c], irl * sizeof(float), hipMemcpyDeviceToHost, s));
            HIPCK(hipStreamSynchronize(s));
            uint64_t at = 0;
            for (uint64_t i = 1; i < irl; ++i)
                if (std::fabs(h[i]) > std::fabs(h[at])) at = i;
            j += std::string(c ? ", " : "") + "{\"index\": " + std::to_string(at) + ", \"value\": " +
                 json_num((double)h[at]) + "}";
        }
        std::printf("%s]}\n", j.c_str());
        FILE *f = std::fopen(out_path, "wb");
        if (!f || std::fwrite(out.data(), 1, hdr + out_bytes, f) != hdr + out_bytes) {
            std::fprintf(stderr, "dspbench_render: cannot write %s\n", out_path);
            return 1;
        }
        std::fclose(f);
        std::printf("dspbench_render: %s deconvolved by %s: %u ch x %llu frames @ %u Hz -> %s (n = %u), %.1f ms end to end\n",
                    in_path, deconv_path.c_str(), Cf, (unsigned long long)irl, info.sample_rate, out_path, n, ms_since(t0));
        for (float *q : dir) (void)hipFree(q);
        for (float *q : dref) (void)hipFree(q);
        for (float *q : din) (void)hipFree(q);
        (void)hipFree(d_ref);
        (void)hipFree(d_opay);
        (void)hipFree(d_pay);
        (void)hipStreamDestroy(s);
        return 0;
    }
    const uint64_t nblocks = loop_blocks ? loop_blocks : (L + B - 1) / B, Lr = nblocks * B;
    for (uint32_t c = 0; c < C; ++c) HIPCK(hipMalloc(&dout[c], Lr * sizeof(float)));

    // ---- plugin ------------------------------------------------------------
    dsp_plugin p{};
    float pv[2] = {0.f, 0.f};
    dsp_module *mod = nullptr;
    std::vector<unsigned char> gparams;
    std::vector<float> taps;
    if (!conv_path.empty()) {  // the IR file's first channel, through the same parse + GPU decode
        std::vector<unsigned char> irf;
        if (!read_file(conv_path.c_str(), irf)) {
            std::fprintf(stderr, "dspbench_render: cannot read %s\n", conv_path.c_str());
            return 1;
        }
        dsp_wav_info ii{};
        if ((st = dsp_wav_parse(irf.data(), irf.size(), &ii))) return fail("dsp_wav_parse (impulse response)", st);
        if (ii.frames == 0 || ii.frames > (1u << 20) || ii.channels == 0 || ii.channels > 16) {
            std::fprintf(stderr, "dspbench_render: %s: %llu frames, %u channels (1..2^20 frames, 1..16 channels)\n",
                         conv_path.c_str(), (unsigned long long)ii.frames, ii.channels);
            return 1;
        }
        std::vector<unsigned char> irp(ii.data_bytes);
        for (uint64_t c = 0, o = 0; c < ii.n_data_chunks; ++c) {
            std::memcpy(irp.data() + o, irf.data() + ii.data_offset[c], ii.data_size[c]);
            o += ii.data_size[c];
        }
        void *d_ir = nullptr;
        HIPCK(hipMalloc(&d_ir, irp.size() + 16));
        HIPCK(hipMemcpyAsync(d_ir, irp.data(), irp.size(), hipMemcpyHostToDevice, s));
        std::vector<float *> dir(ii.channels);
        for (uint32_t c = 0; c < ii.channels; ++c) HIPCK(hipMalloc(&dir[c], ii.frames * sizeof(float)));
        if ((st = dsp_wav_decode(d_ir, &ii, 0, ii.frames, dir.data(), &ex))) return fail("dsp_wav_decode", st);
        uint64_t ntaps = ii.frames;
        float tap_scale = 1.f;
        if (conv_rate && conv_rate != ii.sample_rate) {  // --rate: the response at the render's rate, DC gain kept
            if ((st = dsp_resample_plan(ii.sample_rate, conv_rate, ii.frames, nullptr, nullptr, nullptr, nullptr, &ntaps,
                                        nullptr)))
                return fail("dsp_resample_plan (impulse response)", st);
            if (ntaps == 0 || ntaps > (1u << 20)) {
                std::fprintf(stderr, "dspbench_render: %s: %llu taps at %u Hz (1..2^20 supported)\n", conv_path.c_str(),
                             (unsigned long long)ntaps, conv_rate);
                return 1;
            }
            float *dres = nullptr;
            HIPCK(hipMalloc(&dres, ntaps * sizeof(float)));
            if ((st = dsp_resample(dir.data(), 1, ii.frames, &dres, ntaps, ii.sample_rate, conv_rate, nullptr, &ex)))
                return fail("dsp_resample (impulse response)", st);
            HIPCK(hipStreamSynchronize(s));
            HIPCK(hipFree(dir[0]));
            dir[0] = dres;
            tap_scale = (float)((double)ii.sample_rate / (double)conv_rate);
        }
        taps.resize(ntaps);
        HIPCK(hipMemcpyAsync(taps.data(), dir[0], ntaps * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
        if (tap_scale != 1.f)
            for (float &t : taps) t *= tap_scale;
        for (float *q : dir) HIPCK(hipFree(q));
        HIPCK(hipFree(d_ir));
        p.kind = DSP_PLUGIN_CONV, p.params = taps.data(), p.params_size = (uint32_t)(taps.size() * sizeof(float));
    } else if (plugin == "gain_test") {
        pv[0] = gain >= 0.f ? gain : 0.2f;  // build/gain_test.cpp:23
        p.kind = DSP_PLUGIN_GAIN, p.params = pv, p.params_size = 4;
    } else if (plugin == "static_gain") {
        pv[0] = gain >= 0.f ? gain : 0.1f;  // test/static_gain_plugin.cpp:22
        p.kind = DSP_PLUGIN_STATIC_GAIN, p.state = pv, p.state_size = 4;
    } else if (plugin == "IR_test") {
        pv[0] = ir_gain, pv[1] = ir_step;  // build/IR_test.cpp:24
        p.kind = DSP_PLUGIN_IR_RAMP, p.params = pv, p.params_size = 8;
    } else if (plugin == "no_op") {
        p.kind = DSP_PLUGIN_NOOP;
    } else {  // a plugin source file: compile for gfx950, load, defaults, state
        std::vector<unsigned char> src;
        if (!read_file(plugin.c_str(), src)) {
            std::fprintf(stderr, "dspbench_render: cannot read plugin %s\n", plugin.c_str());
            return 1;
        }
        src.push_back(0);
        void *code = nullptr;
        uint64_t code_size = 0;
        std::vector<char> log(1 << 16);
        if ((st = dsp_module_compile((const char *)src.data(), plugin.c_str(), &code, &code_size, log.data(),
                                     log.size()))) {
            std::fprintf(stderr, "%s\n", log.data());
            return fail("dsp_module_compile", st);
        }
        st = dsp_module_load(code, code_size, device, &mod);
        dsp_module_free_code(code);
        if (st) return fail("dsp_module_load", st);
        uint32_t ps = 0, ss = 0;
        int stateless = 0;
        if ((st = dsp_module_sizes(mod, &ps, &ss, &stateless))) return fail("dsp_module_sizes", st);
        gparams.resize(ps ? ps : 1);
        if ((st = dsp_module_default_parameters(mod, gparams.data()))) return fail("dsp_module_default_parameters", st);
        if ((st = dsp_module_initialize_state(mod, gparams.data(), C, (float)rate, 16u << 20)))
            return fail("dsp_module_initialize_state", st);
        p.kind = DSP_PLUGIN_GENERIC, p.params = gparams.data(), p.params_size = ps, p.module = mod;
    }

    // ---- render (+ STFT) ---------------------------------------------------
    const float sr = (float)rate;
    const uint32_t N = 8192, H = 4096, K = N / 2 + 1;
    const uint64_t F = stft_path.empty() ? 0 : dsp_stft_frame_count(Lr, N, H);
    std::vector<float *> dmag(C, nullptr);
    hipEvent_t e0, e1;
    HIPCK(hipEventCreate(&e0));
    HIPCK(hipEventCreate(&e1));
    dsp_comm *comm = nullptr;
    if (multi) {
        unsigned char id[DSP_COMM_ID_BYTES];
        if (!exchange_comm_id(comm_path, rank, run_id, started, id)) {
            std::fprintf(stderr, "dspbench_render: rank %u: no communicator id at %s\n", rank, comm_path.c_str());
            return 1;
        }
        if ((st = dsp_comm_init(id, world, rank, device, &comm))) return fail("dsp_comm_init", st);
        // every rank has joined (the init is collective): the id is spent
        if (rank == 0) (void)std::remove(comm_path.c_str());
    }
    HIPCK(hipEventRecord(e0, s));
    if (multi) {
        // cfg 5: this rank renders + STFTs its run of channels, rank 0
        // gathers every channel (dout / dmag hold the whole file there)
        dsp_shard sh{};
        if ((st = dsp_shard_plan(L, C, world, rank, B, N, H, DSP_SHARD_CHANNELS, 1, &sh)))
            return fail("dsp_shard_plan", st);
        std::vector<float *> lout(sh.channels), lmag(sh.channels);
        std::vector<const float *> lin;
        for (uint32_t j = 0; j < sh.channels; ++j) {
            const uint32_t c = sh.chan0 + j;
            if (c < Cin) lin.push_back(din[c]);
            if (rank == 0) {
                lout[j] = dout[c];
            } else {
                HIPCK(hipMalloc(&lout[j], Lr * sizeof(float)));
            }
            HIPCK(hipMalloc(&lmag[j], (F ? F : 1) * K * sizeof(float)));
        }
        if (rank == 0)
            for (uint32_t c = 0; c < C; ++c) HIPCK(hipMalloc(&dmag[c], (F ? F : 1) * K * sizeof(float)));
        st = dsp_render_stft_sharded(lin.data(), (uint32_t)lin.size(), L, lout.data(), lmag.data(), K, C, B, sr, &p,
                                     N, H, DSP_WIN_HANN, K, &sh, chunk, comm, 0, rank == 0 ? dout.data() : nullptr,
                                     rank == 0 ? dmag.data() : nullptr, &ex);
        if (st) return fail("dsp_render_stft_sharded", st);
        HIPCK(hipStreamSynchronize(s));
        for (uint32_t j = 0; j < sh.channels; ++j) {
            if (rank != 0) (void)hipFree(lout[j]);
            (void)hipFree(lmag[j]);
        }
    } else if (loop_blocks) {
        uint64_t cursor = 0;
        if ((st = dsp_render_loop(din.data(), Cin, L, 0, dout.data(), C, B, nblocks, sr, &p, &cursor, &ex)))
            return fail("dsp_render_loop", st);
    } else if (!stft_path.empty() && F > 0) {
        for (uint32_t c = 0; c < C; ++c) HIPCK(hipMalloc(&dmag[c], F * K * sizeof(float)));
        st = dsp_render_stft(din.data(), Cin, L, dout.data(), C, B, sr, &p, N, H, DSP_WIN_HANN, K, dmag.data(), K,
                             &ex);
        if (st) return fail("dsp_render_stft", st);
    } else {
        if ((st = dsp_render_offline(din.data(), Cin, L, dout.data(), C, B, sr, &p, &ex)))
            return fail("dsp_render_offline", st);
    }
    HIPCK(hipEventRecord(e1, s));
    if (multi && rank != 0) {  // only the root writes
        HIPCK(hipStreamSynchronize(s));
        float ms = 0.f;
        HIPCK(hipEventElapsedTime(&ms, e0, e1));
        std::printf("dspbench_render: rank %u of %u: channels rendered and gathered to rank 0 in %.3f ms\n", rank,
                    world, ms);
        dsp_comm_destroy(comm);
        return 0;
    }

    // ---- loudness of the render, and the gain to a target level ------------
    if (want_loudness || want_normalize) {
        dsp_loudness_result lr{};
        if ((st = dsp_loudness(dout.data(), C, Lr, rate, nullptr, DSP_LOUDNESS_TRUE_PEAK, nullptr, nullptr, nullptr, &lr,
                               &ex)))
            return fail("dsp_loudness", st);
        float g = 1.f, residual = 1.f;
        dsp_limiter_result lim{};
        if (want_normalize) {
            if (!std::isfinite(lr.integrated)) {
                std::fprintf(stderr, "dspbench_render: --normalize: the render's integrated loudness is %s "
                                     "(no block passes the gates)\n", json_num(lr.integrated).c_str());
                return 1;
            }
            g = (float)std::pow(10.0, (norm_lufs - lr.integrated) / 20.0);
            // the largest gain <= g0 that keeps `peak` at or below the ceiling
            auto fit = [&](double peak, float g0) {
                const double limit = std::pow(10.0, ceiling_dbtp / 20.0);
                if (peak * (double)g0 > limit) {
                    g0 = (float)(limit / peak);
                    while (g0 > 0.f && peak * (double)g0 > limit) g0 = std::nextafterf(g0, 0.f);
                }
                return g0;
            };
            auto scale = [&](float by) {
                for (uint32_t c = 0; c < C; ++c)
                    if (int e = dsp_gain(dout[c], dout[c], by, Lr, &ex)) return e;
                return 0;
            };
            if (want_ceiling && !want_limit) g = fit(lr.true_peak, g);
            if ((st = scale(g))) return fail("dsp_gain", st);
            if (want_limit) {
                // the level stays: the limiter turns down the peaks, then a scalar gain takes what is
                // left of the true peak above the ceiling (the limiter's gain moves between samples)
                dsp_limiter_spec ls{};
                ls.ceiling = (float)std::pow(10.0, ceiling_dbtp / 20.0);
                const double la = std::floor(limit_lookahead_ms * 1e-3 * (double)rate + 0.5);
                ls.lookahead = (uint32_t)(la < 1024.0 ? la : 1024.0);
                ls.release = limit_release_ms * 1e-3 * (double)rate;
                if (ls.release > 0.0 && ls.release < 1.0) ls.release = 1.0;
                ls.flags = DSP_LIMITER_TRUE_PEAK;
                if ((st = dsp_limiter(dout.data(), C, Lr, dout.data(), rate, &ls, nullptr, nullptr, nullptr, &lim, &ex)))
                    return fail("dsp_limiter", st);
                dsp_loudness_result after{};
                if ((st = dsp_loudness(dout.data(), C, Lr, rate, nullptr, DSP_LOUDNESS_TRUE_PEAK, nullptr, nullptr,
                                       nullptr, &after, &ex)))
                    return fail("dsp_loudness", st);
                residual = fit(after.true_peak, 1.f);
                if (residual != 1.f && (st = scale(residual))) return fail("dsp_gain", st);
            }
        }
        if (want_loudness || want_limit) {
            std::string j = "{\"integrated\": " + json_num(lr.integrated) + ", \"range\": " + json_num(lr.range) +
                            ", \"momentary_max\": " + json_num(lr.momentary_max) + ", \"short_term_max\": " +
                            json_num(lr.short_term_max) + ", \"sample_peak\": " + json_num(lr.sample_peak) +
                            ", \"true_peak\": " + json_num(lr.true_peak) + ", \"blocks\": " +
                            std::to_string(lr.blocks) + ", \"gated_blocks\": " + std::to_string(lr.gated_blocks);
            if (want_normalize) j += ", \"gain\": " + json_num((double)g);
            if (want_limit)
                j += ", \"limiter\": {\"min_gain\": " + json_num(lim.min_gain) + ", \"limited\": " +
                     std::to_string(lim.limited) + ", \"residual_gain\": " + json_num((double)residual) + "}";
            std::printf("%s}\n", j.c_str());
        }
    }

    // ---- encode the render (audio.h:123-133 interleave) and write ----------
    uint16_t fmt = info.format, bits = info.bits_per_sample;
    if (bits_opt == "float") fmt = DSP_WAV_FORMAT_FLOAT, bits = 32;
    else if (!bits_opt.empty()) fmt = DSP_WAV_FORMAT_PCM, bits = (uint16_t)std::atoi(bits_opt.c_str());
    const uint64_t out_bytes = Lr * C * (bits / 8u);
    void *d_opay = nullptr;
    HIPCK(hipMalloc(&d_opay, out_bytes + 16));
    if ((st = dsp_wav_encode(dout.data(), C, Lr, fmt, bits, d_opay, &ex))) return fail("dsp_wav_encode", st);
    std::vector<unsigned char> out(64 + out_bytes);
    const int hdr = dsp_wav_write_header(out.data(), out.size(), fmt, (uint16_t)C, rate, bits, Lr);
    if (hdr < 0) return fail("dsp_wav_write_header", hdr);
    HIPCK(hipMemcpyAsync(out.data() + hdr, d_opay, out_bytes, hipMemcpyDeviceToHost, s));
    std::vector<float> mag;
    if (F > 0) {
        mag.resize((size_t)C * F * K);
        for (uint32_t c = 0; c < C; ++c)
            HIPCK(hipMemcpyAsync(mag.data() + (size_t)c * F * K, dmag[c], F * K * sizeof(float),
                                 hipMemcpyDeviceToHost, s));
    }
    HIPCK(hipStreamSynchronize(s));
    float render_ms = 0.f;
    HIPCK(hipEventElapsedTime(&render_ms, e0, e1));
    FILE *f = std::fopen(out_path, "wb");
    if (!f || std::fwrite(out.data(), 1, hdr + out_bytes, f) != hdr + out_bytes) {
        std::fprintf(stderr, "dspbench_render: cannot write %s\n", out_path);
        return 1;
    }
    std::fclose(f);
    if (F > 0) {
        f = std::fopen(stft_path.c_str(), "wb");
        const uint32_t hk[2] = {C, K};
        if (!f || std::fwrite("DSPMAG1", 1, 8, f) != 8 || std::fwrite(hk, 4, 2, f) != 2 ||
            std::fwrite(&F, 8, 1, f) != 1 || std::fwrite(mag.data(), 4, mag.size(), f) != mag.size()) {
            std::fprintf(stderr, "dspbench_render: cannot write %s\n", stft_path.c_str());
            return 1;
        }
        std::fclose(f);
    }
    std::printf("dspbench_render: %s: %u ch x %llu frames @ %u Hz -> %s (%s %u-bit, %llu blocks of %u)%s; "
                "render %.3f ms on the GPU, %.1f ms end to end\n",
                in_path, C, (unsigned long long)L, rate, out_path,
                fmt == DSP_WAV_FORMAT_FLOAT ? "float" : "PCM", bits, (unsigned long long)nblocks, B,
                F ? (" + STFT " + std::to_string(F) + " frames x " + std::to_string(K) + " bins").c_str() : "",
                render_ms, ms_since(t0));

    if (mod) dsp_module_destroy(mod);
    if (comm) dsp_comm_destroy(comm);
    for (uint32_t c = 0; c < Cf; ++c) (void)hipFree(din[c]);
    for (uint32_t c = 0; c < C; ++c) {
        (void)hipFree(dout[c]);
        if (dmag[c]) (void)hipFree(dmag[c]);
    }
    (void)hipFree(d_pay);
    (void)hipFree(d_opay);
    (void)hipStreamDestroy(s);
    return 0;
}
