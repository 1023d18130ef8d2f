// The option table, the rules between options and the --sweep form of
// dspbench_render (the options themselves are described in dspbench_render.cpp).
#include "options.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iterator>

namespace {

// ---- how a value is read, and where it lands (false: usage) ----------------
// The integer and plain floating readers are lenient on purpose: what strtoul
// makes of the text is the value ("x" is 0).
template <auto M> bool flag(Options &o, const char *) { return o.*M = true; }
template <auto M> bool text(Options &o, const char *v) { return o.*M = v, true; }
template <auto M> bool u32(Options &o, const char *v) { return o.*M = (uint32_t)std::strtoul(v, nullptr, 10), true; }
template <auto M> bool u32_nonzero(Options &o, const char *v) { return u32<M>(o, v) && o.*M != 0; }
template <auto M> bool u64(Options &o, const char *v) { return o.*M = std::strtoull(v, nullptr, 10), true; }
template <auto M> bool u64_nonzero(Options &o, const char *v) { return u64<M>(o, v) && o.*M != 0; }
template <auto M> bool f32(Options &o, const char *v) { return o.*M = std::strtof(v, nullptr), true; }
template <auto M> bool f64(Options &o, const char *v) { return o.*M = std::strtod(v, nullptr), true; }
template <auto M> bool number(Options &o, const char *v) {  // the whole text must be a number
    char *end = nullptr;
    o.*M = std::strtod(v, &end);
    return end != v && !*end;
}
template <auto M, auto Given> bool given(Options &o, const char *v) { return o.*Given = true, M(o, v); }
bool ir_pair(Options &o, const char *v) { return std::sscanf(v, "%f,%f", &o.ir_gain, &o.ir_step) == 2; }
bool device(Options &o, const char *v) { return o.device = std::atoi(v), true; }

using O = Options;
const struct {
    const char *name;
    bool takes_value;
    bool (*read)(Options &, const char *);
} kOptions[] = {
    {"--loudness", false, flag<&O::loudness>},
    {"--limit", false, flag<&O::limit>},
    {"--plugin", true, given<text<&O::plugin>, &O::have_plugin>},
    {"--convolve", true, text<&O::conv_path>},
    {"--deconvolve", true, text<&O::deconv_path>},
    {"--deconv-eps", true, f64<&O::deconv_eps>},
    {"--deconv-pre", true, u64<&O::deconv_pre>},
    {"--ir-length", true, u64_nonzero<&O::ir_length>},
    {"--psd", true, text<&O::psd_path>},
    {"--transfer", true, text<&O::transfer_path>},
    {"--decay", true, text<&O::decay_path>},
    {"--decay-bands", true, given<text<&O::decay_bands>, &O::have_decay_bands>},
    {"--gain", true, f32<&O::gain>},
    {"--ir", true, ir_pair},
    {"--block", true, u32<&O::block>},
    {"--bits", true, text<&O::bits>},
    {"--stft", true, text<&O::stft_path>},
    {"--device", true, device},
    {"--device-channels", true, u32<&O::dev_channels>},
    {"--device-rate", true, u32<&O::dev_rate>},
    {"--rate", true, u32_nonzero<&O::rate>},
    {"--normalize", true, given<number<&O::norm_lufs>, &O::normalize>},
    {"--true-peak-ceiling", true, given<number<&O::ceiling_dbtp>, &O::ceiling>},
    {"--limit-lookahead", true, number<&O::limit_lookahead_ms>},
    {"--limit-release", true, number<&O::limit_release_ms>},
    {"--stretch", true, given<number<&O::stretch_rate>, &O::stretch>},
    {"--pitch", true, given<number<&O::pitch_semitones>, &O::pitch>},
    {"--stretch-hop", true, given<u32<&O::stretch_hop>, &O::have_stretch_hop>},
    {"--loop", true, u64<&O::loop_blocks>},
    {"--world", true, u32<&O::world>},
    {"--rank", true, given<u32<&O::rank>, &O::have_rank>},
    {"--comm-id", true, text<&O::comm_path>},
    {"--run-id", true, text<&O::run_id>},
    {"--chunk", true, u64<&O::chunk>},
};

// ---- what must hold between the options, in the order it is reported -------
const struct {
    bool (*broken)(const Options &);
    const char *message;  // null: the usage text alone
    bool usage;
} kRules[] = {
    {[](const O &o) { return o.block == 0; }, nullptr, true},
    {[](const O &o) { return o.have_plugin && !o.conv_path.empty(); },
     "dspbench_render: --convolve and --plugin exclude each other\n", false},
    {[](const O &o) { return o.stretches() && (!o.deconv_path.empty() || !o.transfer_path.empty()); },
     "dspbench_render: --stretch and --pitch exclude --deconvolve and --transfer (they change a render, and those "
     "modes measure a recording)\n", true},
    {[](const O &o) {
         return o.stretches() && (!o.decay_path.empty() || o.decay_alone || !o.stft_path.empty() || o.loop_blocks || o.multi_gpu());
     },
     "dspbench_render: --stretch and --pitch exclude --decay, --stft, --loop and the multi-GPU modes\n", true},
    {[](const O &o) { return o.stretch && o.pitch; },
     "dspbench_render: --stretch and --pitch exclude each other\n", true},
    {[](const O &o) { return o.stretch && !(o.stretch_rate >= 0.125 && o.stretch_rate <= 8.0); },
     "dspbench_render: --stretch RATE must lie in 0.125 .. 8\n", true},
    {[](const O &o) { return o.pitch && !(o.pitch_semitones >= -24.0 && o.pitch_semitones <= 24.0); },
     "dspbench_render: --pitch SEMITONES must lie in -24 .. 24\n", true},
    {[](const O &o) { return o.have_stretch_hop && !o.stretches(); },
     "dspbench_render: --stretch-hop needs --stretch or --pitch\n", true},
    {[](const O &o) { return o.have_stretch_hop && (o.stretch_hop < 512 || o.stretch_hop > 8192); },
     "dspbench_render: --stretch-hop H must lie in 512 .. 8192\n", true},
    {[](const O &o) {
         return !o.deconv_path.empty() && (o.have_plugin || !o.conv_path.empty() || o.loop_blocks || o.multi_gpu() ||
                                           o.rate || !o.stft_path.empty() || o.levels());
     },
     "dspbench_render: --deconvolve excludes --plugin, --convolve, --loop, --stft, --rate, "
     "--loudness, --normalize and the multi-GPU modes\n", true},
    {[](const O &o) { return o.deconv_path.empty() && o.deconv_options(); },
     "dspbench_render: --deconv-eps, --deconv-pre and --ir-length need --deconvolve\n", true},
    {[](const O &o) {
         return !o.transfer_path.empty() &&
                (o.have_plugin || !o.conv_path.empty() || !o.deconv_path.empty() || o.loop_blocks || o.multi_gpu() ||
                 o.rate || !o.stft_path.empty() || !o.psd_path.empty() || o.levels() || !o.bits.empty());
     },
     "dspbench_render: --transfer excludes --plugin, --convolve, --deconvolve, --loop, --stft, --psd, --rate, --bits, "
     "--loudness, --normalize and the multi-GPU modes\n", true},
    {[](const O &o) { return !o.psd_path.empty() && (!o.deconv_path.empty() || o.loop_blocks || o.multi_gpu()); },
     "dspbench_render: --psd excludes --deconvolve, --loop and the multi-GPU modes\n", true},
    {[](const O &o) { return o.have_decay_bands && o.decay_bands != "octave" && o.decay_bands != "third"; }, nullptr, true},
    {[](const O &o) { return o.have_decay_bands && o.decay_path.empty(); },
     "dspbench_render: --decay-bands needs --decay\n", true},
    {[](const O &o) {
         return !o.decay_path.empty() &&
                (o.have_plugin || !o.conv_path.empty() || o.loop_blocks || o.multi_gpu() || o.rate ||
                 !o.stft_path.empty() || !o.psd_path.empty() || !o.transfer_path.empty());
     },
     "dspbench_render: --decay excludes --plugin, --convolve, --loop, --stft, --psd, --transfer, --rate and the "
     "multi-GPU modes\n", true},
    {[](const O &o) { return !o.decay_path.empty() && !o.decay_alone && o.deconv_path.empty(); },
     "dspbench_render: --decay goes with --deconvolve, or stands alone: IR.wav --decay OUT.csv\n", true},
    {[](const O &o) {
         return o.decay_alone && (o.decay_path.empty() || !o.deconv_path.empty() || o.levels() || !o.bits.empty() ||
                                  o.dev_channels || o.dev_rate);
     },
     "dspbench_render: IR.wav --decay OUT.csv takes only --decay-bands and --device\n", true},
    {[](const O &o) { return o.rate && (o.dev_rate || o.loop_blocks || o.multi_gpu()); },
     "dspbench_render: --rate excludes --device-rate, --loop and the multi-GPU modes\n", true},
    {[](const O &o) { return o.levels() && (o.loop_blocks || o.multi_gpu()); },
     "dspbench_render: --loudness, --normalize, --true-peak-ceiling and --limit exclude --loop "
     "and the multi-GPU modes\n", true},
    {[](const O &o) { return o.ceiling && !o.normalize; },
     "dspbench_render: --true-peak-ceiling needs --normalize\n", true},
    {[](const O &o) { return o.limit && !(o.normalize && o.ceiling); },
     "dspbench_render: --limit needs --normalize and --true-peak-ceiling\n", true},
    {[](const O &o) { return o.limit && !(o.limit_lookahead_ms >= 0.0 && o.limit_release_ms >= 0.0); }, nullptr, true},
    {[](const O &o) {
         return (o.normalize && !std::isfinite(o.norm_lufs)) || (o.ceiling && !std::isfinite(o.ceiling_dbtp));
     },
     nullptr, true},
    {[](const O &o) {
         return o.multi() && (o.world == 0 || o.rank >= o.world || o.stft_path.empty() || o.loop_blocks);
     },
     "dspbench_render: --comm-id needs --stft, rank < world and no --loop\n", false},
};

Parsed usage_error(const char *message = nullptr, bool usage = true) {
    Parsed p;
    p.status = 2, p.message = message, p.usage = usage;
    return p;
}

// --sweep SPEC OUT.wav: F1:F2:SECONDS[:RATE[:BITS]]
Parsed parse_sweep(const char *spec, const char *out_path) {
    Parsed p;
    Options &o = p.opt;
    o.mode = Options::SWEEP, o.out_path = out_path;
    char bits[8] = "float", tail = 0;
    const int got = std::sscanf(spec, "%lf:%lf:%lf:%u:%7[a-z0-9]%c", &o.sweep_f1, &o.sweep_f2, &o.sweep_seconds,
                                &o.sweep_rate, bits, &tail);
    o.sweep_bits = bits;
    const std::string &b = o.sweep_bits;
    if (got < 3 || got > 5 || (b != "float" && b != "16" && b != "24" && b != "32")) return usage_error();
    return p;
}

}  // namespace

const char *usage_text() {
    return "usage: dspbench_render IN.wav OUT.wav [--plugin gain_test|IR_test|no_op|static_gain|PATH.cpp]\n"
           "       [--convolve IR.wav] [--gain G] [--ir G,STEP] [--block B] [--bits 16|24|32|float] [--stft MAG.f32]"
           " [--device N]\n"
           "       [--device-channels C] [--device-rate R] [--rate R] [--loop NBLOCKS]\n"
           "       [--loudness] [--normalize LUFS [--true-peak-ceiling DBTP [--limit]]]\n"
           "       [--limit-lookahead MS] [--limit-release MS]\n"
           "       [--deconvolve REF.wav [--deconv-eps E] [--deconv-pre N] [--ir-length N]]\n"
           "       [--stretch RATE | --pitch SEMITONES [--stretch-hop H]]\n"
           "       [--psd OUT.csv] [--decay OUT.csv [--decay-bands octave|third]]\n"
           "       [--world W --rank R --comm-id FILE [--run-id STR] [--chunk SAMPLES]]\n"
           "       dspbench_render REC.wav OUT.csv --transfer REF.wav [--device N]\n"
           "       dspbench_render IR.wav --decay OUT.csv [--decay-bands octave|third] [--device N]\n"
           "       dspbench_render --sweep F1:F2:SECONDS[:RATE[:BITS]] OUT.wav\n";
}

Parsed parse_options(int argc, const char *const *argv, const Env &env) {
    for (int i = 1; i < argc; ++i)
        if (std::string(argv[i]) == "--sweep") {  // its value and one positional argument, nothing else
            if (argc != 4 || i > 2) return usage_error();
            return parse_sweep(argv[i + 1], argv[i == 1 ? 3 : 1]);
        }
    if (argc < 3) return usage_error();
    Parsed p;
    Options &o = p.opt;
    o.in_path = argv[1];
    o.decay_alone = std::string(argv[2]) == "--decay";  // IR.wav --decay OUT.csv: one positional argument
    if (!o.decay_alone) o.out_path = argv[2];
    if (env.dspb_run_id) o.run_id = env.dspb_run_id;
    else if (env.torchelastic_run_id) o.run_id = env.torchelastic_run_id;
    for (int i = o.decay_alone ? 2 : 3; i < argc; ++i) {
        const auto *opt = std::begin(kOptions);
        while (opt != std::end(kOptions) && argv[i] != std::string(opt->name)) ++opt;
        // (a name that is not an option and one whose value is missing are both the usage text)
        if (opt == std::end(kOptions) || (opt->takes_value && ++i == argc) || !opt->read(o, argv[i])) return usage_error();
    }
    if (!o.deconv_path.empty()) o.mode = Options::DECONVOLVE;
    else if (!o.transfer_path.empty()) o.mode = Options::TRANSFER;
    else if (o.decay_alone) o.mode = Options::DECAY;
    if (o.multi()) {  // torchrun-style environment when not given explicitly
        if (!o.world) o.world = env.world_size ? (uint32_t)std::atoi(env.world_size) : 1;
        if (!o.have_rank) o.rank = env.rank ? (uint32_t)std::atoi(env.rank) : 0;
        if (o.device < 0) o.device = env.local_rank ? std::atoi(env.local_rank) : (int)o.rank;
    }
    if (o.device < 0) o.device = 0;
    for (const auto &r : kRules)
        if (r.broken(o)) return usage_error(r.message, r.usage);
    return p;
}
