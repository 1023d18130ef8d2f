// dspbench_render's command line as data: argv and the launcher's environment
// in, one Options or one argument error out.  No HIP and no dspbench header:
// tests/sanitize/cli_options_check.cpp links options.cpp alone.
#pragma once

#include <cstdint>
#include <string>

struct Options {
    enum Mode { RENDER, DECONVOLVE, SWEEP, TRANSFER, DECAY } mode = RENDER;
    std::string in_path, out_path;
    std::string plugin = "gain_test", conv_path, deconv_path, stft_path, bits, comm_path, run_id;
    std::string psd_path, transfer_path;  // --psd OUT.csv (of the render); REC.wav OUT.csv --transfer REF.wav
    // --decay OUT.csv [--decay-bands octave|third]: of --deconvolve's impulse response, or IR.wav --decay OUT.csv
    std::string decay_path, decay_bands = "octave";
    bool have_decay_bands = false, decay_alone = false;
    bool have_plugin = false, have_rank = false;
    bool loudness = false, normalize = false, ceiling = false, limit = false;
    // --stretch RATE | --pitch SEMITONES [--stretch-hop H]: of the render, before the levels and the encode
    bool stretch = false, pitch = false, have_stretch_hop = false;
    double stretch_rate = 1.0, pitch_semitones = 0.0;
    uint32_t stretch_hop = 2048;
    float gain = -1.f, ir_gain = 0.9f, ir_step = 0.002f;
    double deconv_eps = 1e-6, norm_lufs = 0.0, ceiling_dbtp = 0.0, limit_lookahead_ms = 1.5, limit_release_ms = 100.0;
    uint64_t deconv_pre = 0, ir_length = 0, loop_blocks = 0, chunk = 16ull << 20;
    uint32_t block = 512, dev_channels = 0, dev_rate = 0, rate = 0, world = 0, rank = 0;
    int device = -1;  // -1: not given; resolved by the parse (never negative in a mode that opens a device)
    // --sweep F1:F2:SECONDS[:RATE[:BITS]]
    double sweep_f1 = 0.0, sweep_f2 = 0.0, sweep_seconds = 0.0;
    unsigned sweep_rate = 48000;
    std::string sweep_bits = "float";

    // the groups the exclusion rules speak of
    bool stretches() const { return stretch || pitch; }
    bool levels() const { return loudness || normalize || ceiling || limit; }
    bool multi() const { return !comm_path.empty(); }
    bool multi_gpu() const { return multi() || world; }
    bool deconv_options() const { return deconv_pre || ir_length || deconv_eps != 1e-6; }
};

// what the launcher's environment says (each null when unset)
struct Env {
    const char *dspb_run_id = nullptr, *torchelastic_run_id = nullptr;
    const char *world_size = nullptr, *rank = nullptr, *local_rank = nullptr;
};

// status 0: `opt` holds the invocation.  status 2: print `message` (a whole
// line, when there is one) and then the usage text when `usage` is set.
struct Parsed {
    int status = 0;
    const char *message = nullptr;
    bool usage = false;
    Options opt;
};

Parsed parse_options(int argc, const char *const *argv, const Env &env);
const char *usage_text();
