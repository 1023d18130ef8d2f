// module.cpp -- generic GPU dispatch: plugin source -> hiprtc -> gfx950 code
// object -> kernels that call the plugin's own functions (module.h).  This
// file is the part that needs no device: the plugin compiler, the analysis of
// the callback's IR and the facts API.  The rest of the module host:
//   module_load.cpp    load / destroy, State and Parameters, the render dispatch
//   module_seg.cpp     a State-writing callback as speculative segments
//   module_spec.cpp    block classes of a stateless callback (the probes)
//   module_policy.cpp  what the segments learn and how probe results classify:
//                      plain C++ without HIP, tested on the CPU
//   module_impl.hpp    dsp_module and the kernel shape tables they share
//   descriptor.cpp     the parameter descriptor and its C API
//
// The generated translation unit is, in order:
//   plugin_device.h          (as "plugin_header.h": device services)
//   #pragma clang force_cuda_host_device begin
//   #define annotate(...)     (the annotations are read from the text)
//   the plugin source         (unchanged; its #include of plugin_header.h
//                              hits the include guard)
//   #pragma clang force_cuda_host_device end
//   the descriptor            (dspb_desc_blob / dspb_desc_text, descriptor.cpp)
//   kDriver                   (dspb_sizes / _defaults / _init / _render /
//                              _callback kernels)
// compiled with -ffp-contract=off so the plugin's float / double arithmetic
// rounds as the CPU build of the same source does.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "module_impl.hpp"

using dspb::set_last_error;

namespace {

#include "plugin_device_src.inc"  // const char kPluginDeviceSrc[] (generated from plugin_device.h)

// kDriver / kSegDriver: plugin_driver_abi.h + the driver kernels
// (csrc/plugin_driver.inl) and the speculative-segment kernels
// (csrc/plugin_driver_seg.inl), as strings
#include "plugin_driver_src.inc"

// The plugin source inside the device-service header and a
// force_cuda_host_device region: the head of both translation units (the
// module's and the analysis kernel's).
std::string plugin_prelude() {
    std::string tu;
    tu += "#include \"plugin_header.h\"\n";
    tu += "#pragma clang force_cuda_host_device begin\n";
    // the parameter annotations are read from the source text (descriptor.cpp);
    // compiled, each access to an annotated field would go through
    // llvm.ptr.annotation, an opaque pointer that keeps the field in memory
    // (a reload after every LDS store of the callback): drop the attribute
    tu += "#define annotate(...)\n#define __annotate__(...)\n";
    tu += "#include \"dspb_plugin_source.cpp\"\n";
    tu += "#undef annotate\n#undef __annotate__\n";
    tu += "#pragma clang force_cuda_host_device end\n";
    return tu;
}

// The callback's facts (ir_proof.hpp): the plugin compiled again, as a
// flattened analysis kernel, at -O2 without vectorisation or unrolling (the
// same IEEE semantics as the module's -O3 code; scalar IR is what the
// analysis reads), with the module compile's language options.
dspb::irp::Facts analyze_source(const char *source, bool shipped = false) {
    static const char *kProof =
        "extern \"C\" __global__ __attribute__((flatten)) void dspb_proof(Parameters *P, State *S, float **out, "
        "unsigned C, unsigned B, float sr) { audio_callback(*P, *S, out, C, B, sr); }\n";
    dspb::irp::Facts f;
    std::string ir, log;
    const int rc = dspb::irp::compile_to_ir(plugin_prelude() + kProof,
                                            {{"plugin_header.h", kPluginDeviceSrc}, {"dspb_plugin_source.cpp", source}},
                                            shipped ? std::vector<std::string>{"-O3", "-std=c++20", "-ffp-contract=off", "-w"}
                                                    : std::vector<std::string>{"-O2", "-std=c++20", "-ffp-contract=off", "-w",
                                                                               "-fno-vectorize", "-fno-slp-vectorize",
                                                                               "-fno-unroll-loops"},
                                            &ir, &log);
    if (rc != 0) {
        f.why = "the analysis compile failed: " + log.substr(0, 300);
        return f;
    }
    if (const char *dump = std::getenv("DSPB_PROOF_IR")) {  // diagnostics: the IR the analysis reads
        if (FILE *fp = std::fopen(dump, "w")) {
            std::fwrite(ir.data(), 1, ir.size(), fp);
            std::fclose(fp);
        }
    }
    return dspb::irp::analyze(ir, "dspb_proof");
}

}  // namespace

extern "C" {

int dsp_module_compile(const char *source, const char *name, void **code, uint64_t *code_size, char *log,
                       uint64_t log_cap) {
    if (log && log_cap) log[0] = 0;
    if (!source || !code || !code_size) {
        set_last_error("dsp_module_compile: NULL argument");
        return DSP_ERR_INVALID;
    }
    *code = nullptr;
    *code_size = 0;
    std::string tu = plugin_prelude();
    std::string note;
    tu += dspb::desc::generate(source, kPluginDeviceSrc, &note);
    // what the callback does with its block, from its own IR (ir_proof.cpp),
    // stored in the code object for dsp_module_load
    const dspb::irp::Facts facts = analyze_source(source);
    tu += "extern \"C\" __attribute__((used, visibility(\"default\"))) __device__ const unsigned char "
          "dspb_callback_facts[] = {" + dspb::desc::hex_literal(dspb::irp::encode(facts)) + "};\n";
    tu += "#define DSPB_ABI_STATE State\n";  // plugin_driver_abi.h, at the front of kDriver
    tu += kDriver;
    // the segment kernels only where they can run: a callback the analysis
    // bounded that writes its State (the loader treats them as optional)
    if (facts.analyzed && facts.writes_state) {
        // a split State: the words a block-dependent store may hit (kSegDriver
        // dspb_state_dep_words; the State chain of the others)
        if (facts.state_split && !facts.state_dep_words.empty()) {
            tu += "#define DSPB_STATE_DEP_WORDS ";
            for (size_t i = 0; i < facts.state_dep_words.size(); ++i)
                tu += (i ? "," : "") + std::to_string(facts.state_dep_words[i]);
            tu += "\n";
        }
        // diagnostics: pass 1's phase clocks (dsp_module_seg_timing)
        if (std::getenv("DSPB_SEG_TIMING")) tu += "#define DSPB_SEG_TIMING 1\n";
        tu += kSegDriver;
    }
    const std::string round = "-DDSPB_LDS_ROUND_BYTES=" + std::to_string(kLdsRoundBytes) + "u";
    // State chain kernels from the callback's IR with its block stores
    // deleted (ir_proof.cpp strip_chain_block_stores), so that they keep only
    // the State's arithmetic: every chain kernel when no State value depends
    // on the block (a tremolo's phase, not its output), the chain of a split
    // State's block-independent words (dspb_seg_chain_ind_*) when the State
    // splits.  Compiled through comgr from the same translation unit into a
    // code object of their own, carried inside the module's as the symbol
    // dspb_chain_co (dsp_module_load takes the chain kernels from it); every
    // other kernel is the hiprtc compile below.  Nothing is carried if any
    // step fails: the hiprtc chain kernels stand.
    if (facts.analyzed && facts.writes_state && (!facts.state_reads_block || facts.state_split)) {
        std::string ir, clog, co;
        int dropped = 0;
        const char *prefix = facts.state_reads_block ? "@dspb_seg_chain_ind_" : "@dspb_seg_chain_";
        if (dspb::irp::compile_to_ir(tu, {{"plugin_header.h", kPluginDeviceSrc}, {"dspb_plugin_source.cpp", source}},
                                     {"-O3", "-std=c++20", "-ffp-contract=off", "-w", "-fno-discard-value-names",
                                      round},
                                     &ir, &clog) == 0 &&
            (dropped = dspb::irp::strip_chain_block_stores(&ir, prefix)) > 0 &&
            dspb::irp::codegen_ir(ir, {"-O3", "-ffp-contract=off"}, &co, &clog) == 0) {
            tu += "extern \"C\" __attribute__((used, visibility(\"default\"))) __device__ const unsigned char "
                  "dspb_chain_co[] = {" + dspb::desc::hex_literal(co) + "};\n";
        } else if (dropped < 0) {
            note += "State chain: a store outside the block-store model, compiled from source\n";
        } else if (dropped == 0 && clog.empty()) {
            note += "State chain: no block store to drop\n";
        } else {
            note += "State chain compiled from source: " + clog.substr(0, 200) + "\n";
        }
    }
    std::vector<const char *> hdrs = {kPluginDeviceSrc, source}, hnames = {"plugin_header.h", "dspb_plugin_source.cpp"};
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, tu.c_str(), name ? name : "plugin.cpp", (int)hdrs.size(), hdrs.data(),
                            hnames.data()) != HIPRTC_SUCCESS) {
        set_last_error("hiprtcCreateProgram failed");
        return DSP_ERR_INVALID;
    }
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++20", "-ffp-contract=off", "-w", round.c_str()};
    const hiprtcResult rc = hiprtcCompileProgram(prog, (int)(sizeof opts / sizeof *opts), opts);
    size_t ls = 0;
    hiprtcGetProgramLogSize(prog, &ls);
    std::vector<char> lg(ls + 1, 0);
    if (ls) hiprtcGetProgramLog(prog, lg.data());
    if (log && log_cap) {
        std::strncpy(log, lg.data(), log_cap - 1);
        log[log_cap - 1] = 0;
    }
    if (rc != HIPRTC_SUCCESS) {
        hiprtcDestroyProgram(&prog);
        set_last_error("plugin compile failed: %.400s", lg.data());
        return DSP_ERR_INVALID;
    }
    size_t cs = 0;
    hiprtcGetCodeSize(prog, &cs);
    void *buf = std::malloc(cs ? cs : 1);
    if (!buf) {
        hiprtcDestroyProgram(&prog);
        return DSP_ERR_NOMEM;
    }
    hiprtcGetCode(prog, (char *)buf);
    hiprtcDestroyProgram(&prog);
    // the parameter descriptor, validated as the reference's JIT does
    // (compiler.cpp:944-1164): an invalid annotation fails the compile
    dspb::desc::Descriptor d;
    std::string derr;
    if (dspb::desc::read(buf, cs, &d, &derr) != 0) note += "descriptor: " + derr + "\n";
    std::string bad;
    for (const auto &p : d.params)
        if (p.error != dspb::desc::kSuccess)
            bad += "parameter '" + p.name + "' (annotate \"" + p.annotation + "\"): " +
                   dspb::desc::error_name(p.error) + "\n";
    if (log && log_cap) {
        const std::string all = std::string(lg.data()) + note + bad;
        std::strncpy(log, all.c_str(), log_cap - 1);
        log[log_cap - 1] = 0;
    }
    if (!bad.empty()) {
        std::free(buf);
        set_last_error("plugin descriptor: %.400s", bad.c_str());
        return DSP_ERR_INVALID;
    }
    *code = buf;
    *code_size = cs;
    return DSP_OK;
}

void dsp_module_free_code(void *code) { std::free(code); }

int dsp_ir_strip_chain_stores(const char *ir, char *out, uint64_t out_cap, int32_t *dropped) {
    if (!ir || !dropped) {
        set_last_error("dsp_ir_strip_chain_stores: NULL argument");
        return DSP_ERR_INVALID;
    }
    std::string t(ir);
    *dropped = dspb::irp::strip_chain_block_stores(&t);
    if (out && out_cap) {
        if (t.size() + 1 > out_cap) {
            set_last_error("dsp_ir_strip_chain_stores: %llu bytes needed", (unsigned long long)t.size() + 1);
            return DSP_ERR_INVALID;
        }
        std::memcpy(out, t.c_str(), t.size() + 1);
    }
    return DSP_OK;
}

static void facts_out(const dspb::irp::Facts &f, bool present, dsp_callback_facts *o) {
    std::memset(o, 0, sizeof *o);
    o->present = present ? 1 : 0;
    o->analyzed = f.analyzed;
    o->reads_block = f.reads_block;
    o->writes_state = f.writes_state;
    o->input_control = f.input_control;
    o->gain_form = f.gain_form;
    std::strncpy(o->gain, f.gain_expr.c_str(), sizeof o->gain - 1);
    o->gain_source = f.gain_src;
    o->gain_offset = f.gain_off;
    std::memcpy(&o->gain_constant, &f.gain_bits, 4);
    std::strncpy(o->why, f.why.c_str(), sizeof o->why - 1);
    o->gain_table_form = f.gain_table_form;
    std::strncpy(o->table_why, f.table_why.c_str(), sizeof o->table_why - 1);
    o->state_reads_block = f.state_reads_block;
    o->state_split = f.state_split;
    std::string dw;
    for (int64_t w : f.state_dep_words)
        dw += (dw.empty() ? "" : ",") + (w >= 0 ? std::to_string(w) : std::to_string(-w - 2) + "-");
    std::strncpy(o->state_dep_words, dw.c_str(), sizeof o->state_dep_words - 1);
}

int dsp_module_facts(const dsp_module *m, dsp_callback_facts *out) {
    if (!m || !out) return DSP_ERR_INVALID;
    facts_out(m->facts, m->has_facts, out);
    return DSP_OK;
}

int dsp_code_facts(const void *code, uint64_t code_size, dsp_callback_facts *out) {
    if (!code || !out) return DSP_ERR_INVALID;
    dspb::irp::Facts f;
    std::string ft;
    bool present = false;
    if (dspb::desc::code_symbol(code, code_size, "dspb_callback_facts", &ft)) {
        while (!ft.empty() && ft.back() == '\0') ft.pop_back();
        present = dspb::irp::decode(ft, &f);
    }
    facts_out(f, present, out);
    return DSP_OK;
}

int dsp_plugin_analyze(const char *source, dsp_callback_facts *out) {
    if (!source || !out) {
        set_last_error("dsp_plugin_analyze: NULL argument");
        return DSP_ERR_INVALID;
    }
    facts_out(analyze_source(source), true, out);
    return DSP_OK;
}

int dsp_plugin_analyze_shipped(const char *source, dsp_callback_facts *out) {
    if (!source || !out) {
        set_last_error("dsp_plugin_analyze_shipped: NULL argument");
        return DSP_ERR_INVALID;
    }
    facts_out(analyze_source(source, true), true, out);
    return DSP_OK;
}

}  // extern "C"
