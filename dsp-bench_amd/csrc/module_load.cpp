// module_load.cpp -- a plugin module on its device: load and destroy, the
// State and Parameters plumbing, and the render dispatch of
// DSP_PLUGIN_GENERIC (module_render: the stateless paths, the speculative
// segments of module_seg.cpp, the serial chain).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "module_impl.hpp"

using namespace dspb;

namespace {

int launch1(hipFunction_t f, void **args, hipStream_t s = nullptr) {
    DSPB_HIP(hipModuleLaunchKernel(f, 1, 1, 1, 1, 1, 1, 0, s, args, nullptr));
    return DSP_OK;
}

int make_arena(dsp_module *m, int slot, uint64_t bytes) {
    if (m->arena_mem[slot]) (void)hipFree(m->arena_mem[slot]);
    m->arena_mem[slot] = nullptr;
    if (!m->d_arena[slot]) DSPB_HIP(hipMalloc(&m->d_arena[slot], sizeof(ArenaHost)));
    if (bytes) DSPB_HIP(hipMalloc(&m->arena_mem[slot], bytes));
    if (bytes) DSPB_HIP(hipMemset(m->arena_mem[slot], 0, bytes));
    ArenaHost h{m->arena_mem[slot], bytes, 0, nullptr, 0};
    DSPB_HIP(hipMemcpy(m->d_arena[slot], &h, sizeof h, hipMemcpyHostToDevice));
    return DSP_OK;
}

int init_slot(dsp_module *m, int slot, const void *params, uint32_t C, float sr, uint64_t arena_bytes,
              hipStream_t s) {
    if (int st = wait_uses(m)) return st;
    if (!params && m->params_size > 0) {
        set_last_error("initialize_state: params blob is NULL");
        return DSP_ERR_INVALID;
    }
    int st = make_arena(m, slot, arena_bytes);
    if (st) return st;
    DSPB_HIP(hipMemcpy(m->d_params, params, m->params_size, hipMemcpyHostToDevice));
    void *a_p = m->d_params, *a_s = m->d_state[slot], *a_a = m->d_arena[slot];
    unsigned a_c = C;
    float a_sr = sr;
    void *args[] = {&a_p, &a_s, &a_c, &a_sr, &a_a};
    if ((st = launch1(m->f_init, args, s))) return st;
    ArenaHost h{};
    DSPB_HIP(hipMemcpyAsync(&h, m->d_arena[slot], sizeof h, hipMemcpyDeviceToHost, s));
    DSPB_HIP(hipStreamSynchronize(s));
    if (h.failed) {  // an allocator returned NULL: Runtime_Low_Memory (errors.inc:22-23)
        set_last_error("initialize_state: arena of %llu bytes exhausted (%llu used, a request of %llu failed)",
                       (unsigned long long)h.capacity, (unsigned long long)h.used,
                       (unsigned long long)h.failed);
        return DSP_ERR_NOMEM;
    }
    return DSP_OK;
}

}  // namespace

extern "C" {

int dsp_module_load(const void *code, uint64_t code_size, int device, dsp_module **out) {
    if (!code || !code_size || !out) {
        set_last_error("dsp_module_load: NULL argument");
        return DSP_ERR_INVALID;
    }
    *out = nullptr;
    DeviceGuard g(device);
    if (g.status) return g.status;
    dsp_module *m = new dsp_module();
    m->device = g.dev;
    if (hipDeviceGetAttribute(&m->cus, hipDeviceAttributeMultiprocessorCount, m->device) != hipSuccess || m->cus < 1)
        m->cus = 256;
    {
        dsp_descriptor *dd = new dsp_descriptor();
        if (dspb::desc::read(code, code_size, &dd->d, nullptr) == 0) m->desc = dd;
        else delete dd;
    }
    auto fail = [&](int s) {
        dsp_module_destroy(m);
        return s;
    };
    hipError_t e = hipModuleLoadData(&m->mod, code);
    if (e != hipSuccess) return fail(dspb::hip_fail(e, "hipModuleLoadData"));
    struct { hipFunction_t *f; const char *n; } fs[] = {{&m->f_sizes, "dspb_sizes"}, {&m->f_defaults, "dspb_defaults"},
                                                        {&m->f_init, "dspb_init"}, {&m->f_render, "dspb_render"},
                                                        {&m->f_callback, "dspb_callback"}};
    for (auto &f : fs)
        if ((e = hipModuleGetFunction(f.f, m->mod, f.n)) != hipSuccess) return fail(dspb::hip_fail(e, f.n));
    auto optional = [&](hipFunction_t *f, const char *name) {
        if (hipModuleGetFunction(f, m->mod, name) != hipSuccess) {
            (void)hipGetLastError();
            *f = nullptr;
        }
    };
    // a chain kernel with its private memory per lane (all or nothing)
    auto chain = [&](hipModule_t mod, hipFunction_t *f, int *priv, const char *name) {
        hipFunction_t g = nullptr;
        if (hipModuleGetFunction(&g, mod, name) != hipSuccess ||
            hipFuncGetAttribute(priv, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, g) != hipSuccess) {
            (void)hipGetLastError();
            g = nullptr;
        }
        *f = g;
    };
    for (size_t i = 0; i < std::size(kLdsShapes); ++i) optional(&m->f_render_lds[i], kLdsShapes[i].name);
    for (size_t i = 0; i < std::size(kStShapes); ++i) optional(&m->f_render_st[i], kStShapes[i].name);
    for (size_t i = 0; i < std::size(kSegShapes); ++i) {
        optional(&m->f_seg[i], kSegShapes[i].name);
        if (kSegShapes[i].rerun) optional(&m->f_seg_rerun[i], kSegShapes[i].rerun);
    }
    for (size_t i = 0; i < std::size(kWalkShapes); ++i) optional(&m->f_seg_walk[i], kWalkShapes[i].name);
    optional(&m->f_seg_check, "dspb_seg_check");
    for (size_t i = 0; i < std::size(kChainShapes); ++i) {
        chain(m->mod, &m->f_seg_chain[i], &m->chain_priv[i], kChainShapes[i].name);
        chain(m->mod, &m->f_seg_chain_ind[i], &m->chain_ind_priv[i], kChainIndShapes[i].name);
    }
    {
        // the State chain kernels compiled from the callback's edited IR
        // (dsp_module_compile: the symbol dspb_chain_co), a code object of
        // their own; the module's facts say which of them it holds
        std::string cco, ft;
        dspb::irp::Facts cf;
        if (dspb::desc::code_symbol(code, code_size, "dspb_chain_co", &cco) && !cco.empty() &&
            dspb::desc::code_symbol(code, code_size, "dspb_callback_facts", &ft)) {
            while (!ft.empty() && ft.back() == '\0') ft.pop_back();
            if (dspb::irp::decode(ft, &cf) && hipModuleLoadData(&m->chain_mod, cco.data()) == hipSuccess) {
                for (size_t i = 0; i < std::size(kChainShapes); ++i) {
                    if (!cf.state_reads_block)
                        chain(m->chain_mod, &m->f_seg_chain[i], &m->chain_priv[i], kChainShapes[i].name);
                    chain(m->chain_mod, &m->f_seg_chain_ind[i], &m->chain_ind_priv[i], kChainIndShapes[i].name);
                }
            } else {
                (void)hipGetLastError();
                m->chain_mod = nullptr;
            }
        }
    }
    unsigned *d_o = nullptr;
    if ((e = hipMalloc(&d_o, 4 * sizeof(unsigned))) != hipSuccess) return fail(dspb::hip_fail(e, "hipMalloc"));
    void *args[] = {&d_o};
    int st = launch1(m->f_sizes, args);
    unsigned h[4] = {0, 0, 0, 0};
    if (!st && (e = hipMemcpy(h, d_o, sizeof h, hipMemcpyDeviceToHost)) != hipSuccess) st = dspb::hip_fail(e, "sizes");
    (void)hipFree(d_o);
    if (st) return fail(st);
    m->params_size = h[0];
    m->state_size = h[1];
    m->stateless = (int)h[2];
    {
        std::string ft;
        if (dspb::desc::code_symbol(code, code_size, "dspb_callback_facts", &ft)) {
            while (!ft.empty() && ft.back() == '\0') ft.pop_back();
            m->has_facts = dspb::irp::decode(ft, &m->facts);
        }
        m->par = (m->has_facts && m->facts.analyzed && !m->facts.writes_state) ? 1 : 0;
    }
    if ((e = hipMalloc(&m->d_params, m->params_size ? m->params_size : 1)) != hipSuccess ||
        (e = hipMalloc(&m->d_state[0], m->state_size ? m->state_size : 1)) != hipSuccess ||
        (e = hipMalloc(&m->d_state[1], m->state_size ? m->state_size : 1)) != hipSuccess)
        return fail(dspb::hip_fail(e, "hipMalloc"));
    (void)hipMemset(m->d_state[0], 0, m->state_size ? m->state_size : 1);
    (void)hipMemset(m->d_state[1], 0, m->state_size ? m->state_size : 1);
    *out = m;
    return DSP_OK;
}

void dsp_module_destroy(dsp_module *m) {
    if (!m) return;
    DeviceGuard g(m->device);
    if (g.status == DSP_OK) {
        for (int i = 0; i < 2; ++i) {
            if (m->d_state[i]) (void)hipFree(m->d_state[i]);
            if (m->d_arena[i]) (void)hipFree(m->d_arena[i]);
            if (m->arena_mem[i]) (void)hipFree(m->arena_mem[i]);
        }
        if (m->d_params) (void)hipFree(m->d_params);
        (void)hipDeviceSynchronize();  // no launch may still read a table
        for (auto &e : m->spec)
            if (e.use) m->retired.push_back(e.use);
        for (auto &u : m->retired) {
            (void)hipFree(u->table);
            for (auto &kv : u->ev) (void)hipEventDestroy(kv.second);
        }
        for (hipEvent_t e : {m->upload_ev, m->use_ev, m->seg.ev[0], m->seg.ev[1]})
            if (e) {
                (void)hipEventSynchronize(e);
                (void)hipEventDestroy(e);
            }
        if (m->h_params) (void)hipHostFree(m->h_params);
        if (m->seg.h_stats) (void)hipHostFree(m->seg.h_stats);
        if (m->mod) (void)hipModuleUnload(m->mod);
        if (m->chain_mod) (void)hipModuleUnload(m->chain_mod);
    }
    delete m->desc;
    delete m;  // (the segment workspaces go with it: DevBuf)
}

int dsp_module_block_class(dsp_module *m, const void *params, uint32_t params_size, uint32_t C, uint32_t B,
                           float sr, int32_t *block_class, float *gain, const dsp_exec *ex) {
    if (!m || !block_class) {
        set_last_error("dsp_module_block_class: NULL argument");
        return DSP_ERR_INVALID;
    }
    DeviceGuard g(ex && ex->device >= 0 ? ex->device : m->device);
    if (g.status) return g.status;
    dspb::ModuleSpec r;
    const int st = dspb::module_specialize(m, params, params_size, C, B, sr, ex ? (hipStream_t)ex->stream : nullptr, &r);
    if (!st && r.use) (void)dspb::module_spec_done(m, r.use, ex ? (hipStream_t)ex->stream : nullptr);  // no launch
    if (st) return st;
    *block_class = r.kind == dspb::kSpecTable ? DSP_BLOCK_TABLE
                   : r.kind == dspb::kSpecGain ? DSP_BLOCK_GAIN
                   : r.kind == dspb::kSpecGainTable ? DSP_BLOCK_GAIN_TABLE
                                                   : DSP_BLOCK_CALLBACK;
    if (gain) *gain = r.gain;
    return DSP_OK;
}

int dsp_module_retired_tables(dsp_module *m, uint64_t *n) {
    if (!m || !n) return DSP_ERR_INVALID;
    *n = dspb::module_spec_retired(m);
    return DSP_OK;
}

int dsp_module_state_spec(dsp_module *m, dsp_state_spec_info *out) {
    if (!m || !out) {
        set_last_error("dsp_module_state_spec: NULL argument");
        return DSP_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(m->mu);
    if (int st = dspb::module_seg_collect(m, true)) return st;
    *out = m->learn.serial ? dsp_state_spec_info{} : m->learn.last;
    out->disabled = (m->learn.off || m->learn.chain_bad) ? 1 : 0;
    return DSP_OK;
}

int dsp_module_debug(dsp_module *m, int what, uint64_t value) {
    if (!m || what != DSP_MODULE_DEBUG_PERTURB_CHAIN || value == ~0ull) {
        set_last_error("dsp_module_debug: unknown hook");
        return DSP_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(m->mu);
    m->seg.perturb = value + 1;
    return DSP_OK;
}

int dsp_module_seg_timing(dsp_module *m, uint32_t out[8]) {
    if (!m || !out) return DSP_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    std::memset(out, 0, 8 * sizeof(uint32_t));
    if (!m->seg.words.p) return DSP_OK;
    DSPB_HIP(hipDeviceSynchronize());
    static_assert(DSPB_STAT_WORDS - DSPB_STAT_TIMING == 8, "out[8]: the timing words");
    DSPB_HIP(hipMemcpy(out, m->seg.words.p + DSPB_WORD_STATS + DSPB_STAT_TIMING, 8 * sizeof(uint32_t),
                       hipMemcpyDeviceToHost));
    return DSP_OK;
}

int dsp_module_sizes(const dsp_module *m, uint32_t *params_size, uint32_t *state_size, int *stateless) {
    if (!m) return DSP_ERR_INVALID;
    if (params_size) *params_size = m->params_size;
    if (state_size) *state_size = m->state_size;
    if (stateless) *stateless = m->par;
    return DSP_OK;
}

int dsp_module_default_parameters(dsp_module *m, void *params) {
    if (!m || (!params && m->params_size)) return DSP_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    if (int st = wait_uses(m)) return st;
    DeviceGuard g(m->device);
    if (g.status) return g.status;
    void *a_p = m->d_params;
    void *args[] = {&a_p};
    if (int st = launch1(m->f_defaults, args)) return st;
    DSPB_HIP(hipMemcpy(params, m->d_params, m->params_size, hipMemcpyDeviceToHost));
    return DSP_OK;
}

int dsp_module_initialize_state(dsp_module *m, const void *params, uint32_t C, float sr, uint64_t arena_bytes) {
    if (!m) return DSP_ERR_INVALID;
    if (C == 0 || C > (uint32_t)dspb::kMaxChannels) {
        set_last_error("channels must be 1..%d", dspb::kMaxChannels);
        return DSP_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(m->mu);
    DeviceGuard g(m->device);
    if (g.status) return g.status;
    const int st = init_slot(m, 0, params, C, sr, arena_bytes, nullptr);
    m->initialized = (st == DSP_OK);
    // block classes were found with the previous State: forget them (their
    // tables are freed once no call holds them, dspb::spec_reap)
    for (auto &e : m->spec)
        if (e.use) m->retired.push_back(e.use);
    m->spec.clear();
    dspb::spec_reap(m);
    return st;
}

const dsp_descriptor *dsp_module_descriptor(const dsp_module *m) { return m ? m->desc : nullptr; }

int dsp_descriptor_from_code(const void *code, uint64_t code_size, dsp_descriptor **out) {
    if (!code || !code_size || !out) {
        set_last_error("dsp_descriptor_from_code: NULL argument");
        return DSP_ERR_INVALID;
    }
    *out = nullptr;
    dsp_descriptor *d = new dsp_descriptor();
    std::string err;
    if (dspb::desc::read(code, code_size, &d->d, &err) != 0) {
        delete d;
        set_last_error("%s", err.c_str());
        return DSP_ERR_INVALID;
    }
    *out = d;
    return DSP_OK;
}

int dsp_module_read_state(const dsp_module *m, void *state) {
    if (!m || (!state && m->state_size)) return DSP_ERR_INVALID;
    if (int st = wait_uses(const_cast<dsp_module *>(m))) return st;
    DSPB_HIP(hipMemcpy(state, m->d_state[0], m->state_size, hipMemcpyDeviceToHost));
    return DSP_OK;
}

}  // extern "C"

namespace dspb {

// DSPB_STATELESS_PATH=0 / 3 forces the in-place wave path / the LDS-blocks
// path for a stateless plugin (tools/generic_probe.py A/B); -1: by size
static int stateless_path_forced() {
    static const int v = [] {
        const char *e = std::getenv("DSPB_STATELESS_PATH");
        return e && (e[0] == '0' || e[0] == '3') ? e[0] - '0' : -1;
    }();
    return v;
}

// the caller's Parameters blob -> the module's device Parameters, stream
// ordered: through a pinned staging copy (reused once the previous upload
// from it has completed), behind every earlier render's use of the device
// Parameters on any stream (use_ev), so the call returns without a sync
int upload_params(dsp_module *m, const void *params, uint32_t n, hipStream_t s) {
    if (!m->upload_ev) {
        DSPB_HIP(hipEventCreateWithFlags(&m->upload_ev, hipEventDisableTiming));
        DSPB_HIP(hipEventCreateWithFlags(&m->use_ev, hipEventDisableTiming));
        DSPB_HIP(hipEventRecord(m->upload_ev, s));
        DSPB_HIP(hipEventRecord(m->use_ev, s));
    }
    DSPB_HIP(hipStreamWaitEvent(s, m->use_ev, 0));
    if (!n) return DSP_OK;
    if (!m->h_params) DSPB_HIP(hipHostMalloc(&m->h_params, n, hipHostMallocDefault));
    DSPB_HIP(hipEventSynchronize(m->upload_ev));
    std::memcpy(m->h_params, params, n);
    DSPB_HIP(hipMemcpyAsync(m->d_params, m->h_params, n, hipMemcpyHostToDevice, s));
    DSPB_HIP(hipEventRecord(m->upload_ev, s));
    return DSP_OK;
}

// A GENERIC render cannot be captured into a graph: its Parameters upload
// waits on the host for the pinned staging buffer and copies from it, so a
// replay would upload whatever a later call left there.  Refused instead.
int refuse_generic_capture(hipStream_t s) {
    if (capturing(s)) {
        set_last_error("GENERIC plugin: calls cannot be captured into a graph (the Parameters upload is "
                       "host-staged); call it eagerly");
        return DSP_ERR_INVALID;
    }
    return DSP_OK;
}

// the module's code object, Parameters and State live on m->device: a call
// made on another device (e.g. a mis-wired shard rank) is refused
int check_device(const dsp_module *m) {
    int dev = -1;
    DSPB_HIP(hipGetDevice(&dev));
    if (dev != m->device) {
        set_last_error("GENERIC plugin: module loaded on device %d, called on device %d", m->device, dev);
        return DSP_ERR_INVALID;
    }
    return DSP_OK;
}

int check_params(const dsp_module *m, const void *params, uint32_t n) {
    if (!params_fit(m, params, n)) {
        set_last_error("GENERIC plugin: params blob is %u bytes, the plugin's Parameters %u", n, m->params_size);
        return DSP_ERR_INVALID;
    }
    return DSP_OK;
}

int callback_on(dsp_module *m, int slot, float *const *rows, uint32_t C, uint32_t B, float sr, hipStream_t s) {
    dspb_render_args A{};
    A.P = m->d_params;
    A.S = m->d_state[slot];
    for (uint32_t c = 0; c < C; ++c) A.out[c] = rows[c];
    A.C = C;
    A.B = B;
    A.sr = sr;
    void *args[] = {&A};
    DSPB_HIP(hipModuleLaunchKernel(m->f_callback, 1, 1, 1, 1, 1, 1, 0, s, args, nullptr));
    if (!m->use_ev) DSPB_HIP(hipEventCreateWithFlags(&m->use_ev, hipEventDisableTiming));
    DSPB_HIP(hipEventRecord(m->use_ev, s));
    return DSP_OK;
}

// dsp_render_offline / dsp_render_stft with DSP_PLUGIN_GENERIC (device buffers)
int module_render(dsp_module *m, const void *params, uint32_t params_size, const float *const *in,
                  uint32_t in_ch, uint64_t L, float *const *out, uint32_t C, uint32_t B, float sr,
                  uint64_t goff, hipStream_t s, uint32_t flags) {
    if (!m || !m->initialized) {
        set_last_error("GENERIC plugin: module not loaded / initialize_state not run");
        return DSP_ERR_INVALID;
    }
    if (int st = check_device(m)) return st;
    if (int st = refuse_generic_capture(s)) return st;
    if (int st = check_params(m, params, params_size)) return st;
    if (C > (uint32_t)kMaxChannels || in_ch > (uint32_t)kMaxChannels) {
        set_last_error("GENERIC plugin: at most %d channels", kMaxChannels);
        return DSP_ERR_INVALID;
    }
    if (goff % B) {
        set_last_error("sample_offset must be a multiple of B");
        return DSP_ERR_INVALID;
    }
    const bool par = m->par != 0;
    if (!par && goff) {
        set_last_error("GENERIC plugin with State: whole files only (sample_offset 0)");
        return DSP_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(m->mu);
    if (int st = upload_params(m, params, params_size, s)) return st;
    dspb_render_args A{};
    A.P = m->d_params;
    A.S = m->d_state[0];
    for (uint32_t c = 0; c < in_ch; ++c) A.in[c] = const_cast<float *>(in[c]);
    for (uint32_t c = 0; c < C; ++c) A.out[c] = out[c];
    A.L = L;
    A.nblocks = (L + B - 1) / B;
    A.block0 = goff / B;
    A.in_ch = in_ch;
    A.C = C;
    A.B = B;
    A.sr = sr;
    A.par = (unsigned)m->par;
    if (A.nblocks == 0) return DSP_OK;
    void *args[] = {&A};
    unsigned grid = 1, block = 1, lds_bytes = 0;
    if (par) {
        // default: the LDS-blocks path (dspb_render_lds) when a round of at
        // least 4 blocks fits the per-workgroup LDS budget, else the
        // in-place wave path; DSPB_STATELESS_PATH=0/3 forces one
        // the most specific instantiation for (C, B); a constant shape runs
        // the software-pipelined rounds of dspb_stateless_lds_pf, on a
        // persistent grid of two workgroups per CU
        const int fi = pick_shape(kLdsShapes, C, B, [&](size_t i) { return m->f_render_lds[i] != nullptr; });
        hipFunction_t f = fi < 0 ? nullptr : m->f_render_lds[fi];
        const bool persistent = fi >= 0 && dspb_lds_pipelined(kLdsShapes[fi].C, kLdsShapes[fi].B);
        const uint64_t stride = persistent ? dspb_stride_pf(C, B) : dspb_stride(C, B);
        const uint64_t nb = dspb_lds_nb(stride);  // blocks per round
        int path = stateless_path_forced();
        if (path < 0) path = nb >= 4 ? 3 : 0;
        if (path == 3 && (nb < 4 || !f)) path = 0;
        if (path == 3) {
            A.lds = 3;
            A.lds_nb = (unsigned)nb;
            A.lds_stride = (unsigned)stride;
            uint64_t g = (A.nblocks + nb - 1) / nb;
            if (persistent) g = std::min<uint64_t>(g, kLdsWgPerCu * m->cus);
            DSPB_HIP(hipModuleLaunchKernel(f, (unsigned)(g < (1u << 20) ? g : (1u << 20)), 1, 1, 256, 1, 1,
                                          (unsigned)(nb * stride * sizeof(float)), s, args, nullptr));
            DSPB_HIP(hipEventRecord(m->use_ev, s));
            return DSP_OK;
        }
        block = 64;  // one wave per 64 blocks
        const uint64_t g = (A.nblocks + 63) / 64;
        grid = (unsigned)(g < 65535 ? g : 65535);
    }
    // a State the callback writes, and no other memory (the analysis), a
    // State a lane can copy, rows apart: speculative segments, the serial
    // chain's bits (module_render_seg)
    if (!par && !(flags & DSP_EXEC_SERIAL_STATE) && m->has_facts && m->facts.analyzed && m->facts.writes_state &&
        m->state_size > 0 && m->state_size <= kSegMaxState &&
        !rows_overlap(Rows{in, in_ch, L}, Rows{out, C, A.nblocks * B})) {
        SegLearner &W = m->learn;
        if (int st = module_seg_collect(m, false)) return st;
        W.begin(params, params_size, C, B);
        // (learned never to forget: the State chain, then the segments exactly)
        // (the chain's records failed their check once: the serial chain)
        const int st = W.chain_bad ? 1 : module_render_seg(m, A, s, W.off);
        W.serial = st > 0;
        if (st <= 0) return st;
    }
    if (!par) m->learn.serial = true;
    hipFunction_t f = m->f_render;
    if (!par && 2ull * C * B * sizeof(float) <= kStagedLdsBytes) {
        // stateful: 4 waves, the block double-buffer in LDS (the callback's
        // loads and stores hit LDS, the copies run on 192 lanes beside it)
        A.lds = 1;
        block = 256;
        lds_bytes = (unsigned)(2ull * C * B * sizeof(float));
        const int fi = pick_shape(kStShapes, C, B, [&](size_t i) { return m->f_render_st[i] != nullptr; });
        if (fi >= 0) f = m->f_render_st[fi];
    }
    DSPB_HIP(hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, lds_bytes, s, args, nullptr));
    DSPB_HIP(hipEventRecord(m->use_ev, s));
    return DSP_OK;
}

// The callback once on device buffers, with the live State (DSP_EXEC_VERIFY_CLASS:
// blocks of a call rendered by a block class, re-run through the callback).
// Only for a module whose blocks are independent (par): its callback never
// writes the State, so this run leaves it as it was.
int module_callback_once(dsp_module *m, const void *params, uint32_t params_size, float *const *bufs, uint32_t C,
                         uint32_t B, float sr, hipStream_t s) {
    if (!m || !m->par || !m->initialized) {
        set_last_error("module_callback_once: a loaded module with independent blocks is needed");
        return DSP_ERR_INVALID;
    }
    if (C == 0 || C > (uint32_t)kMaxChannels || params_size != m->params_size) return DSP_ERR_INVALID;
    if (int st = check_device(m)) return st;
    std::lock_guard<std::mutex> lk(m->mu);
    if (int st = upload_params(m, params, params_size, s)) return st;
    return callback_on(m, 0, bufs, C, B, sr, s);
}

// dsp_ir_analysis with DSP_PLUGIN_GENERIC: fresh scratch State (compute_IR,
// plugin.cpp:33-49), then the callback once on the impulse buffers.
int module_ir(dsp_module *m, const void *params, uint32_t params_size, float *const *bufs, uint32_t C,
              uint32_t n, float sr, hipStream_t s) {
    if (!m) return DSP_ERR_INVALID;
    if (C == 0 || C > (uint32_t)kMaxChannels) {  // the driver's channel table holds 16 pointers
        set_last_error("GENERIC plugin: 1..%d channels", kMaxChannels);
        return DSP_ERR_INVALID;
    }
    if (int st = check_device(m)) return st;
    if (int st = refuse_generic_capture(s)) return st;
    if (int st = check_params(m, params, params_size)) return st;
    std::lock_guard<std::mutex> lk(m->mu);
    if (int st = init_slot(m, 1, params, C, sr, 16ull << 20, s)) return st;
    return callback_on(m, 1, bufs, C, n, sr, s);
}

}  // namespace dspb
