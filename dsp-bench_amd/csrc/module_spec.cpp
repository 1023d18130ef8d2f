// module_spec.cpp -- block classes of a stateless plugin: the cache, the probe
// launches and the class tables.  The probes' values and the decision over
// their results are make_probes / classify / affine_ramp (module_policy.cpp,
// no HIP).
#include <cstring>

#include "module_impl.hpp"

namespace dspb {

// Block classes (kernels.hpp ModuleSpec).  A plugin whose blocks are
// independent (an empty State, or one its callback never writes) computes
// each block as f(Parameters, State, block, C, B, sr): it cannot see where
// the block lies in the file.  A class is taken only when the callback's own
// IR proves it (dsp_module_facts, ir_proof.cpp) and the callback, run on
// probe blocks, pins what the IR leaves open:
//   TABLE  the callback reads no sample of its block (IR), so its output is
//          one block B for every input; two probes that differ in every
//          element (zeros, noise) render the same values, so every element
//          is written: the render is that block (computed by the callback)
//          tiled, read by the fused kernels as a block table
//          (MapKind::Ramp).  All channels must render the same row.
//   GAIN   every block store is fl(x g) at the address x was loaded from,
//          with one call-invariant g, under input-independent control flow
//          (IR); a probe of ones renders g in every element, so every element
//          is stored exactly once (or the map is fl(x g) anyway): the gain
//          map with that g (MapKind::Gain).  A callback with no block store
//          at all is the identity (g = 1).
// The other probes (uniform in [-1000, 1000], signed steps with a -0) are a
// second check of the same class.  Without facts (a code object compiled
// before them) or without a proof, the callback runs on every block.
constexpr uint32_t kSpecMaxB = 1u << 16;
constexpr size_t kSpecCache = 4;

// frees the retired tables no call holds and no stream still reads (m->mu held)
void spec_reap(dsp_module *m) {
    for (size_t i = 0; i < m->retired.size();) {
        auto &u = m->retired[i];
        bool done = !u->captured && u->inflight == 0;
        for (auto &kv : u->ev) done = done && hipEventQuery(kv.second) == hipSuccess;
        if (!done) {
            ++i;
            continue;
        }
        (void)hipFree(u->table);
        for (auto &kv : u->ev) (void)hipEventDestroy(kv.second);
        m->retired.erase(m->retired.begin() + (long)i);
    }
}

// a call that rendered with a table class's block releases it: an event on
// its stream after its launches (none under capture: the table then stays
// until dsp_module_destroy)
int module_spec_done(dsp_module *m, void *use, hipStream_t s) {
    if (!m || !use) return DSP_OK;
    std::lock_guard<std::mutex> lk(m->mu);
    auto *u = static_cast<dsp_module::SpecUse *>(use);
    --u->inflight;
    if (capturing(s)) {
        u->captured = true;
    } else {
        hipEvent_t &e = u->ev[s];
        if (!e) DSPB_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        DSPB_HIP(hipEventRecord(e, s));
    }
    spec_reap(m);
    return DSP_OK;
}

size_t module_spec_retired(dsp_module *m) {
    std::lock_guard<std::mutex> lk(m->mu);
    spec_reap(m);
    return m->retired.size();
}

int module_specialize(dsp_module *m, const void *params, uint32_t params_size, uint32_t C, uint32_t B, float sr,
                      hipStream_t s, ModuleSpec *out) {
    *out = ModuleSpec{};
    if (!m || !m->initialized || !m->par || C == 0 || C > (uint32_t)kMaxChannels || B == 0 || B > kSpecMaxB)
        return DSP_OK;
    const dspb::irp::Facts &F = m->facts;
    const bool may_table = m->has_facts && F.analyzed && !F.writes_state && !F.reads_block;
    const bool may_gain = m->has_facts && F.analyzed && !F.writes_state && F.gain_form && !F.input_control;
    const bool may_gtab = m->has_facts && F.analyzed && !F.writes_state && F.gain_table_form && !F.input_control;
    if (!may_table && !may_gain && !may_gtab) return DSP_OK;  // the callback on every block
    if (!params_fit(m, params, params_size)) return DSP_OK;  // module_render reports it
    if (int st = check_device(m)) return st;
    std::lock_guard<std::mutex> lk(m->mu);
    spec_reap(m);
    for (const auto &e : m->spec)
        if (e.C == C && e.B == B && same_bits(e.sr, sr) && e.params.size() == params_size &&
            (!params_size || std::memcmp(e.params.data(), params, params_size) == 0)) {
            *out = e.r;
            if (e.use) {
                ++e.use->inflight;
                out->use = e.use.get();
            }
            return DSP_OK;
        }
    if (int st = refuse_generic_capture(s)) return st;  // probing allocates and synchronises
    if (int st = upload_params(m, params, params_size, s)) return st;
    const uint64_t n = (uint64_t)C * B;
    const std::vector<float> h = make_probes(C, B);
    float *d = nullptr;
    DSPB_HIP(hipMalloc(&d, sizeof(float) * h.size()));
    struct Free {
        float **p;
        ~Free() { if (*p) (void)hipFree(*p); }
    } fr{&d};
    DSPB_HIP(hipMemcpyAsync(d, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice, s));
    for (int p = 0; p < kProbes; ++p) {
        float *rows[kMaxChannels];
        for (uint32_t c = 0; c < C; ++c) rows[c] = d + (uint64_t)(p * C + c) * B;
        if (int st = callback_on(m, 0, rows, C, B, sr, s)) return st;
    }
    std::vector<float> r(h.size());
    DSPB_HIP(hipMemcpyAsync(r.data(), d, sizeof(float) * r.size(), hipMemcpyDeviceToHost, s));
    // g's value from where the IR says the callback reads it -- not from the
    // callback's output -- so that the probe of ones checks how often each
    // element is scaled: fl(g^k) == g for k != 1 only for g = 0, 1, -1,
    // where x g ... g = x g for every x
    float ge = 0.f;
    bool have_ge = false;
    if (may_gain) {
        if (F.gain_src == 'K') {
            std::memcpy(&ge, &F.gain_bits, 4);
            have_ge = true;
        } else if (F.gain_src == 'R') {
            ge = sr;
            have_ge = true;
        } else if (F.gain_src == 'P' && (uint64_t)F.gain_off + 4 <= params_size) {
            std::memcpy(&ge, (const char *)params + F.gain_off, 4);
            have_ge = true;
        } else if (F.gain_src == 'S' && (uint64_t)F.gain_off + 4 <= m->state_size) {
            DSPB_HIP(hipMemcpyAsync(&ge, (const char *)m->d_state[0] + F.gain_off, 4, hipMemcpyDeviceToHost, s));
            have_ge = true;
        }
    }
    DSPB_HIP(hipStreamSynchronize(s));
    const BlockClass cls = classify(h.data(), r.data(), C, B, may_table, may_gain, may_gtab, have_ge, ge);
    static_assert(kBlockTable == (int)kSpecTable && kBlockGain == (int)kSpecGain &&
                      kBlockGainTable == (int)kSpecGainTable && kBlockCallback == (int)kSpecNone,
                  "one numbering of the classes");
    ModuleSpec res{};
    res.kind = cls.kind;
    if (cls.kind == kBlockTable) {
        float *t = nullptr;
        DSPB_HIP(hipMalloc(&t, sizeof(float) * B));
        DSPB_HIP(hipMemcpyAsync(t, d, sizeof(float) * B, hipMemcpyDeviceToDevice, s));
        res.table = t;
        res.affine = affine_ramp(r.data(), B, &res.rg0, &res.rs);
    } else if (cls.kind == kBlockGain) {
        res.gain = cls.gain;
    } else if (cls.kind == kBlockGainTable) {
        float *t = nullptr;
        DSPB_HIP(hipMalloc(&t, sizeof(float) * n));
        DSPB_HIP(hipMemcpyAsync(t, d + 4 * n, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
        res.table = t;
    }
    // an evicted entry's table is retired, not freed: a call (this thread's
    // or another's) or a captured graph may still read it (spec_reap)
    if (m->spec.size() >= kSpecCache) {
        if (m->spec.front().use) m->retired.push_back(m->spec.front().use);
        m->spec.erase(m->spec.begin());
    }
    std::shared_ptr<dsp_module::SpecUse> use;
    if (res.table) {
        use = std::make_shared<dsp_module::SpecUse>();
        use->table = const_cast<float *>(res.table);
        use->inflight = 1;
    }
    m->spec.push_back({std::vector<unsigned char>((const unsigned char *)params,
                                                  (const unsigned char *)params + params_size),
                       C, B, sr, res, use});
    *out = res;
    out->use = use.get();
    return DSP_OK;
}

}  // namespace dspb
