#include "wavio.hpp"

#include <cstdlib>
#include <cstring>

#include "dspbench/dspbench.h"

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

int write_file(const char *path, std::initializer_list<std::pair<const void *, size_t>> pieces) {
    FILE *f = std::fopen(path, "wb");
    bool ok = f != nullptr;
    for (const auto &p : pieces) ok = ok && std::fwrite(p.first, 1, p.second, f) == p.second;
    if (f) std::fclose(f);
    if (!ok) std::fprintf(stderr, "dspbench_render: cannot write %s\n", path);
    return ok ? 0 : 1;
}

// wav_reader.h:57-205 (load + parse), audio.h:66-121 (decode to planar float)
int load_wav(const char *path, const char *role, const std::function<int(const dsp_wav_info &)> &limits, Device &dev,
             Wav &w) {
    std::vector<unsigned char> file;
    if (!read_file(path, file)) {
        std::fprintf(stderr, "dspbench_render: cannot read %s\n", path);
        return 1;
    }
    int st = dsp_wav_parse(file.data(), file.size(), &w.info);
    if (st) return fail((std::string("dsp_wav_parse") + role).c_str(), st);
    if (int refused = limits(w.info)) return refused;
    w.payload.resize(w.info.data_bytes);
    for (uint64_t c = 0, o = 0; c < w.info.n_data_chunks; ++c) {
        std::memcpy(w.payload.data() + o, file.data() + w.info.data_offset[c], w.info.data_size[c]);
        o += w.info.data_size[c];
    }
    file.clear();
    file.shrink_to_fit();  // (given back before the device's clock starts)
    if (int e = dev.open()) return e;
    HIPCK(hipMalloc(&w.d_payload.h, w.payload.size() + 16));
    HIPCK(hipMemcpyAsync(w.d_payload.h, w.payload.data(), w.payload.size(), hipMemcpyHostToDevice, dev.stream.h));
    HIPCK(w.rows.alloc(w.info.channels, w.info.frames ? w.info.frames : 1));  // (an empty file still decodes)
    if ((st = dsp_wav_decode(w.d_payload.h, &w.info, 0, w.info.frames, w.rows.ptr.data(), &dev.ex)))
        return fail("dsp_wav_decode", st);
    return 0;
}

int resample_rows(Rows &rows, uint32_t C, uint64_t &L, uint32_t from, uint32_t to, const char *role,
                  const std::function<int(uint64_t)> &limits, Device &dev) {
    uint64_t Ln = 0;
    int st = dsp_resample_plan(from, to, L, nullptr, nullptr, nullptr, nullptr, &Ln, nullptr);
    if (st) return fail((std::string("dsp_resample_plan") + role).c_str(), st);
    if (int refused = limits(Ln)) return refused;
    Rows now;
    HIPCK(now.alloc(C, Ln ? Ln : 1));
    if ((st = dsp_resample(rows.ptr.data(), C, L, now.ptr.data(), Ln, from, to, nullptr, &dev.ex)))
        return fail((std::string("dsp_resample") + role).c_str(), st);
    HIPCK(hipStreamSynchronize(dev.stream.h));
    for (uint32_t c = 0; c < C; ++c) rows.replace(c, std::move(now.own[c]));
    L = Ln;
    return 0;
}

Format resolve_bits(const std::string &bits_opt, Format otherwise) {
    if (bits_opt.empty()) return otherwise;
    if (bits_opt == "float") return {DSP_WAV_FORMAT_FLOAT, 32};
    return {DSP_WAV_FORMAT_PCM, (uint16_t)std::atoi(bits_opt.c_str())};
}

int wav_header(WavOut &w, Format f, uint32_t C, uint32_t rate, uint64_t frames) {
    const uint64_t payload = frames * C * (f.bits / 8u);
    w.bytes.resize(64 + payload);
    w.hdr = dsp_wav_write_header(w.bytes.data(), w.bytes.size(), f.fmt, (uint16_t)C, rate, f.bits, frames);
    if (w.hdr < 0) return fail("dsp_wav_write_header", w.hdr);
    w.size = w.hdr + payload;
    return 0;
}

// audio.h:123-133 (interleave)
int queue_wav(const Rows &rows, uint32_t C, uint64_t frames, uint32_t rate, Format f, Device &dev, WavOut &w) {
    const uint64_t payload = frames * C * (f.bits / 8u);
    HIPCK(hipMalloc(&w.d_payload.h, payload + 16));
    if (int st = dsp_wav_encode(rows.ptr.data(), C, frames, f.fmt, f.bits, w.d_payload.h, &dev.ex))
        return fail("dsp_wav_encode", st);
    if (int e = wav_header(w, f, C, rate, frames)) return e;
    HIPCK(hipMemcpyAsync(w.bytes.data() + w.hdr, w.d_payload.h, payload, hipMemcpyDeviceToHost, dev.stream.h));
    return 0;
}
