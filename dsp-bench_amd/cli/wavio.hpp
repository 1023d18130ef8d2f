// WAV files to device rows and back, once each (every function returns the
// process's exit status: 0, or what to return after the message it printed).
#pragma once

#include <functional>
#include <initializer_list>
#include <string>
#include <utility>

#include "device.hpp"
#include "dspbench/wav.h"

bool read_file(const char *path, std::vector<unsigned char> &out);
// the pieces, in order, as the file at `path` ("cannot write" otherwise)
int write_file(const char *path, std::initializer_list<std::pair<const void *, size_t>> pieces);

// ---- WAV file -> device rows ------------------------------------------------
struct Wav {
    dsp_wav_info info{};
    std::vector<unsigned char> payload;  // the data chunks, concatenated
    DevBuf d_payload;
    Rows rows;  // info.channels rows of info.frames floats
};
// Read and parse `path` (`role`: what follows "dsp_wav_parse" in a message,
// "" for the input), let `limits` refuse the header (non-zero: the status,
// its message printed), open the device if nothing has yet, then payload to
// HBM and dsp_wav_decode on the stream.
int load_wav(const char *path, const char *role, const std::function<int(const dsp_wav_info &)> &limits, Device &dev,
             Wav &w);

// rows[0 .. C) of L frames at `from` Hz -> the same rows at `to` Hz, L the new
// length (--rate); `limits` sees that length before anything is allocated
int resample_rows(Rows &rows, uint32_t C, uint64_t &L, uint32_t from, uint32_t to, const char *role,
                  const std::function<int(uint64_t)> &limits, Device &dev);

// ---- device rows -> WAV file ------------------------------------------------
struct Format {
    uint16_t fmt, bits;
};
Format resolve_bits(const std::string &bits_opt, Format otherwise);  // --bits 16|24|32|float over a default

struct WavOut {
    std::vector<unsigned char> bytes;  // header + payload; `size` of it is the file
    int hdr = 0;
    size_t size = 0;
    DevBuf d_payload;
};
int wav_header(WavOut &w, Format f, uint32_t C, uint32_t rate, uint64_t frames);
// encode on the stream and queue the payload's copy into w.bytes: the file is
// whole after the caller's next synchronise, then write_file
int queue_wav(const Rows &rows, uint32_t C, uint64_t frames, uint32_t rate, Format f, Device &dev, WavOut &w);
