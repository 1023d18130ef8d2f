"""The frame-reuse flag and result bit: the Python binding's constants equal
the header's, and the flag is one of the method flags the chunked and sharded
drivers pass on to every chunk."""
import os
import re

import dspbench._lib as L

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dspbench",
                      "dspbench.h")


def header_text():
    with open(HEADER) as f:
        return f.read()


def define(text, name):
    m = re.search(r"^#define\s+" + name + r"\s+(0x[0-9a-fA-F]+)u\b", text, re.M)
    assert m, name
    return int(m.group(1), 16)


def test_constants_match_the_header():
    t = header_text()
    assert L.DSP_EXEC_EVERY_FRAME == define(t, "DSP_EXEC_EVERY_FRAME") == 0x40
    assert L.DSP_RESULT_FRAME_REUSE == define(t, "DSP_RESULT_FRAME_REUSE") == 0x8
    m = re.search(r"DSP_DEBUG_FRAME_RUN\s*=\s*(\d+)", t)
    assert m and int(m.group(1)) == L.DSP_DEBUG_FRAME_RUN


def test_flag_is_a_method_flag():
    t = header_text()
    m = re.search(r"^#define\s+DSP_EXEC_METHOD_FLAGS\s*\\\n((?:.*\\\n)*.*)$", t, re.M)
    assert m
    names = re.findall(r"DSP_EXEC_[A-Z_]+", m.group(1))
    assert "DSP_EXEC_EVERY_FRAME" in names
    value = 0
    for n in names:
        value |= define(t, n)
    assert value == L.DSP_EXEC_METHOD_FLAGS
    assert L.DSP_EXEC_METHOD_FLAGS & L.DSP_EXEC_EVERY_FRAME
    # no method flag collides with a buffer / sync flag
    assert not (L.DSP_EXEC_METHOD_FLAGS & (L.DSP_EXEC_HOST_BUFFERS | L.DSP_EXEC_SYNC))
