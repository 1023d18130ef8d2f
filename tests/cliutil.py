"""What the dspbench_render tests (test_cli*.py) share: the binary and how it
is run, a PCM-16 file of seeded noise, a host array on the GPU, the one JSON
line of a run's stdout."""
import json
import os
import subprocess

import numpy as np
import pytest

from wavutil import chunk, wav_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dsp-bench_amd", "dspbench_render")

needs_cli = pytest.mark.skipif(not os.path.exists(CLI), reason="dspbench_render not built")


def run(*args, env=None):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300, env=env)


def pcm16_file(path, channels, L, seed, sr=48000, lo=-32768, hi=32768, edit=None, **image):
    """Write L frames of uniform noise in [lo, hi) as a PCM-16 WAV (`edit`
    changes the interleaved codes in place first, `image` goes to wav_image);
    returns the codes."""
    raw = np.random.default_rng(seed).integers(lo, hi, size=channels * L, dtype=np.int64).astype("<i2")
    if edit is not None:
        edit(raw)
    path.write_bytes(wav_image(raw.tobytes(), fmt=1, channels=channels, bits=16, sr=sr, **image))
    return raw


def cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).cuda()


def json_line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def split_chunks(n_bytes, at):
    """wav_image arguments that store a payload of n_bytes as two data chunks,
    cut at byte `at` (a whole frame), with an odd-sized unrelated chunk (and
    its pad byte) between them."""
    return dict(split_data=[(0, at), (at, n_bytes)], between=chunk(b"LIST", b"abcde"))
