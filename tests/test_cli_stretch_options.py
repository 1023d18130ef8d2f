"""dsp-bench_amd/cli/options.cpp over --stretch, --pitch and --stretch-hop: the
option parser compiled with g++ alone (no HIP, no dspbench header) into
tests/sanitize/cli_stretch_options_check.cpp; once more under AddressSanitizer +
UndefinedBehaviorSanitizer (a stand-alone host program).  The program walks a
table of argument vectors: what the three options parse to, alone and beside
the levels, --rate, --psd and --convolve, and every refusal with its message:
--deconvolve and --transfer (named), --decay, --stft, --loop, the multi-GPU
modes, both at once, values out of range, not numbers or missing, and
--stretch-hop alone or outside 512 .. 8192."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLI_SRC = os.path.join(os.path.dirname(HERE), "dsp-bench_amd", "cli")


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_stretch_option_table(tmp_path, san):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the option parser alone"
    exe = str(tmp_path / "cli_stretch_options_check")
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O2"]
    if san:
        # whether the compiler has the sanitizers' runtime: a trivial program, so that an
        # error in the check program itself fails below instead of skipping
        probe = tmp_path / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        r = subprocess.run([gxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True,
                           timeout=300)
        if r.returncode != 0:
            pytest.skip("the compiler has no sanitizer runtime")
    r = subprocess.run([gxx, "-std=c++17", "-Wall", *flags, f"-I{CLI_SRC}", f"{HERE}/sanitize/cli_stretch_options_check.cpp",
                        f"{CLI_SRC}/options.cpp", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    m = re.fullmatch(r"checked (\d+), 0 failed\n", r.stdout)
    assert m and int(m.group(1)) == 39, r.stdout      # (the table's size: a case that never ran would pass unseen)
