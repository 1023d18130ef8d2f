"""dsp-bench_amd/cli/options.cpp: dspbench_render's command line as data -- the
option table, the rules between options, the --sweep form and the launcher's
environment -- compiled with g++ alone (no HIP, no dspbench header) into
tests/sanitize/cli_options_check.cpp; once more under AddressSanitizer +
UndefinedBehaviorSanitizer (a stand-alone host program).

The program walks a table of argument vectors: every argument error the
test_cli*.py files provoke through the binary (status 2, the message, usage
or not), an accepted vector per mode with every field of Options compared,
--sweep in both orders, a value-less flag first and last, a value missing, an
unknown option, and the rank / world / device / run id defaults with and
without the flags.
"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLI_SRC = os.path.join(os.path.dirname(HERE), "dsp-bench_amd", "cli")


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan_ubsan"])
def test_option_table(tmp_path, san):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the option parser alone"
    exe = str(tmp_path / "cli_options_check")
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O2"]
    r = subprocess.run([gxx, "-std=c++17", "-Wall", *flags, f"-I{CLI_SRC}", f"{HERE}/sanitize/cli_options_check.cpp",
                        f"{CLI_SRC}/options.cpp", "-o", exe], capture_output=True, text=True, timeout=300)
    if san and r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("the compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    m = re.fullmatch(r"checked (\d+), 0 failed\n", r.stdout)
    assert m and int(m.group(1)) == 71, r.stdout      # (the table's size: a case that never ran would pass unseen)
