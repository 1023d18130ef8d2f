"""csrc/module_policy.cpp: what the speculative segments of a State-writing
plugin learn from their counters (SegLearner), how a render's levels and
geometry are planned, and how a stateless callback's probe results classify --
plain C++ over counters and float arrays, compiled with g++ alone (no HIP)
into tests/sanitize/module_policy_check.cpp; once more under AddressSanitizer
+ UndefinedBehaviorSanitizer (a stand-alone host program).

Every learner case is 1024 segments of 8 blocks after begin(): a render
guesses the first State of 1023 segments, less those whose whole history the
warm-up covers (warm / 8), and a level fails when more than 1/8 of the guessed
ones started wrong.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "dsp-bench_amd", "csrc")

NONE, TABLE, GAIN, GAIN_TABLE = 0, 1, 2, 3


def run_check(tmp, san):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the module policy alone"
    exe = str(tmp / ("module_policy_check" + ("_san" if san else "")))
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O2"]
    r = subprocess.run([gxx, "-std=c++17", "-Wall", *flags, f"-I{CSRC}", f"-I{REPO}/include",
                        f"{HERE}/sanitize/module_policy_check.cpp", f"{CSRC}/module_policy.cpp", "-o", exe],
                       capture_output=True, text=True, timeout=300)
    if san and r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("the compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return dict(ln.split() for ln in r.stdout.splitlines())


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def figures(request, tmp_path_factory):
    return run_check(tmp_path_factory.mktemp("module_policy"), request.param)


def learnt(figures, tag):
    keys = ("warm", "one_level", "off", "chain_bad", "bumps")
    return tuple(int(figures[f"{tag}_{k}"]) for k in keys)


def last(figures, tag):
    return tuple(int(figures[f"{tag}_last_{k}"]) for k in ("used", "levels", "warmup", "chain"))


def test_begin_starts_with_the_first_warm_up(figures):
    assert (figures["begin_warm"], figures["begin_gen"]) == ("4", "1")


def test_first_level_sufficed(figures):
    """A: three levels launched, level 1 never ran and no segment differed."""
    assert learnt(figures, "A") == (4, 1, 0, 0, 0)
    assert last(figures, "A") == (1, 1, 4, 0)


def test_second_level_stood(figures):
    """B: level 1 (64 blocks) ran and 10 segments differed: 8 early segments,
    1015 guessed, 80 <= 1015."""
    assert learnt(figures, "B") == (64, 0, 0, 0, 0)
    assert last(figures, "B") == (1, 2, 64, 0)


def test_last_level_failed(figures):
    """C: levels 1 and 2 ran, 200 differed at 1024 blocks: 128 early, 895
    guessed, 1600 > 895 -- the chain does not forget (warm is left alone)."""
    assert learnt(figures, "C") == (4, 0, 1, 0, 0)
    assert last(figures, "C") == (1, 3, 1024, 0)


def test_one_level_renders_bump_the_warm_up_twice(figures):
    """D: after A, each render plans two levels and is marked as such; 3
    segments missed each time: one block longer, at most twice."""
    for i in range(3):
        assert (figures[f"D{i}_levels"], figures[f"D{i}_slot_one"]) == ("2", "1")
    assert [int(figures[f"D{i}_warm"]) for i in range(3)] == [5, 6, 6]
    assert learnt(figures, "D") == (6, 1, 0, 0, 2)


def test_a_render_from_an_older_warm_up_teaches_nothing(figures):
    """Two renders launched with warm 4: the first landing makes it 5, the
    second (the newest call: it is what is reported) changes nothing."""
    assert figures["Dstale_first_warm"] == "5"
    assert (figures["Dstale_warm"], figures["Dstale_bumps"], figures["Dstale_last_warmup"]) == ("5", "1", "4")


def test_one_level_is_unlearnt_when_the_second_level_ran(figures):
    """E."""
    assert learnt(figures, "E") == (4, 0, 0, 0, 0)
    assert last(figures, "E") == (1, 2, 64, 0)


def test_other_parameters_before_the_landing(figures):
    """F: B's counters land after begin() with other Parameters: nothing
    learnt (warm stays 4), yet the render is the one reported."""
    assert figures["F_gen_bumped"] == "1"
    assert learnt(figures, "F") == (4, 0, 0, 0, 0)
    assert last(figures, "F") == (1, 2, 64, 0)


def test_begin_resets_on_parameters_or_shape_only(figures):
    assert (figures["Fsame_one_level"], figures["Fsame_gen_kept"]) == ("1", "1")
    assert (figures["FC_one_level"], figures["FC_gen_bumped"], figures["FC_warm"]) == ("0", "1", "4")
    assert (figures["FB_one_level"], figures["FB_gen_bumped"]) == ("0", "1")
    assert figures["Fsize_gen_bumped"] == "1"


@pytest.mark.parametrize("tag", ["Gm", "Gr"])
def test_chain_records_that_fail_their_check(figures, tag):
    """G: the State chain alone (no level), CHAIN_MISMATCH or CHAIN_RECORDS
    set: these Parameters render serially from now on."""
    assert learnt(figures, tag) == (4, 0, 1, 1, 0)
    assert last(figures, tag) == (1, 0, 0, 1)


def test_chain_records_that_pass(figures):
    assert learnt(figures, "Gok") == (4, 0, 0, 0, 0)
    assert last(figures, "Gok") == (1, 0, 0, 1)


def test_slots_and_landing_order(figures):
    """H: the first two launches fill slots 0 and 1, the third takes the
    older one; landings are visited oldest first."""
    assert figures["H_slots"] == "01"
    assert figures["H_order"] == "01"
    assert figures["H_third"] == "0"
    assert figures["H_order_after"] == "10"
    assert figures["H_pending"] == "11"


def test_levels(figures):
    """x16 each up to 4096, shorter than half the file; with a State chain, a
    level's warm-up plus a segment within 1/16 of the file; two levels once
    the first is known to suffice."""
    assert figures["levels_long"] == "4,64,1024,4096"
    assert figures["levels_long_one"] == "4,64"
    assert figures["levels_chain"] == "4,64"       # 16 (1024 + 8) > 10000
    assert figures["levels_short"] == "4"          # 2 * 64 >= 100
    assert figures["levels_max"] == "4096"


def geometry(figures, tag):
    return tuple(int(figures[f"{tag}_{k}"]) for k in ("ok", "seg", "K"))


def test_geometry(figures):
    assert geometry(figures, "geo_min_seg") == (1, 4, 25)         # never fewer than 4 blocks
    assert geometry(figures, "geo_large") == (1, 1000, 1000)
    assert geometry(figures, "geo_one_segment")[0] == 0           # K < 2
    assert geometry(figures, "geo_2p32")[0] == 0                  # block indices in 32 bits
    assert geometry(figures, "geo_below_2p32")[0] == 1
    assert geometry(figures, "geo_8gib")[0] == 1                  # 2^23 States of 1024 bytes: 8 GiB
    assert geometry(figures, "geo_over_8gib")[0] == 0             # one more


def test_probes(figures):
    assert figures["probes_size"] == str(5 * 2 * 8)
    assert figures["probes_zeros_in_noise"] == "0"
    assert figures["probes_first_is_one"] == "2"
    assert figures["probes_negative_zero"] == "1"
    assert (figures["probes_zero_probe"], figures["probes_ones_probe"]) == ("1", "1")


def test_classify(figures):
    kind = lambda name: int(figures["class_" + name])
    assert kind("table") == TABLE
    assert kind("table_not_proved") == NONE
    assert kind("table_channel_differs") == NONE
    assert kind("gain") == GAIN and float(figures["class_gain_value"]) == 0.5
    assert kind("gain_no_g") == NONE
    assert kind("gain_table_allowed") == GAIN      # not one row: no table, the next class
    assert kind("gain_twice") == NONE              # the ones probe rendered g^2 in one element
    assert kind("gain_table") == GAIN_TABLE
    assert kind("gain_table_not_proved") == NONE
    assert kind("zero_block") == TABLE             # also x * 0: the table comes first


def test_affine_ramp(figures):
    assert (figures["ramp_found"], figures["ramp_g0_exact"], figures["ramp_s_exact"]) == ("1", "1", "1")
    assert figures["ramp_one_ulp_off"] == "0"
    assert (figures["ramp_subnormal_input"], figures["ramp_subnormal"]) == ("1", "0")
    assert (figures["ramp_b1"], float(figures["ramp_b1_g0"]), float(figures["ramp_b1_s"])) == ("1", 0.75, 0.0)
    assert figures["ramp_inf"] == "0"
