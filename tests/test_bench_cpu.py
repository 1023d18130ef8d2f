"""bench.py's host-side helpers (CPU): the PMC traffic figure applies only to
a launch of the profiled size, and every workload with an instantiation
names a committed summary."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


HEADLINE_BYTES = 2 * 42186 * (4 * 4096 + 4 * 4097)  # C * F * (4H + 4K), 1 h stereo at 48 kHz


def test_pmc_traffic_of_the_profiled_launch(bench):
    t, src, inst = bench.pmc_traffic("headline", HEADLINE_BYTES)
    assert t is not None and src.startswith("profiles/") and inst
    assert 0.99 < t / HEADLINE_BYTES < 1.01


def test_pmc_traffic_refuses_another_size(bench):
    # a 5-minute run (one twelfth of the bytes) must not borrow the 1 h launch's figure
    t, src, inst = bench.pmc_traffic("headline", HEADLINE_BYTES / 12)
    assert t is None and "another size" in src and inst


def test_every_instantiation_has_a_summary(bench):
    for wl, inst in bench.PK_INST.items():
        _, src, got = bench.pmc_traffic(wl, 0)  # size 0: no figure, but the summary is found
        assert got == inst
        assert src is not None, f"{wl}: no committed PMC summary names {inst}"


def test_headline_plugin_defaults_to_the_source(bench, monkeypatch):
    # the headline measures IR_test.cpp compiled unchanged unless --ir-plugin enum
    monkeypatch.setattr("sys.argv", ["bench.py"])
    assert bench.parse().ir_plugin == "source"
    monkeypatch.setattr("sys.argv", ["bench.py", "--ir-plugin", "enum"])
    assert bench.parse().ir_plugin == "enum"
    name = bench.source_plugin_name("IR_test", "table")
    assert "IR_test.cpp" in name and "compiled unchanged" in name and "table" in name


def test_plain_run_is_the_default_and_full_is_an_option(bench, monkeypatch):
    # the passes beside the timed steps (distribution, companion, end to end, CPU baseline) need --full
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(bench, monkeypatch, tmp_path):
    """A small array is written whole; a large one as head, tail and a seeded
    sample, within the budget, float32, and the same from call to call."""
    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2 * 4 * 3000)  # 3000 floats per array
    small = torch.arange(2 * 500, dtype=torch.float32).reshape(2, 500)
    big = torch.arange(2 * 50 * 41, dtype=torch.float64).reshape(2, 50, 41)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"out": small, "mag": big, "none": None})
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["mag_head.npy", "mag_sample.npy", "mag_tail.npy", "out.npy"]
    got = {n: np.load(tmp_path / "a" / n) for n in names}
    assert all(v.dtype == np.float32 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 2 * 4 * 3000
    assert np.array_equal(got["out.npy"], small.numpy())
    n = got["mag_head.npy"].shape[1]
    assert n == 1000 // (2 * 41) and got["mag_head.npy"].shape == (2, n, 41)
    assert np.array_equal(got["mag_head.npy"], big[:, :n].numpy().astype(np.float32))
    assert np.array_equal(got["mag_tail.npy"], big[:, 50 - n:].numpy().astype(np.float32))
    flat = np.random.default_rng(bench.DUMP_SEED).integers(0, big.numel(), 1000)
    assert np.array_equal(got["mag_sample.npy"], big.reshape(-1).numpy()[flat].astype(np.float32))
    for nme in names:
        assert np.array_equal(np.load(tmp_path / "b" / nme), got[nme])
    # at N > 1 every rank writes its own files, within its share
    bench.dump_outputs(str(tmp_path / "c"), {"out": small}, world=2, rank=1)
    assert [p.name for p in (tmp_path / "c").iterdir()] == ["out_rank1.npy"]


def test_gpus_flag_launches_or_checks_the_world(bench):
    """--gpus N: unlaunched N > 1 starts N ranks (torch.distributed.run as a
    child, rendezvous on 127.0.0.1); under a launcher WORLD_SIZE must equal
    N; N = 1 unlaunched runs in place."""
    assert bench.check_world(1, {}) == ("run", None)
    assert bench.check_world(8, {}) == ("launch", None)
    assert bench.check_world(8, {"WORLD_SIZE": "8"}) == ("run", None)
    what, why = bench.check_world(8, {"WORLD_SIZE": "2"})
    assert what == "error" and "WORLD_SIZE=2" in why
    assert bench.check_world(0, {})[0] == "error"
    cmd = bench.rank_launch_cmd(4, ["--gpus", "4", "--steps", "5"])
    i = cmd.index("--nproc-per-node")
    assert cmd[i + 1] == "4" and "torch.distributed.run" in cmd
    assert "127.0.0.1:0" in cmd
    assert cmd[-5].endswith("bench.py") and cmd[-4:] == ["--gpus", "4", "--steps", "5"]


def test_world_mismatch_exits_nonzero():
    import subprocess
    import sys
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stderr


def test_gather_watchdog_prints_the_line_and_fails(bench):
    """A gather pass that never finishes: the watchdog prints the line (with
    the error) and exits with a non-zero status, so a hung gather shows in
    the run's rc."""
    import threading
    done = threading.Event()
    got = {}

    def emit(ms, err):
        got["line"] = (ms, err)

    def fake_exit(rc):
        got["rc"] = rc
        done.set()
    bench.start_gather_watchdog(0.05, 0, emit, exit_fn=fake_exit)
    assert done.wait(5.0)
    assert got["rc"] == bench.GATHER_TIMEOUT_RC != 0
    assert got["line"][0] is None and "timed out" in got["line"][1]


def test_gather_watchdog_cancelled_in_time(bench):
    called = []
    dog = bench.start_gather_watchdog(0.5, 0, lambda *a: called.append(a), exit_fn=lambda rc: called.append(rc))
    dog.cancel()
    import time
    time.sleep(0.7)
    assert called == []
