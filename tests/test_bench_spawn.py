"""CPU: `python bench.py --gpus N` without a launcher starts N rank processes itself — before the parent imports
torch or touches a GPU — with the rendezvous environment the contract names, and returns the worst exit code."""
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_gpus_n_spawns_ranks_with_the_rendezvous_environment():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HIP_VISIBLE_DEVICES"] = "-1"                              # no device visible, even where a GPU is present
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300, env=env)
    # no GPU: every rank must stop with the no-device message (a loud failure, never a CPU fallback), and the parent
    # returns their exit code rather than failing itself ...
    assert out.returncode == 1 and "Traceback" not in out.stderr, out.stderr[-2000:]
    assert out.stderr.count("bench.py needs an MI355X") == 3, out.stderr[-2000:]
    assert "torch.distributed.run" not in out.stderr              # ... and nobody asks for an external launcher any more


def test_spawn_ranks_environment(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    seen = []

    class P:
        def __init__(self, cmd, env=None):
            seen.append((cmd, env))

        def poll(self):
            return 0

        def wait(self):
            return 0

    import subprocess as sp
    monkeypatch.setattr(sp, "Popen", P)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    assert bench.spawn_ranks(4) == 0
    assert len(seen) == 4
    ports = {e["MASTER_PORT"] for _, e in seen}
    assert len(ports) == 1
    for r, (cmd, e) in enumerate(seen):
        assert cmd[0] == sys.executable and cmd[1].endswith("bench.py") and cmd[2:] == ["--gpus", "4", "--steps", "3"]
        assert e["RANK"] == e["LOCAL_RANK"] == str(r) and e["WORLD_SIZE"] == "4" and e["MASTER_ADDR"] == "127.0.0.1"
        assert e["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_launcher_world_size_must_match():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True, text=True,
                         timeout=300, env=env)
    assert out.returncode != 0 and "--gpus 4 but the launcher started 2" in out.stderr


def test_cpu_baseline_child_reports_its_phases(tmp_path):
    """bench.py's CPU baseline runs in a child process (no torch, no GPU): one JSON line per sample and a wall-clock line per
    phase in the log, so that a run that is cut short still says where the time went."""
    import json
    log = tmp_path / "phases.log"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-baseline-child", "96,160", "--cpu-iters", "3",
                          "--cpu-threads", "2", "--cpu-log", str(log)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert [d["sample"] for d in lines] == [96, 160]
    for d in lines:
        assert d["iters"] == 3 and d["value"] > 0 and d["index_type"] == "int" and d["kind"] in ("reference", "port")
        assert set(d["phases_s"]) >= {"warm", "generator", "rhs"}
    text = log.read_text()
    for what in ("warm (first touch", "generator (closed form", "b = A x_true", "gaussSeidel, 3 sweeps"):
        assert text.count(what) == 2, what


def test_the_headline_system_needs_the_wide_index_type():
    sys.path.insert(0, ROOT)
    import bench
    assert not bench.cpu_needs_wide_index(4096) and not bench.cpu_needs_wide_index(14336)
    assert bench.cpu_needs_wide_index(16384)                   # 5 x 16384^2 > 2^30: getNearestIndex's (end + idx) / 2 overflows int
    assert 50.0 < bench.cpu_system_gb(16384) < 70.0


def test_dump_plan_is_fixed_by_the_shape_and_stays_within_64_mb():
    """--dump-outputs samples the iterate at positions that depend on the shape alone (two runs, two builds: the same
    pixels), always holding the first and last row, and never writes more than 64 MB whatever the shape."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    for W, H, C in ((16384, 16384, 1), (4096, 4096, 3), (2048, 1536, 1), (1, 1, 1), (10 ** 7, 3, 3), (64, 2 * 10 ** 6, 3)):
        rows, cols, band = bench.dump_plan(W, H, C)
        again = bench.dump_plan(W, H, C)
        assert np.array_equal(rows, again[0]) and np.array_equal(cols, again[1]) and band == again[2]
        assert rows[0] == 0 and rows[-1] == H - 1 and np.all(np.diff(rows) > 0) and np.all(np.diff(cols) > 0)
        assert 0 <= cols[0] and cols[-1] < W
        assert 8 * C * (len(rows) * len(cols) + -(-H // band)) <= 64 << 20, (W, H, C)
    rows, cols, _ = bench.dump_plan(16384, 16384, 1)
    assert len(cols) == 16384 and len(rows) >= 256                # the headline shape: whole rows, hundreds of them


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode != 0 and "--steps must be >= 1" in out.stderr


def test_cpu_baseline_child_skips_what_the_c_oracle_cannot_sweep(tmp_path):
    """Without the compiled reference (oracle/_ref) the baseline is the C oracle, whose int positions overflow past 2^30
    entries: the child must skip such a size at once, with a line in the log, instead of sweeping it."""
    sys.path.insert(0, ROOT)
    import oracle
    import pytest
    try:
        oracle.Ref()
        pytest.skip("oracle/_ref is built here: the 64-bit reference sweep takes this size")
    except (FileNotFoundError, OSError):
        pass
    log = tmp_path / "phases.log"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-baseline-child", "16384", "--cpu-log", str(log)],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert "16384^2 skipped" in log.read_text() and "oracle/_ref" in log.read_text()
