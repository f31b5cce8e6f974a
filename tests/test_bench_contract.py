"""Static checks of the driver contract that do not need a GPU: bench.py's flags and helper
arithmetic, __graft_entry__'s entry points, the committed profile evidence."""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_flags_and_helpers(monkeypatch):
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert (a.gpus, a.workload, a.engine) == (1, "ped10", "enum") and a.steps >= 1 and a.warmup >= 0
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "3", "--warmup", "1", "--workload", "ped15"])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup, a.workload) == (8, 3, 1, "ped15")
    assert bench.WORKLOADS["ped10"] == (2, 10_000_000) and bench.WORKLOADS["ped5"] == (1, 1_000_000)
    assert bench.fp64_ops_per_site({}, 10) == 59049
    assert 1 <= bench.host_cores() <= (os.cpu_count() or 1)
    assert bench.HBM_PEAK_GBPS == 8000.0


def test_bench_full_and_dump_flags(monkeypatch):
    """A plain run is the headline alone (--full adds the side measurements); --dump-outputs names a directory;
    --steps is the number of timed steps, so it must be at least one."""
    import pytest

    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out_dir"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out_dir"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_cpu_baseline_leg_runs_on_a_tiny_budget():
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    import famseq_amd as fs

    out = bench.cpu_baseline(fs.synthetic_pedigree("ped5"), 1, 0.3, 5)
    assert out["kind"] == "port" and out["unit"] == "sites/s" and out["value"] > 0 and out["cores"] >= 1


def test_graft_entry_points_exist():
    sys.path.insert(0, ROOT)
    g = importlib.import_module("__graft_entry__")
    assert callable(g.build) and callable(g.smoke)


def test_profile_evidence_is_committed():
    prof = os.path.join(ROOT, "profiles")
    rounds = sorted(d for d in os.listdir(prof) if os.path.isdir(os.path.join(prof, d)))
    assert rounds, "no rocprofv3 summaries under profiles/"
    latest = os.path.join(prof, rounds[-1])
    assert any(f.startswith("kernel_stats") for f in os.listdir(latest))
    t = json.load(open(os.path.join(prof, "hbm_traffic_ped10.json")))
    assert t["sites_per_launch"] > 0 and t["bytes_per_launch"] >= t["algorithmic_bytes_per_launch"] * 0.9


def test_bench_launches_ranks_itself_or_says_why_not():
    """`python bench.py --gpus N` as a plain command is the driver's multi-GPU shape: outside
    torch.distributed.run bench.py starts the ranks itself (tests/test_gpu_multi.py runs that on the GPU box).
    Without enough GPUs it must say so before launching anything — not the round-1 "needs a
    torch.distributed.run launch" refusal, and not a hang."""
    import subprocess

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300)
    import torch

    if torch.cuda.device_count() >= 2:
        return  # a real multi-GPU host: the GPU suite covers it
    assert r.returncode != 0 and "GPU(s) visible" in r.stderr and "torch.distributed.run launch" not in r.stderr
    assert r.stdout.strip() == ""


def test_warm_only_builds_the_kernels_without_a_gpu(tmp_path):
    """bench.py --warm-only (what the profiling scripts run before rocprofv3): plan-only contexts, kernels
    found in (or compiled into) the cache, no GPU call."""
    import subprocess

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--warm-only", "--workload", "ped5"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "warm: ped5" in r.stdout and ".hsaco" in r.stdout
