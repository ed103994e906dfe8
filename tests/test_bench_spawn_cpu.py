"""bench.py's self-spawn path (`python bench.py --gpus N` without a launcher re-executes itself under
torch.distributed.run, the launch line of scripts/grpo_pickscore.sh:7-11): the command it builds starts N ranks that
rendezvous on 127.0.0.1 and see each other.  World size 2 over gloo on the CPU; the stub stands in for the script body."""
import json
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_spawn_command_starts_n_ranks_that_see_each_other(tmp_path):
    import bench
    stub = tmp_path / "stub.py"
    stub.write_text(textwrap.dedent("""
        import argparse, json, os
        import torch, torch.distributed as dist
        ap = argparse.ArgumentParser(); ap.add_argument("--gpus", type=int); ap.add_argument("--steps", type=int)
        a = ap.parse_args()
        world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
        assert world == a.gpus and os.environ["MASTER_ADDR"] == "127.0.0.1" and "LOCAL_RANK" in os.environ
        dist.init_process_group("gloo")
        ones = torch.ones(1); dist.all_reduce(ones)
        if rank == 0:
            print(json.dumps({"ranks_seen": int(ones.item()), "steps": a.steps}))
        dist.destroy_process_group()
    """))
    cmd = bench.spawn_command(["--gpus", "2", "--steps", "5"], 2, script=str(stub))
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nproc-per-node=2" in cmd and "127.0.0.1" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    assert json.loads(line) == {"ranks_seen": 2, "steps": 5}


def test_gpus_gt_1_without_launcher_takes_the_spawn_path(monkeypatch):
    """No WORLD_SIZE in the environment + --gpus 2 -> self_spawn (which refuses politely here: no GPUs), never the old assert."""
    import pytest
    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "GPU(s) visible" in str(e.value)


def test_dump_outputs_keeps_to_the_limit_and_samples_the_same_elements(tmp_path, monkeypatch):
    """--dump-outputs: float32 .npy files, whole when they fit, else a seeded sample that depends on name and shape only."""
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20_000)
    g = torch.Generator().manual_seed(0)
    arrays = {"images": torch.rand(4, 3, 32, 32, generator=g), "log_probs": torch.randn(4, 2, generator=g).to(torch.bfloat16),
              "timesteps": torch.arange(8, dtype=torch.int32).reshape(4, 2).float()}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["images.npy", "log_probs.npy", "timesteps.npy"]
    total = sum((tmp_path / "a" / f).stat().st_size for f in files)
    assert total <= 20_000 + 3 * 256
    lp = np.load(tmp_path / "a" / "log_probs.npy")
    assert lp.dtype == np.float32 and np.array_equal(lp, arrays["log_probs"].float().numpy())
    im_a, im_b = np.load(tmp_path / "a" / "images.npy"), np.load(tmp_path / "b" / "images.npy")
    assert im_a.dtype == np.float32 and im_a.ndim == 1 and 0 < im_a.size < 4 * 3 * 32 * 32
    assert np.array_equal(im_a, im_b) and np.isin(im_a, arrays["images"].numpy().reshape(-1)).all()


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (4, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"
