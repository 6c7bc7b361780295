"""bench.py's multi-GPU control flow, executed on the CPU box: `python bench.py --gpus 2 --dry-run-cpu`
goes through respawn_under_torchrun -> torch.distributed.run -> two ranks -> rendezvous (gloo) -> per-rank jobs on the
host-emulated kernels -> bucketed gradient all-reduce during backward -> barrier / max-over-ranks timing -> the weak- and
strong-scaling legs -> ONE JSON line from rank 0.  The numbers mean nothing; that every branch of the 8-GPU run executes does."""
import json
import os
import subprocess
import sys

from helpers import ROOT


def test_two_rank_dry_run_through_the_respawn_path():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
                        "--dry-run-cpu", "--full", "--profile-steps", "0"], capture_output=True, text=True, env=env, timeout=1500)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]            # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 1 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert "DRY RUN" in out["data"] and "DRY RUN" in out["metric"]
    assert out["config"]["parallelism"] == "dp2" and "hostemu" in out["config"]["library"]
    comm = out["communication"]
    assert comm["backend"] == "gloo" and comm["ranks"] == 2
    assert comm["bucketed_steps"] >= 2 and comm["bucket_collectives"] == 3 * comm["bucketed_steps"] and comm["monolithic_steps"] == 0
    assert comm["allreduce_bytes"] > 0 and comm["allreduce_ms"] > 0
    assert len(out["host_enqueue_ms_per_rank"]) == 2 and all(v > 0 for v in out["host_enqueue_ms_per_rank"])
    assert out["variants"]["weak_scaling"]["one_gpu_same_box"] > 0
    assert out["variants"]["strong_scaling_global64"]["global_pairs"] == 4
    assert list(out)[-1] == "summary" and out["summary"]["communication"]["ranks"] == 2
    assert out["value"] > 0 and abs(out["value"] - 2 * 2 * 2 * 1 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]


def test_plain_run_times_only_the_steps_and_dumps_reproducible_outputs(tmp_path):
    """Without --full the line carries the headline alone; --dump-outputs writes the last timed step's results, float32 /
    float64, identical from run to run with the same arguments."""
    import numpy as np
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dumps = []
    for run in range(2):
        d = str(tmp_path / ("run%d" % run))
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--dry-run-cpu", "--dump-outputs", d], capture_output=True, text=True, env=env, timeout=900)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
        assert abs(out["value"] - 2 * 2 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-6 * out["value"]
        assert out["variants"] == {} and out["roofline"] is None and out["breakdown"] is None
        assert out["cpu_baseline"] is None and out["communication"] is None and out["host_enqueue_idle_gpu_ms_per_step"] is None
        z = {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}
        assert sorted(z) == ["bn_buffers", "grads", "loss", "params"]
        assert all(v.dtype in (np.float32, np.float64) and v.size > 0 and np.isfinite(v).all() for v in z.values())
        assert sum(v.nbytes for v in z.values()) <= 64 << 20
        assert float(z["loss"][0]) == out["config"]["final_loss"]
        dumps.append(z)
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
