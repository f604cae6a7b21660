"""bench.py --gpus N without torch.distributed.run's environment starts the ranks itself
(a child `torch.distributed.run` process; no GPU touched before it) and returns the child's
exit status.  CPU: --launch-probe ranks report their environment and exit.  GPU: one plain
run of the smallest config (what the line holds without --full, --dump-outputs)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env,
                          capture_output=True, text=True, timeout=240)


@pytest.mark.slow
def test_gpus_n_self_launches_n_ranks():
    r = _run("--gpus", "3", "--launch-probe")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert sorted(d["rank"] for d in lines) == [0, 1, 2]
    assert all(d["world"] == 3 and d["master"] == "127.0.0.1" for d in lines)
    assert sorted(d["local_rank"] for d in lines) == [0, 1, 2]


@pytest.mark.slow
def test_child_failure_propagates_nonzero_status():
    r = _run("--gpus", "2", "--launch-probe", "--config", "no-such-config")
    assert r.returncode != 0


def test_emulate_flags_validated_before_any_gpu_call():
    r = _run("--emulate-world", "8", "--emulate-rank", "9")
    assert r.returncode == 2 and "emulate" in r.stderr


FULL_ONLY = ("roofline", "embedding_roofline", "interaction_roofline", "kernel_us_per_step",
             "box_calibration", "input_pipeline", "skew_zipf", "comm", "cpu_baseline")


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps, reports ms_per_step, measures
    nothing else, and --dump-outputs writes the last step's arrays as float32/float64 .npy
    (C1 shape: the smallest config)."""
    import numpy as np
    out = tmp_path / "dump"
    r = _run("--gpus", "1", "--config", "small", "--steps", "3", "--warmup", "1",
             "--preheat-ms", "0", "--dump-outputs", str(out))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - 2048 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    assert all(d.get(k) is None for k in FULL_ONLY) and "gpu_over_cpu" not in d
    files = {p.name: np.load(p) for p in out.iterdir()}
    assert {"prob.npy", "loss.npy", "dense_W0.npy", "dense_b0.npy", "emb_rows_sample.npy",
            "emb_rows_last_batch.npy"} <= set(files)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    total = sum(a.nbytes for a in files.values())
    assert total == d["dumped_output_bytes"] <= 64 << 20
    assert files["prob.npy"].shape == (2048,) and files["loss.npy"].shape == (1,)
    assert all(np.isfinite(a).all() for a in files.values())
    assert float(files["loss.npy"][0]) == pytest.approx(d["loss_last"], rel=1e-6)
    # the sampled rows are the rows the index arrays name
    assert files["emb_rows_sample.npy"].shape == (len(files["emb_rows_sample_index.npy"]), 64)
    assert files["emb_rows_last_batch.npy"].shape == \
        (len(files["emb_rows_last_batch_index.npy"]), 64)
