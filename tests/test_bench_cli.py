"""bench.py's multi-GPU contract rehearsed on CPU: the driver launches it as
``python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`` (one rank per GPU);
here the same command runs N gloo ranks on the CPU and rank 0 must print exactly one JSON line
with the whole-job numbers (n_gpus = N, global batch = N x per-GPU batch, dpN, comm fields)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# the rehearsal is a CPU one wherever it runs: on a GPU machine the ranks would otherwise all open its first GPU
_NO_GPU = {"CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": ""}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("n", [2, 4])
def test_bench_torchrun_json_line(n):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", str(n), "--steps", "1", "--warmup", "1", "--image", "32", "--batch", "2"]
    env = dict(os.environ, OMP_NUM_THREADS="1", **_NO_GPU)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd="/tmp")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["steps"] == 1 and d["warmup"] == 1
    assert d["config"]["global_batch"] == 2 * n and d["config"]["parallelism"] == f"dp{n}"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["dtype"] == "bf16" and d["data"] == "synthetic"
    for k in ("comm_ms", "exposed_comm_ms", "bucket_mb", "buckets", "grad_mb", "backend"):
        assert k in d["config"], k
    assert d["config"]["backend"] == "gloo"


@pytest.mark.parametrize("model,extra", [("resnet50", ["--image", "32"]), ("vgg16", ["--image", "32"]),
                                         ("bert", ["--layers", "1", "--seq", "32"])])
def test_bench_torchrun_n8_every_dp_config(model, extra):
    """The driver's N=8 launch, rehearsed with 8 gloo ranks for each BASELINE.json DP config
    (tiny shapes): one JSON line, whole-job value, dp8, bucket / comm fields; bf16 wire for bert."""
    n = 8
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
           "--model", model, "--gpus", str(n), "--steps", "1", "--warmup", "1", "--batch", "2", "--full", *extra]
    if model == "bert":
        cmd += ["--reduce-dtype", "bf16"]
    env = dict(os.environ, OMP_NUM_THREADS="1", **_NO_GPU)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd="/tmp")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["config"]["parallelism"] == "dp8" and d["config"]["global_batch"] == 2 * n
    assert d["value"] > 0 and d["config"]["buckets"] >= 1 and d["config"]["backend"] == "gloo"
    assert d["config"]["comm_ms"] is not None  # --full: the stand-alone all-reduce measurement ran
    if model == "bert":
        assert d["config"]["reduce_dtype"] == "bf16" and d["config"]["bf16_algo"] == "a2a"
        assert d["unit"] == "tokens/sec"


def _dump_run(d, env, extra):
    """One ``bench.py --gpus 1 ... --dump-outputs d`` run: the result line and the arrays it wrote (checked to be
    ``loss.npy`` and ``weight_norms.npy``, finite float32, far below the 64 MB limit, the loss of the result line)."""
    import numpy as np

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *extra, "--dump-outputs", str(d)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=str(d.parent))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == int(extra[extra.index("--steps") + 1]) and res["ms_per_step"] > 0
    assert sorted(p.name for p in d.iterdir()) == ["loss.npy", "weight_norms.npy"]
    arrs = {p.stem: np.load(p) for p in d.iterdir()}
    assert all(a.dtype == np.float32 and a.ndim == 1 and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert arrs["loss"].shape == (1,) and abs(float(arrs["loss"][0]) - res["config"]["final_loss"]) < 1e-3
    assert arrs["weight_norms"].size > 50  # one norm per convolution / Dense kernel and BatchNorm scale
    return res, arrs


def test_bench_dump_outputs_cpu(tmp_path):
    """``--dump-outputs`` on the CPU (one thread, so a fixed summation order): two runs with the same arguments
    get the same inputs and write the same arrays; a run with one timed step less ends on another batch and
    another update, so both arrays differ: they are the LAST timed step's."""
    import numpy as np

    env = dict(os.environ, OMP_NUM_THREADS="1", **_NO_GPU)
    shape = ["--warmup", "1", "--image", "32", "--batch", "2"]
    _, a = _dump_run(tmp_path / "a", env, ["--steps", "3", *shape])
    _, b = _dump_run(tmp_path / "b", env, ["--steps", "3", *shape])
    _, c = _dump_run(tmp_path / "c", env, ["--steps", "2", *shape])
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert not np.array_equal(a[k], c[k]), k


@pytest.mark.gpu
def test_bench_dump_outputs_gpu_default_kernels(tmp_path):
    """``--dump-outputs`` on the GPU, small ResNet-50, in the default mode (fp32-atomic reductions; two eager
    steps, the hipGraph capture and replays, models/step.py): the dump does not change the mode, and two runs
    agree in the loss to rounding.  The last timed step starts from the seeded initial weights (bench.py
    rewind_state), so its loss is one forward pass of fixed weights on a fixed batch.  Bound: the logits are
    bf16 (8-bit significand, unit roundoff 2^-8); another summation order of the statistics can flip such
    roundings, and each of the two runs may sit one rounding off the exact value, so the losses agree within
    2 * 2^-8 relative.  (With an SGD update at lr 0.1 between the rewind and the loss no such argument holds:
    at this small shape the update throws the loss from 7 to 11 and two runs were seen 5 % apart.)"""
    env = dict(os.environ)
    env.pop("DDL_DETERMINISTIC", None)
    args = ["--steps", "3", "--warmup", "3", "--image", "64", "--batch", "128"]
    ra, a = _dump_run(tmp_path / "a", env, args)
    rb, b = _dump_run(tmp_path / "b", env, args)
    assert "deterministic" not in ra["config"]
    la, lb = float(a["loss"][0]), float(b["loss"][0])
    print(f"loss {la!r} vs {lb!r}; weight norms max rel diff "
          f"{float((abs(a['weight_norms'] - b['weight_norms']) / (abs(a['weight_norms']) + 1e-12)).max()):.3e}")
    assert abs(la - lb) <= 2 * 2.0 ** -8 * abs(la), (la, lb)
