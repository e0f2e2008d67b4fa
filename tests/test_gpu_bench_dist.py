"""bench.py's own multi-rank path, executed: `torch.distributed.run
--nproc-per-node 2 bench.py --gpus 2` as the driver launches it for the
scaling runs, on the box's one GPU (both ranks on cuda:0 over gloo: RCCL
cannot place two ranks on one device; SEL_BENCH_BACKEND / SEL_BENCH_SHARE_GPU
are rehearsal knobs, the driver's runs use RCCL with one rank per GPU).

Covers what only the N > 1 bench runs: the DDP-wrapped generator with the
frozen quantizer / decoder, the batch-global add_noise exchange, the
barrier + max-over-ranks step timing, the rank-0 JSON line (n_gpus, weak
scaling, whole-job value), for C3 and for C5 (GAN step with both modules
DDP-wrapped and the concurrent sub-discriminator chains).  The launcher is a
child process; the pytest process never execs.

Also the plain one-GPU command line (no --full) with --dump-outputs, at a
small batch."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("cfg", ["c3", "c5"])
def test_bench_two_ranks(cfg, tmp_path):
    env = dict(os.environ, SEL_BENCH_BACKEND="gloo", SEL_BENCH_SHARE_GPU="1",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.join(REPO, "bench.py"),
           "--gpus", "2", "--config", cfg, "--steps", "2", "--warmup", "1", "--batch", "4",
           "--full", "--no-cpu-baseline", "--no-fp32-companion"]  # --full: the per-launch roofline under two ranks
    log = tmp_path / "bench.log"
    with open(log, "w") as f:
        rc = subprocess.call(cmd, cwd=REPO, env=env, stdout=f, stderr=subprocess.STDOUT, timeout=280)
    text = log.read_text()
    assert rc == 0, text[-3000:]
    lines = [ln for ln in text.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, text[-3000:]  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0, d
    assert d["config"]["global_batch"] == 8 and d["config"]["parallelism"] == "dp2", d["config"]
    assert d["full"] is True and d["roofline"]["kernel"] and d["ms_per_step"] > 0, d


def test_bench_plain_run_dumps_its_last_step(tmp_path):
    """A plain one-GPU run does its steps only (the --full legs are null in the
    result line) and --dump-outputs leaves the last step's trained parameters,
    their gradients and the loss totals as finite float .npy files."""
    import numpy as np
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", "4", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["full"] is False, d
    assert d["dtype"] == "bf16" and d["unit"] == "frames/s" and d["higher_is_better"] is True, d
    assert all(d[k] is None for k in ("roofline", "cpu_baseline", "fp32_companion", "stft_kernel")), d
    files = sorted(os.listdir(out))
    params = [f for f in files if f.startswith("param.generator.encoder.")]
    assert params and all("grad." + f[len("param."):] in files for f in params), files
    assert "loss_total.train.generator_loss.npy" in files and not any(".decoder." in f for f in files), files
    total = 0
    for f in files:
        a = np.load(out / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        total += a.nbytes
    assert 0 < total <= 64 << 20
    # the step really trained: some gradient is non-zero
    assert any(np.abs(np.load(out / f)).max() > 0 for f in files if f.startswith("grad."))
