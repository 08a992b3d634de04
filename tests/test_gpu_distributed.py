"""Row-sharded solve with two and three processes on a GPU box (the N > 1 path of bench.py), through the C ABI."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _run(cmd, env, timeout):
    """a child process with a time limit, started a second time if the first one ran into it: N workers of torch.distributed.run on ONE
    device over gloo hung once in ~20 runs of this file in round 6 (16 s otherwise; never reproduced in isolation) -- a launcher that hangs
    twice in a row is a failure, one that hangs once must not take the whole suite's time limit with it"""
    import signal
    for attempt in (0, 1):
        pr = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
        try:
            out, err = pr.communicate(timeout=timeout)
            return subprocess.CompletedProcess(cmd, pr.returncode, out, err)
        except subprocess.TimeoutExpired:
            os.killpg(pr.pid, signal.SIGKILL)             # (the launcher AND its workers: exactly the process group started here)
            pr.communicate()
            if attempt:
                raise


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 3])              # 3: the row split leaves a remainder on the last rank
def test_ranks_share_one_gpu(nproc):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(29575 + nproc), str(ROOT / "tests" / "dist_gpu_worker.py")]
    r = _run(cmd, env, 300)
    assert "DIST_GPU_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.gpu
def test_rccl_collectives_at_world_size_one():
    """RCCL itself, on a one-GPU box: process group "nccl" of world size 1 and OEM_FORCE_COLLECTIVES=1 make every collective of
    oem_amd/distributed.py execute (tests/rccl_world1_worker.py counts them) -- with the bits of the plain call."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29631", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = _run([sys.executable, str(ROOT / "tests" / "rccl_world1_worker.py")], env, 300)
    assert "RCCL_W1_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.gpu
def test_bench_launches_its_own_workers():
    """`python bench.py --gpus 2` without a torchrun environment: the parent starts the two workers itself (here both on the one
    GPU of the box, over gloo: OEM_BENCH_ONE_DEVICE) and the one JSON line comes back through it."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(OEM_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = _run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--n", "200000", "--full", "--no-c5", "--no-cpu-baseline"], env, 240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["value"] > 0 and out["collective_backend"] == "gloo" and out["allreduce_ms"] > 0
    # the in-library leg (opts.ngpus = N; here two contexts of the one device), appended by rank 0 after the group is gone
    hr = out["host_resident_ms"]
    assert "error" not in hr, hr
    assert hr["c1"]["ngpus"] == 2 and hr["c1"]["median_ms"] > 0 and hr["c1"]["max_abs_beta_diff_vs_the_rank_sharded_solve"] < 1e-9
    assert hr["c5_sample"]["ngpus"] == 2 and hr["c5_sample"]["median_ms"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["peer copies", "staged through the host"])
def test_bench_launcher_at_eight_ranks(route):
    """the first 8-rank run should not be the driver's.  `python bench.py --gpus 8` on the one GPU of the box
    (OEM_BENCH_ONE_DEVICE: eight workers on device 0 over gloo): rendezvous, ordinals, the row split with n not a multiple of 8,
    the one JSON line with its `scaling_point` -- and behind the ranks the in-library leg, opts.ngpus = 8 (eight
    contexts of the one device), by BOTH hand-over routes of hoststream.hip: peer copies, and OEMGPU_NO_PEER=1 -- every moment buffer
    through a pinned host buffer, as between devices that cannot access each other."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "OEMGPU_NO_PEER")}
    env.update(OEM_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if route == "staged through the host":
        env["OEMGPU_NO_PEER"] = "1"
    r = _run([sys.executable, str(ROOT / "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--n", "100003", "--full", "--no-c5", "--no-cpu-baseline"], env, 240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["steps"] == 2 and out["value"] > 0 and out["collective_backend"] == "gloo" and out["allreduce_ms"] > 0
    assert out["scaling"] == "strong"
    sp = out["scaling_point"]
    assert sp["n_gpus"] == 8 and sp["c1_strong"]["rows_per_gpu"] in (100003 // 8, 100003 - 7 * (100003 // 8))
    assert sp["c1_strong"]["moments_ms"] > 0 and sp["c1_strong"]["allreduce_ms"] > 0 and sp["c1_strong"]["allgather_ms"] > 0 and sp["c1_strong"]["solve_ms"] > 0
    hr = out["host_resident_ms"]
    assert "error" not in hr, hr
    assert hr["c1"]["ngpus"] == 8 and hr["c1"]["max_abs_beta_diff_vs_the_rank_sharded_solve"] < 1e-9
    staged = hr["c1"]["handovers_staged_through_host"]
    assert (staged >= 7) if route == "staged through the host" else (staged == 0), staged
