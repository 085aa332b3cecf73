"""GPU test of the drop-in boundary against the REAL CompV library: oracle/_ref/headless_samples runs the
samples' call sequences (samples/edges_canny, samples/hough_lines) through CompVEdgeDete::newObj / CompVHough::newObj
twice -- stock CPU factories, then the HIP factories registered by id with CompVFeature::addFactory -- and compares.
The binary is built with the reference library (oracle/build_ref.sh needs the CompV sources) and travels with oracle/_ref/."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "headless_samples")


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,frames", [(641, 480, 1), (1280, 720, 2), (1920, 1080, 1)])
def test_real_compv_with_hip_factories(W, H, frames):
    # on a GPU box the prebuilt drop-in binary must be there: a missing one is a failure of the build / snapshot, not a reason to skip
    assert os.path.exists(BIN), "oracle/_ref/headless_samples is missing: run __graft_entry__.build() where the CompV sources are (oracle/build_ref.sh)"
    r = subprocess.run([BIN, str(W), str(H), str(frames)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert "DROP-IN PARITY OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.returncode == 0


@pytest.mark.gpu
def test_bench_under_torchrun_nccl_single_rank(tmp_path):
    """The multi-GPU code path of bench.py (torch.distributed with backend nccl = RCCL: init_process_group, barrier around the timed
    region, all_reduce(MAX) of the elapsed time, all_gather of the per-frame line counts) executed on real hardware with the one
    GPU a test box has: `torch.distributed.run --nproc-per-node 1 bench.py --force-dist`."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", "29617",
           os.path.join(root, "bench.py"), "--gpus", "1", "--force-dist", "--steps", "3", "--warmup", "1", "--reps", "2", "--frames-per-gpu", "2",
           "--width", "1280", "--height", "720", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["dist_backend"] == "nccl" and res["n_gpus"] == 1 and res["value"] > 0
    assert res["lines_last_step_all_ranks"] is not None and res["lines_frame0"] > 0
    assert res["n_ranks_seen"] == 1 and res["ranks_seen"] == [0] and res["rccl_version"]      # what a SCALE record is checked against


def _two_rank_scatter_run(backend, port):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "2", "--shared-gpu", "--scatter", "--steps", "4", "--warmup", "2", "--reps", "2", "--frames-per-gpu", "2",
           "--batches", "4", "--width", "1280", "--height", "720", "--no-cpu-baseline", "--no-extras", "--full", "--dist-backend", backend]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    res = None
    if r.returncode == 0:
        res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return r, res


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu_with_the_rccl_data_path(tmp_path):
    """N > 1 logic driving the HIP path on hardware, with the one GPU a test box has: two ranks (two processes, two HIP contexts) share
    cuda:0, torch.distributed backend nccl (= RCCL) carries bench.py --scatter's data path -- rank 0 owns every step's batch and sends
    rank 1 its block (grouped send/recv), line counts and the strongest lines are all-gathered -- plus the barrier / MAX brackets.
    The backend that carried the payload is asserted and printed.  An RCCL build that refuses two ranks on ONE device ("Duplicate GPU
    detected") cannot run this on a one-GPU box: that is reported as an xfail naming the reason, never silently replaced by another backend
    (the gloo run is its own test below)."""
    r, res = _two_rank_scatter_run("nccl", 29618)
    if r.returncode != 0 and ("Duplicate GPU detected" in r.stderr or "invalid usage" in r.stderr):
        pytest.xfail("this RCCL build refuses two ranks on one device (Duplicate GPU detected): the RCCL scatter needs two GPUs")
    assert r.returncode == 0, r.stderr[-3000:]
    print("two-rank scatter / gather carried by torch.distributed backend:", res["dist_backend"])
    assert res["dist_backend"] == "nccl"
    assert res["n_gpus"] == 2 and res["value"] > 0 and "scattered from rank 0 over nccl" in res["config"]["parallelism"]
    assert res["lines_last_step_all_ranks"] is not None and res["lines_frame0"] > 0


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu_gloo_host_staged(tmp_path):
    """The same two-rank run with the gloo backend (payload staged through the host): two processes and two HIP contexts drive the HIP path
    under the N > 1 logic whatever the RCCL build allows on one device."""
    r, res = _two_rank_scatter_run("gloo", 29619)
    assert r.returncode == 0, r.stderr[-3000:]
    assert res["dist_backend"] == "gloo" and res["ranks_seen"] == [0, 1]
    assert res["n_gpus"] == 2 and res["value"] > 0 and "scattered from rank 0 over gloo" in res["config"]["parallelism"]
    assert res["lines_last_step_all_ranks"] is not None and res["lines_frame0"] > 0


@pytest.mark.gpu
def test_plain_bench_dumps_the_last_step_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps and prints the headline only; --dump-outputs writes what the last timed step returned,
    and those outputs match the reference-derived fixture of the frames that step processed (line counts, strength sums, line-set hashes, edge counts)."""
    import json
    import sys
    import numpy as np
    from compv_amd import sharding
    steps, warmup, F, NB, W, H = 3, 1, 2, 2, 3840, 2160
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--frames-per-gpu", str(F),
           "--batches", str(NB), "--width", str(W), "--height", str(H), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(out) == 1, r.stdout[-2000:]
    res = json.loads(out[0])
    assert res["metric"].startswith("Mpixels/s") and res["unit"] == "Mpixels/s" and res["higher_is_better"] is True and res["dtype"] == "u8"
    assert res["steps"] == steps and res["reps"] == 1 and res["ms_per_step"] > 0 and res["value"] > 0
    assert abs(res["value"] - F * W * H / (res["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * res["value"] + 1
    assert "roofline" not in res and "cpu_baseline" not in res and "kht" not in res
    arrays = {n[:-4]: np.load(str(tmp_path / n)) for n in os.listdir(str(tmp_path))}
    assert sorted(arrays) == ["counts", "edge_rows", "edges_sample", "lines"]
    assert all(a.dtype == np.float32 for a in arrays.values()) and sum(a.nbytes for a in arrays.values()) <= 64 << 20
    with open(os.path.join(ROOT, "tests", "golden", "golden_batch.json")) as f:
        golden = {g["seed"]: g for g in json.load(f)["frames"]}
    seeds = sharding.block_seeds(F, NB)[sharding.block_of_step(0, warmup + steps - 1, NB)]
    counts = arrays["counts"].astype(np.int64)
    assert len(arrays["lines"]) == counts.sum() and arrays["edge_rows"].shape == (F, H)
    first = 0
    for f, seed in enumerate(seeds):
        g = golden[seed]
        ln = arrays["lines"][first:first + counts[f]].astype(np.int64)
        first += counts[f]
        h = sum(((W + H) - int(row) + 32768) * 1000003 + int(col) * 7919 + int(st) * 31337 for st, row, col in ln[:, 2:]) & ((1 << 64) - 1)
        got = (int(counts[f]), int(ln[:, 2].sum()), "%016x" % h, int(arrays["edge_rows"][f].sum()))
        assert got == (g["lines"], g["sum_strength"], g["line_hash"], g["edges"]), (seed, got)


@pytest.mark.gpu
def test_bare_bench_gpus_2_starts_two_ranks_itself():
    """NO launcher in the command.  `python bench.py --gpus 2 ...` must start its own two ranks (one GPU on a test box: --shared-gpu, gloo
    carrying the scatter), print exactly ONE JSON line on stdout, and that line must say two ranks ran."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--shared-gpu", "--dist-backend", "gloo", "--scatter", "--steps", "4", "--warmup", "2",
           "--reps", "2", "--frames-per-gpu", "2", "--batches", "4", "--width", "1280", "--height", "720", "--no-cpu-baseline", "--no-extras"]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(out) == 1 and out[0].startswith("{"), r.stdout[-2000:]
    res = json.loads(out[0])
    assert res["n_gpus"] == 2 and res["ranks_seen"] == [0, 1] and res["n_ranks_seen"] == 2
    assert res["dist_backend"] == "gloo" and res["value"] > 0


@pytest.mark.gpu
def test_bare_bench_refuses_more_gpus_than_visible():
    """A bare `python bench.py --gpus N` with N > the GPUs of the node: the ranks it starts itself name the missing GPU and the launch ends non-zero in seconds,
    with no JSON line (on a node that has the GPUs the same command is a normal run)."""
    import subprocess
    import sys
    import torch
    want = torch.cuda.device_count() + 1
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(want), "--steps", "2", "--warmup", "1", "--reps", "1", "--frames-per-gpu", "2", "--batches", "2",
           "--width", "1280", "--height", "720", "--no-cpu-baseline", "--no-extras"]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode != 0
    assert ("wants cuda:%d but this node shows %d GPU" % (want - 1, want - 1)) in r.stderr, r.stderr[-2000:]
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


MGB = os.path.join(ROOT, "integration", "_build", "multi_gpu_batch")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [["--devices", "1"], ["--virtual", "2"]])
def test_cxx_multi_gpu_batch_driver(mode):
    """integration/multi_gpu_batch.cxx: ONE C++ process, one compvhip context + plan + stream per device, batch born on device 0 and split with a
    grouped ncclSend / ncclRecv (RCCL directly), per-frame line counts all-gathered; every frame checked against tests/golden/golden_batch.json.
    A test box has one GPU: `--devices 1` runs the RCCL code path (communicator, group calls, all-gather) with one rank, `--virtual 2` runs two
    ranks (two contexts, plans, streams) on that GPU with device copies as transport."""
    import json
    assert os.path.exists(MGB), "integration/_build/multi_gpu_batch is missing: run integration/build.sh"
    r = subprocess.run([MGB, "--frames-per-device", "3", "--steps", "2"] + mode, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0 and "MULTI-GPU BATCH OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    ranks = 2 if mode[0] == "--virtual" else 1
    assert res["ranks"] == ranks and res["frames_checked"] == 3 * ranks and res["Mpixels_per_s"] > 0
    assert ("rccl" in res["transport"]) == (mode[0] == "--devices")


@pytest.mark.gpu
def test_cxx_multi_gpu_batch_driver_refuses_missing_peers():
    """The first N > 1 run of the C++ driver will be unattended: asking for more devices than the node shows is a clear non-zero exit, not a
    silently smaller run."""
    import torch
    assert os.path.exists(MGB), "integration/_build/multi_gpu_batch is missing: run integration/build.sh"
    want = torch.cuda.device_count() + 1
    r = subprocess.run([MGB, "--devices", str(want), "--frames-per-device", "1", "--steps", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 3 and ("only %d HIP device" % (want - 1)) in r.stderr, (r.returncode, r.stderr[-500:])


@pytest.mark.gpu
def test_bench_refuses_a_rank_without_a_gpu():
    """The first N > 1 bench run will be the driver's, unattended: a rank whose LOCAL_RANK has no GPU must end the job with a message that names both numbers
    (on a node that does have the GPUs the same command is a normal two-rank run)."""
    import json
    import sys
    import torch
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29621",
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--reps", "1", "--frames-per-gpu", "2", "--batches", "2",
           "--width", "1280", "--height", "720", "--no-cpu-baseline", "--no-extras"]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if torch.cuda.device_count() >= 2:
        assert r.returncode == 0, r.stderr[-3000:]
        res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert res["n_gpus"] == 2 and res["ranks_seen"] == [0, 1] and res["dist_backend"] == "nccl"
    else:
        assert r.returncode != 0
        assert "wants cuda:1 but this node shows 1 GPU" in (r.stderr + r.stdout), r.stderr[-2000:]
