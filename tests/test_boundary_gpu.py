"""GPU tests of the boundary's housekeeping entry points: the per-device context (ss_create / ss_destroy) and the
RCCL wrappers (single-rank communicator: the box has one GPU; the 2-rank exchange logic is covered on CPU with gloo in
test_host_cpu.py and on the multi-GPU node by ``bench.py --partition slots``)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_context_create_info_destroy_keeps_tile_table():
    from seedstory import _lib, comm, tune
    with pytest.raises(_lib.SSError):
        comm.Context(99)
    ctx = comm.Context(0)
    info = ctx.info()
    assert info["device"] == 0 and info["cu_count"] == 256 and info["hbm_bytes"] > 200 * 2 ** 30
    tune.load_default_table()
    n = len(tune.export_table())
    assert n > 0
    ctx.close()
    # the tile table is process-global (ops take no handle): other users of the library keep their tuned tiles
    assert len(tune.export_table()) == n


def test_rccl_single_rank_bcast_and_argument_errors():
    from seedstory import _lib, comm
    uid = comm.rccl_unique_id()
    assert len(uid) == 128 and any(uid)
    c = comm.RcclComm(uid, 1, 0)
    t = torch.arange(4096, device=DEV, dtype=torch.float32).to(torch.bfloat16)
    ref = t.clone()
    c.bcast(t, 0)
    torch.cuda.synchronize()
    assert torch.equal(t, ref)
    with pytest.raises(_lib.SSError):
        c.send(t, 0)                                # peer == self
    with pytest.raises(_lib.SSError):
        c.recv(t, 3)                                # peer out of range
    c.close()


def test_slot_ring_and_replicas_under_rccl_world_size_1(tmp_path):
    """The first multi-GPU run must not be the first RCCL run: ``bench.py --partition slots`` and the replica mode on THIS
    box's one GPU with a real ``nccl`` (= RCCL) process group of world size 1 — communicator initialisation, the
    header + flat-payload broadcasts of the slot ring, barrier and max-over-ranks all go through RCCL."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29561",
               SS_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for extra in (["--partition", "slots"],):      # (the replica partition has no data-path collective; its N > 1 bookkeeping —
        # barrier, all_gather of per-rank clocks, max over ranks — is the same code the gloo 2-rank test below runs)
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
               "--stories-per-gpu", "2", "--diffusion-steps", "2", "--story-len", "3", "--no-cpu-baseline", "--no-batch1",
               "--no-tolerance-modes", "--no-roofline"] + extra
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
        line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        assert line["n_gpus"] == 1 and line["value"] > 0
        if extra:
            assert line["backend"] == "nccl" and line["config"]["partition"] == "slots"


def _two_rank_bench(env_extra, extra_args, port, timeout=900):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--stories-per-gpu", "2", "--diffusion-steps", "2", "--story-len", "3", "--full", "--no-cpu-baseline", "--no-batch1",
           "--no-tolerance-modes"] + extra_args
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)


def test_two_ranks_one_device_under_rccl_or_recorded_refusal():
    """the header + flat-payload broadcast of the slot ring should cross a real RCCL communicator with
    TWO ranks before the driver's 8-GPU run.  The box has one GPU: both ranks are put on cuda:0 (``SS_BENCH_SHARE_DEVICE``).
    RCCL 2.26 refuses that at communicator creation ("Duplicate GPU detected : rank 0 and rank 1 both on CUDA device ...",
    no environment switch in librccl.so) — then the refusal text is asserted (so a future RCCL that accepts it turns
    this into a real 2-rank run) and the test is SKIPPED with that reason; the 2-rank flow itself is covered by
    ``test_two_ranks_one_device_gloo_slot_ring`` below and, for the payload logic, by the CPU gloo tests."""
    import json
    out = _two_rank_bench({"SS_BENCH_SHARE_DEVICE": "1", "NCCL_DEBUG": "WARN"}, ["--partition", "slots"], 29571, timeout=600)
    if out.returncode != 0:
        text = out.stdout[-6000:] + out.stderr[-6000:]
        assert "Duplicate GPU detected" in text or "invalid usage" in text.lower() or "ncclInvalidUsage" in text, text[-3000:]
        pytest.skip("RCCL refuses two ranks on one device (Duplicate GPU detected): 2-rank nccl needs 2 GPUs")
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["backend"] == "nccl" and line["rccl_ranks"] == 2 and line["value"] > 0


def test_two_ranks_one_device_gloo_slot_ring():
    """Both partitions' N > 1 code paths end to end on the GPU with TWO processes (gloo carries the collectives, device tensors
    staged through the host): owner rotation, header + flat payload, KV mirror install, render on the owner's side stream,
    per-rank numbers and the roofline section in the JSON line."""
    import json
    out = _two_rank_bench({"SS_BENCH_SINGLE_DEVICE": "1", "SS_BENCH_WATCHDOG_S": "800"}, ["--partition", "slots"], 29573)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["rccl_ranks"] == 2 and line["backend"] == "gloo" and line["value"] > 0
    assert len(line["per_rank"]) == 2 and sum(r["rounds_rendered"] for r in line["per_rank"]) == 2
    assert line["roofline"] is not None and line["roofline"]["bound"] == "mfma"
