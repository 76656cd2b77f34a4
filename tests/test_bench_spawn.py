"""`python bench.py --gpus N` must start N ranks itself.  CPU coverage of that spawn path: the dry-run mode
runs bench.py's own launcher + rendezvous + gather skeleton over gloo without a GPU; the mismatch cases must exit non-zero
instead of silently reporting one rank."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(kw)
    return e


def test_bench_gpus2_spawns_two_ranks_gloo_dryrun():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"], env=_env(NPP_BENCH_DRYRUN="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                      # rank 0 prints ONE line
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["collective_ranks"] == 2
    assert j["gathered"] == [0.0, 1.0] and j["max_over_ranks"] == 2.0


def test_bench_refuses_more_gpus_than_devices():
    """No GPU in this container: `--gpus 2` without the dry-run knob must fail loudly, not print an N=1 line."""
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("node has >= 2 GPUs")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "--gpus 2" in r.stderr and not any(l.startswith("{") for l in r.stdout.splitlines())


def test_bench_refuses_world_size_mismatch():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4"], env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_bench_refuses_bad_step_and_window_counts():
    """--steps sets the number of timed steps (at least one); --windows 0 reports the pre-drawn-pool loop, which only --full runs."""
    for extra in (["--steps", "0"], ["--windows", "0"], ["--windows", "-1", "--full"]):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + extra, env=_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and not any(l.startswith("{") for l in r.stdout.splitlines()), extra


def test_launch_ranks_helper_returns_child_code(tmp_path):
    sys.path.insert(0, ROOT)
    from npp_amd.parallel import launch_ranks
    ok = tmp_path / "ok.py"
    ok.write_text("import os, torch.distributed as d\nd.init_process_group('gloo')\nassert d.get_world_size() == 2\n"
                  "d.barrier()\nd.destroy_process_group()\n")
    bad = tmp_path / "bad.py"
    bad.write_text("import sys\nsys.exit(3)\n")
    assert launch_ranks(str(ok), 2, [], timeout=240) == 0
    assert launch_ranks(str(bad), 2, [], timeout=240) != 0


import pytest  # noqa: E402


@pytest.mark.gpu
def test_bench_under_torchrun_initialises_rccl_on_the_card():
    """The driver's launch form (python -m torch.distributed.run ... bench.py --gpus N) with N = 1 on a real GPU: the nccl (= RCCL)
    process group is initialised with device_id binding, and the barrier / all_gather / all_reduce of the timing protocol run
    through it -- the same code path as N = 8, exercised on hardware by the one rank this box has (a child process: the test
    process itself has touched the GPU)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from npp_amd.parallel import free_port
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", str(free_port()), BENCH, "--gpus", "1", "--steps", "40", "--warmup", "5", "--no-extras",
                        "--no-cpu-baseline"], env=_env(HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 1 and j["collective"] == {"backend": "nccl (RCCL)", "ranks": 1}
    assert j["per_rank_rows_per_s"] == [j["value"]] and j["value"] > 1e6 and j["scaling"] == "weak"


@pytest.mark.gpu
def test_four_ranks_on_one_card_with_a_node_share_of_cpus_each():
    """SURVEY 8e names the risk of config c3: eight ranks' host threads (34 C-ABI calls per 0.65-ms iteration + a sampler producer
    thread each) on shared cores.  Rehearsal on the one card a box has: 4 ranks (gloo, all on cuda:0), each confined to 2 logical
    CPUs (= 16 / 8, the share a rank gets on the 8-GPU node).  The card is shared four ways, so the device numbers mean nothing
    here; what is asserted is the HOST side: every rank enqueues an iteration in less time than the device needs for it on a card
    of its own (0.65 ms), i.e. the loop stays device-bound with the node's CPU share, and every rank's sampling-inclusive loop runs."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if len(os.sched_getaffinity(0)) < 8:
        pytest.skip("fewer than 8 CPUs")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--steps", "40", "--warmup", "5", "--full", "--no-psnr", "--no-cpu-baseline"],
                       env=_env(NPP_BENCH_DEVICE="0", NPP_BENCH_BACKEND="gloo", NPP_BENCH_CPUS_PER_RANK="2",
                                HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert j["n_gpus"] == 4 and j["collective"]["ranks"] == 4 and len(j["per_rank_rows_per_s"]) == 4
    e = j["all_ranks_incl_sampling"]
    # (round 6: the headline `value` IS the sampling-inclusive loop of every rank -- per_rank_rows_per_s; the pre-drawn-pool loop is
    #  reported beside it)
    assert len(e["host_enqueue_ms_per_iter"]) == 4 and len(j["device_only_per_rank_rows_per_s"]) == 4 and "samples" in j["config"]["value_is"]
    print("host enqueue ms per iteration, per rank:", [round(v, 3) for v in e["host_enqueue_ms_per_iter"]],
          "| sampling-inclusive rows/s per rank (card shared 4 ways):", [round(v) for v in j["per_rank_rows_per_s"]])
    assert max(e["host_enqueue_ms_per_iter"]) < 0.6, e


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_outputs(tmp_path):
    """A plain run prints the headline line of exactly --steps timed steps (one window) and nothing beside it, and
    --dump-outputs writes the last step's arrays as float32 .npy files within 64 MB (a child process, like the tests above)."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "10", "--warmup", "2", "--dump-outputs", str(out)],
                       env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["steps"] == 10 and j["unit"] == "rows/s" and j["higher_is_better"] is True and j["dtype"] == "bf16"
    assert j["ms_per_step"] > 0 and j["value"] > 1e6 and j["config"]["value_is"].startswith("one window")
    assert "roofline" not in j and "cpu_baseline" not in j and "device_only_rows_per_s" not in j["config"]
    files = sorted(p.name for p in out.iterdir())
    assert files == ["latents.npy", "params.npy", "patch_loss.npy", "pixel_loss.npy", "pred.npy"]
    arrays = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["pred"].shape == (j["config"]["rows_per_step"], 3)
