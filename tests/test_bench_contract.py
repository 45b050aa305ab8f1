"""bench.py against the driver's contract.  The line is PRODUCED here, never read from a committed file: on the GPU box
the whole bench runs (small batch) and its JSON line is checked field by field and for internal consistency; on CPU the
cpu_baseline leg alone runs (it needs no GPU) next to the CLI flags."""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT


def _check_cpu_baseline(c, unit):
    for k in ("value", "unit", "cores", "kind", "sample", "build", "same_math_brute", "reference_algorithm"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["cores"] == 1 and c["unit"] == unit
    b, r = c["same_math_brute"], c["reference_algorithm"]
    assert b["value"] == c["value"] and b["cores"] == 1
    assert abs(1e3 / b["value"] - b["ms_per_frame"]) / b["ms_per_frame"] < 1e-6
    if r is None:  # oracle/_ref/libnanoflann_ref.so (built from the reference's header, git-ignored) is not in this checkout
        return
    # the two baselines differ only in the association: kd-tree 5-NN is far cheaper than the exhaustive sweep
    assert r["cores"] == 1 and r["assoc_ms_per_frame"] < b["assoc_ms_per_frame"] and r["ms_per_frame"] < b["ms_per_frame"]


def test_cpu_baseline_leg_runs_without_gpu():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-baseline-worker", "20200901", "3"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    _check_cpu_baseline(json.loads(out.stdout.strip().split("\n")[-1]), "frames/s")


def test_bench_cli_accepts_the_driver_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--dump-outputs", "--full"):
        assert flag in out.stdout


def _stub_line(cmd, env=None):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.strip().split("\n") if l.startswith("{")]
    assert len(lines) == 1, out.stdout  # rank 0 alone prints
    return json.loads(lines[0])


def test_bench_gpus_n_starts_n_ranks_itself():
    """`python bench.py --gpus 2` with no launcher around it (what the driver's BENCH / SCALE command is) must become two
    ranks that meet in a process group: same spawn / barrier / MAX-over-ranks code as the real bench, gloo + a stand-in
    step here because there is no GPU."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    d = _stub_line([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "7", "--warmup", "2", "--stub", "gloo"], env)
    assert d["n_gpus"] == 2 and d["steps"] == 7 and d["warmup"] == 2 and d["backend"] == "gloo"
    assert d["steps_run_all_ranks"] == 2 * (7 + 2)  # both ranks ran every step (all_reduce SUM over the group)


def test_bench_gpus_8_walks_the_whole_node_on_cpu():
    """The node of the north star has 8 GPUs and no session has had one: walk `bench.py --gpus 8` once on CPU (gloo, stand-in
    step) so that the first real run meets no surprise of the launch itself - eight ranks in ONE group, every rank ran every step,
    eight per-rank rates that agree with the headline's clock."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["GMMLOC_STUB_STEP_MS"] = "40"
    d = _stub_line([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "4", "--warmup", "1", "--stub", "gloo"], env)
    assert d["n_gpus"] == 8 and d["ranks_in_group"] == 8 and d["backend"] == "gloo"
    assert d["steps_run_all_ranks"] == 8 * (4 + 1)
    assert len(d["per_rank_rate"]) == 8
    share = 1e3 / d["ms_per_step"]
    for r in d["per_rank_rate"]:
        assert share * 0.999 <= r <= 1.25 * share, (r, share)  # (8 processes on a few host cores: the slowest rank sets the headline)


def test_per_rank_rate_is_a_throughput_not_an_enqueue_time():
    """The steps of the real bench only ENQUEUE kernels.  A rank's own rate must be taken after its device is idle: with an
    asynchronous stand-in step (60 ms of 'device' work per step) every rank's rate has to sit within 5 % of its share of the
    headline (the headline is the MAX over ranks; the ranks do the same work) - a clock read before the synchronise reports the
    microseconds of the enqueue instead (round 4: 122 702 326 frames/s beside a headline of 367 633)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["GMMLOC_STUB_STEP_MS"] = "60"
    d = _stub_line([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "1", "--stub", "gloo"], env)
    share = 1e3 / d["ms_per_step"]  # steps/s of one rank by the headline's clock (the stub's `value` also counts the warm-up steps)
    assert 1e3 * 5 * 0.060 <= d["ms_per_step"] * 5 < 1e3 * 5 * 0.060 * 1.25  # the timed region holds the asynchronous work
    assert len(d["per_rank_rate"]) == 2
    for r in d["per_rank_rate"]:
        assert share * 0.999 <= r <= 1.05 * share, (r, share)


def test_bench_under_torchrun_is_a_rank():
    """The documented form: the launcher starts the ranks, bench.py must NOT spawn again."""
    from gmmloc_amd import launch
    d = _stub_line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                    "--master-port", str(launch.free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                    "--stub", "gloo"])
    assert d["n_gpus"] == 2 and d["steps_run_all_ranks"] == 2 * (3 + 1)


def test_bench_gpus_n_refuses_a_node_with_fewer_gpus():
    """No GPU here: the real bench with --gpus 2 must fail loudly instead of printing a 1-GPU line labelled 2."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("node has 2+ GPUs")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode != 0 and "GPU(s) visible" in out.stderr and not out.stdout.strip()


FULL_ONLY = ("cpu_baseline", "latency", "speedup_batched", "assoc_index", "roofline_assoc", "step_with_exhaustive_sweep",
             "step_two_streams", "step_anchored_prior")


@pytest.mark.gpu
def test_bench_plain_line_live():
    """A plain run times the steps and prints the headline with what the timed steps' own timers give; whatever takes runs of
    its own (the other legs, the sweep, the latencies, the CPU baselines) is left to --full."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "512"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.strip().split("\n") if l.startswith("{")]
    assert len(lines) == 1  # ONE JSON line
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "kernel_ms_per_step"):
        assert k in d, k
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    frames = d["config"]["frames_per_step_per_gpu"] * d["steps"] * d["n_gpus"]
    assert abs(d["value"] - frames / (d["ms_per_step"] * d["steps"] / 1e3)) / d["value"] < 1e-6
    r = d["roofline"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0 < r["frac"] < 1
    assert r["avg_launch_ms"] * d["steps"] <= d["ms_per_step"] * d["steps"] * 1.001  # the kernel fits inside the step
    assert "class_1000" not in r
    for k in FULL_ONLY:
        assert k not in d, k


@pytest.mark.gpu
def test_bench_line_contract_live():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "512",
                          "--full"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.strip().split("\n") if l.startswith("{")]
    assert len(lines) == 1  # ONE JSON line
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and d["vs_baseline"] is None  # the exact fp64 step is what is timed
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert "workload" in d["config"] and "model" not in d["config"]
    for k in FULL_ONLY:
        assert k in d, k
    frames = d["config"]["frames_per_step_per_gpu"] * d["steps"] * d["n_gpus"]
    assert abs(d["value"] - frames / (d["ms_per_step"] * d["steps"] / 1e3)) / d["value"] < 1e-6
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0 < r["frac"] < 1
    assert abs(r["achieved"] - r["flop_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e12) / r["achieved"] < 1e-6
    assert r["avg_launch_ms"] * d["steps"] <= d["ms_per_step"] * d["steps"] * 1.001  # the kernel fits inside the step
    _check_cpu_baseline(d["cpu_baseline"], d["unit"])
    sw = d["step_with_exhaustive_sweep"]
    assert sw["unit"] == d["unit"] and 0 < sw["value"] < d["value"]  # the sweep costs more than the index
    lat = d["latency"]
    assert abs(lat["speedup_vs_cpu_same_math_brute"] - lat["cpu_same_math_brute_ms_per_frame"] / lat["single_frame_ms"]) < 1e-6
    assert lat["speedup_vs_cpu_same_math_brute"] >= 50.0  # north-star latency target, against the same arithmetic
    if d["cpu_baseline"]["reference_algorithm"] is not None:
        assert lat["speedup_vs_cpu_reference_algorithm"] >= 50.0  # ... and against the reference's kd-tree algorithm


@pytest.mark.gpu
def test_bench_dump_outputs_live(tmp_path):
    """--dump-outputs: the last timed step's results as float64 .npy files; the inputs are fixed, so two runs with other step
    counts write the same bits, and the refined poses stay unit quaternions with every association in range or -1."""
    import numpy as np
    lines, dirs = [], []
    for steps in (1, 3):
        d = tmp_path / ("s%d" % steps)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                              "--batch", "300", "--no-extra-legs", "--no-cpu-baseline", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:]
        lines.append(json.loads([l for l in out.stdout.strip().split("\n") if l.startswith("{")][0]))
        dirs.append(d)
    assert [l["steps"] for l in lines] == [1, 3] and all(l["ms_per_step"] > 0 for l in lines)
    names = sorted(p.name for p in dirs[0].iterdir())
    assert names == ["Xw.npy", "assoc.npy", "frame_index.npy", "pose.npy", "pose_frame_index.npy"]
    assert sorted(p.name for p in dirs[1].iterdir()) == names
    a = {n[:-4]: np.load(dirs[0] / n) for n in names}
    for n in names:
        b = np.load(dirs[1] / n)
        assert a[n[:-4]].dtype == np.float64 and np.array_equal(a[n[:-4]], b), n
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    B, M, S = 300, 2000, 256  # every pose; the points and associations of a seeded sample of 256 of the 300 frames
    assert a["pose"].shape == (B, 7) and np.array_equal(a["pose_frame_index"], np.arange(B))
    fi = a["frame_index"]
    assert fi.shape == (S,) and (np.diff(fi) > 0).all() and fi[0] >= 0 and fi[-1] < B
    assert a["Xw"].shape == (S, M, 3) and a["assoc"].shape == (S, M)
    assert np.abs(np.linalg.norm(a["pose"][:, :4], axis=1) - 1).max() < 1e-6  # (qx qy qz qw tx ty tz)
    assert ((a["assoc"] >= -1) & (a["assoc"] < 4096)).all() and (a["assoc"] >= 0).mean() > 0.5


def test_bench_gpus_n_walks_the_nccl_path_up_to_the_first_device_call(monkeypatch):
    """Dress rehearsal of the first N > 1 run on a node without GPUs: with torch.cuda.device_count() faked to 2, the REAL argument
    path (`bench.py --gpus 2`, no launcher) must spawn two ranks under torch.distributed.run that each take the nccl branch
    (launch.Ranks("nccl").init) and stop at its first device call with the loud assertion - not fall back to anything."""
    import torch
    from gmmloc_amd import launch
    if torch.cuda.is_available():
        pytest.skip("node has a GPU: covered live by test_bench_nccl_dry_run_on_the_gpu_box")
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 2)
    seen = {}
    real_call = launch.subprocess.call

    def call(cmd, env=None):
        seen["cmd"] = cmd
        r = launch.subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        seen["out"], seen["err"] = r.stdout, r.stderr
        return r.returncode
    monkeypatch.setattr(launch.subprocess, "call", call)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    rc = launch.spawn_ranks(2, os.path.join(ROOT, "bench.py"), ["--gpus", "2", "--steps", "2", "--warmup", "1", "--stub", "nccl-dry"], need_gpus=True)
    monkeypatch.setattr(launch.subprocess, "call", real_call)
    cmd = seen["cmd"]
    # the driver's own command line, rank for rank
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and cmd[cmd.index("--nproc-per-node") + 1] == "2"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert rc != 0 and not [l for l in seen["out"].split("\n") if l.startswith("{")]  # no line without GPUs
    assert seen["err"].count("the HIP path needs a GPU") >= 2  # BOTH ranks reached Ranks("nccl").init()'s device check


@pytest.mark.gpu
def test_bench_nccl_dry_run_on_the_gpu_box():
    """the same path live with the GPUs the box has (1 here): RCCL process group, barrier / MAX / gather on device tensors"""
    import torch
    n = max(1, min(torch.cuda.device_count(), 2))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    d = _stub_line([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "3", "--warmup", "1", "--stub", "nccl-dry"], env)
    assert d["backend"] == "nccl" and d["n_gpus"] == n and d["ranks_in_group"] == n and len(d["per_rank_rate"]) == n
    assert d["steps_run_all_ranks"] == n * (3 + 1)
