"""The path's only exchange on hardware: a 1-rank RCCL ("nccl") process group on the MI355X runs the pose-stream gathers
with device tensors, including the int64 all-reduces of the ragged form (BASELINE configs[3]; SURVEY.md §8e — new design,
the reference has no collective).  Each case runs in a child process so the group never leaks into the other GPU tests.
More ranks cannot share one card under RCCL; the N > 1 layout is covered by tests/test_sharding_gloo.py (gloo, 2 ranks)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import os, sys, json
import numpy as np
sys.path.insert(0, %(root)r)
import torch, torch.distributed as dist
from stereo_visual_odometry_amd import sharding
os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = "29541"
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
rng = np.random.default_rng(7)
local = rng.normal(size=(3, 6, 17))
out = sharding.gather_pose_streams(torch.from_numpy(local).to(dev), dst=0)
assert len(out) == 1 and out[0].is_cuda and np.array_equal(out[0].cpu().numpy(), local)
lens = [27, 11, 46]
streams = [rng.normal(size=(n, 17)) for n in lens]
rag = sharding.gather_ragged_pose_streams(streams, dst=0, device=dev)
assert sorted(rag) == [0, 1, 2] and all(np.array_equal(rag[k], streams[k]) for k in range(3))
empty = sharding.gather_ragged_pose_streams([], dst=0, device=dev)
assert empty == {}
t = torch.tensor([3.5], dtype=torch.float64, device=dev); dist.all_reduce(t, op=dist.ReduceOp.MAX)
assert float(t.item()) == 3.5
dist.barrier()
dist.destroy_process_group()
print(json.dumps({"ok": True, "backend": "nccl"}))
"""


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


def test_rccl_world1_pose_gathers_on_device():
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"ok": True, "backend": "nccl"}


def test_bench_runs_its_exchange_through_rccl():
    """bench.py with a forced 1-rank group: init_process_group("nccl"), the warm-up gather, the timed gather of the pose
    streams and the all-reduces all execute on the device; the line still says n_gpus 1."""
    env = _env(); env["SVO_BENCH_FORCE_GROUP"] = "1"; env["MASTER_PORT"] = "29543"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--seqs", "8",
                        "--contexts", "1", "--cpu-frames", "0"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["config"]["pose_ok_fraction"] > 0.9
    # the exchange is outside nobody's clock, so it must not cost the rate: same arguments without the group, same box
    env2 = _env(); env2.pop("SVO_BENCH_FORCE_GROUP", None)
    best = {True: 0.0, False: 0.0}
    for rep in range(2):                                             # best of two each way: a 3 x 8-sequence run is short, boxes jitter
        for grouped, e in ((True, env), (False, env2)):
            rr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "4", "--seqs", "32",
                                 "--contexts", "1", "--cpu-frames", "0", "--ate-frames", "0"], env=e, capture_output=True, text=True, timeout=900)
            assert rr.returncode == 0, rr.stderr[-2000:]
            best[grouped] = max(best[grouped], json.loads(rr.stdout.strip().splitlines()[-1])["value"])
    assert abs(best[True] - best[False]) < 0.03 * best[False], best


def test_bench_two_ranks_end_to_end_on_one_gpu_gloo():
    """The N > 1 path of bench.py on hardware, as far as a one-GPU box allows: `python bench.py --gpus 2` starts two ranks itself
    (torch.distributed.run child); both use GPU 0 (--same-device) and exchange over gloo, because RCCL refuses two ranks on one
    device.  Sharded sequences, barrier, max-over-ranks timing, the pose-stream gather to rank 0 and the reductions all run; the
    line says n_gpus 2 and counts both ranks' sequences."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--same-device", "--steps", "3",
                        "--warmup", "1", "--seqs", "8", "--contexts", "1", "--pool", "2", "--full", "--cpu-frames", "6", "--ate-frames", "3"],
                       env=_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["config"]["sequences_per_gpu"] == 8 and line["config"]["pose_ok_fraction"] > 0.9
    assert abs(line["value"] - 2 * 8 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-6 * line["value"]     # whole-job rate over both ranks
    # an N > 1 line is COMPLETE (round-2 verdict): roofline from the slowest rank's kernel time, the CPU baseline leg run by rank 0
    # after the timed region, and every rank's own rate so that a straggler shows
    assert line["roofline"]["frac"] > 0 and line["roofline"]["kernel_avg_ms"] > 0
    assert len(line["per_rank_value"]) == 2 and all(v > 0 for v in line["per_rank_value"])
    assert len(line["per_rank_lk_kernel_avg_ms"]) == 2 and line["roofline"]["kernel_avg_ms"] == max(line["per_rank_lk_kernel_avg_ms"])
    assert line["value"] <= sum(line["per_rank_value"]) * (1 + 1e-9)
    cpu = line["cpu_baseline"]
    assert cpu is not None and cpu["value"] > 0 and cpu["kind"] == "port" and "opencv" in cpu
    assert line["ate"]["long_run"]["frames"] == 3 and line["ate"]["long_run"]["frames_with_identical_flags_and_counters"] == 4
    # the extra leg in the reference's own LK rounding (lk_float_sums = 1): rank 0's GPU, after the timed region
    fs = line["float_sums_mode"]
    assert fs is not None and fs["value"] > 0 and fs["n_gpus"] == 1 and fs["pose_ok_fraction"] > 0.9 and fs["lk_kernel_avg_ms"] > 0


# ---------------------------------------------------------------------------- the C entry of the exchange (libsvo_rccl.so)
@pytest.mark.gpu
def test_c_entry_of_the_pose_gather_on_a_one_device_communicator():
    """a C / C++ host that drives the GPUs from one process gathers its pose streams through
    svo_gather_pose_streams (ncclCommInitAll + grouped ncclSend / ncclRecv).  The test box has one GPU: a 1-device communicator
    (the N-device run is the driver's, like every N > 1 run); plain g++, no torch, no Python in the child."""
    import subprocess
    exe = os.path.join(ROOT, "tests", "cpp", "gather_gpu_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gather_gpu_test.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_rccl",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([exe, "1"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "GATHER OK 1" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cfg4_from_a_cpp_host_matches_the_python_api(tmp_path):
    """BASELINE configs[3] without Python in the data path: tools/svo_multi_gpu.cpp shards S sequences over the devices (one host
    thread each, the reference's driver loop per GPU), gathers the pose streams through libsvo_rccl.so and writes one
    result_seqNN.csv per sequence.  One device here; the trajectories must equal those of the Python API on the same frames."""
    import subprocess
    import numpy as np
    sys.path.insert(0, ROOT)
    from stereo_visual_odometry_amd import api, evaluate, synthetic as syn
    cal = dict(syn.KITTI00, width=320, height=160, cx=160.0, cy=80.0)
    S, F = 3, 5
    seqs = [syn.StereoSequence(cal=cal, n_frames=F, seed=0x5EED0040 + s, step=0.3) for s in range(S)]
    path = tmp_path / "frames.bin"
    with open(path, "wb") as f:
        f.write(np.array([S, F, 160, 320], np.int32).tobytes())
        f.write(np.array([cal["fx"], cal["cx"], cal["cy"], cal["bf"]], np.float32).tobytes())
        for q in seqs:
            for l, r in zip(q.left, q.right):
                f.write(l.tobytes()); f.write(r.tobytes())
    exe = os.path.join(ROOT, "tools", "svo_multi_gpu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "svo_multi_gpu.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"),
                           "-lsvo_hip", "-lsvo_rccl", "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, str(path), "1", str(tmp_path), "10", "2.0"], capture_output=True, text=True, timeout=300, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0 and "MULTI OK 3 sequences 5 frames 1 devices" in out.stdout, out.stdout + out.stderr
    Pl, Pr = syn.projection_matrices(cal)
    for s, q in enumerate(seqs):
        vo = api.VisualOdometry(cfg=api.default_config(max_translation_norm=2.0)); vo.initalize_projection_matricies(Pl, Pr)
        pose, track = np.eye(4), []
        for k in range(F):
            ok, T = vo.stereo_callback(q.left[k], q.right[k])
            pose = pose @ T; track.append(pose[:3, 3].copy())
        rows = evaluate.read_result_csv(tmp_path / ("result_seq%02d.csv" % s))
        assert rows.shape[0] == F and np.abs(rows[:, :3] - np.array(track)).max() < 1e-8, s
