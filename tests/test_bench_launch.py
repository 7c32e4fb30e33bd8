"""bench.py's rank launch (no GPU): `--gpus N` without a launcher starts N
rank processes itself, a launcher whose WORLD_SIZE differs from --gpus is
refused, and the RCCL-id hand-over reaches every spawned rank.  --dry-run
stops each rank before its first HIP call."""
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO

BENCH = os.path.join(REPO, "bench.py")


def _clean_env():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_PORT", "RTAMD_RUN_ID",
              "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    return env


@pytest.mark.parametrize("n", [2, 3])
def test_gpus_n_spawns_n_ranks(n):
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--dry-run"], capture_output=True, text=True,
                       timeout=120, env=_clean_env(), cwd=REPO)
    assert r.returncode == 0, r.stderr
    views = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert sorted(v["rank"] for v in views) == list(range(n))
    assert all(v["world"] == n and v["local_rank"] == v["rank"] and v["id_ok"] for v in views)


def test_single_gpu_runs_in_process():
    r = subprocess.run([sys.executable, BENCH, "--dry-run"], capture_output=True, text=True, timeout=120,
                       env=_clean_env(), cwd=REPO)
    assert r.returncode == 0, r.stderr
    (v,) = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert (v["rank"], v["world"]) == (0, 1)


def test_launcher_world_must_match_gpus():
    env = dict(_clean_env(), RANK="0", WORLD_SIZE="2", LOCAL_RANK="0", LOCAL_WORLD_SIZE="2", MASTER_PORT="1")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--dry-run"], capture_output=True, text=True,
                       timeout=120, env=env, cwd=REPO)
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stderr
    assert not r.stdout.strip()


def test_multi_node_world_is_refused():
    env = dict(_clean_env(), RANK="0", WORLD_SIZE="2", LOCAL_RANK="0", LOCAL_WORLD_SIZE="1", MASTER_PORT="1")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run"], capture_output=True, text=True,
                       timeout=120, env=env, cwd=REPO)
    assert r.returncode != 0 and "LOCAL_WORLD_SIZE" in r.stderr


def _bench_module():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _check_ranks_block(blk, world, H):
    assert blk["rccl_world"] == [world]
    assert len(blk["kernel_ms"]["per_rank"]) == world
    assert blk["kernel_ms"]["min"] <= blk["kernel_ms"]["max"]
    assert sum(blk["rows"]) == H
    for key in ("reduce_device", "verdict_wait_host"):
        assert len(blk["agreement_ms"][key]) == world
    assert len(blk["gather_ms"]["per_rank"]) == world and len(blk["gather_ms"]["last_chunk_per_rank"]) == world
    assert set(blk["placement_ms"]) == {"root_total", "root_last_chunk"}
    assert len(blk["call_ms"]) == world and len(blk["tail_ms"]) == world
    json.dumps(blk)   # (goes into the JSON line)


def test_ranks_block_schema_synthetic():
    """The N > 1 line's per-rank block from synthetic rank values (no GPU)."""
    b = _bench_module()
    world, H = 3, 50
    splits = [[1.5 + r, 0.01, 0.02, 0.1, 0.3 if r == 0 else 0.0, 0.03, 0.05 if r == 0 else 0.0, 0.04, world,
               [18, 16, 16][r]] for r in range(world)]
    blk = b.ranks_block([1.0, 1.2, 1.1], [0.05] * 3, splits)
    _check_ranks_block(blk, world, H)
    assert blk["kernel_ms"]["max"] == 1.2 and blk["placement_ms"]["root_total"] == 0.3


def test_dump_outputs_whole_frame_and_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs' writer (no GPU): a small frame is written whole; a
    frame above DUMP_MAX_PIXELS is cut to that many pixels, the same ones on
    every call, in ascending order, as float64."""
    import numpy as np

    b = _bench_module()
    fb = np.random.default_rng(7).random((9, 11, 3))
    info = b.dump_outputs(str(tmp_path / "whole"), fb, [5, 6, 7])
    assert (info["frame_pixels"], info["of"]) == (99, 99)
    assert np.array_equal(np.load(tmp_path / "whole" / "frame.npy"), fb.reshape(-1, 3))
    assert np.array_equal(np.load(tmp_path / "whole" / "rays.npy"), [5.0, 6.0, 7.0])

    monkeypatch.setattr(b, "DUMP_MAX_PIXELS", 40)
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), fb, [5, 6, 7])
    idx = np.load(tmp_path / "s1" / "frame_pixels.npy")
    got = np.load(tmp_path / "s1" / "frame.npy")
    assert idx.dtype == np.float64 and got.dtype == np.float64 and got.shape == (40, 3)
    assert (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < 99
    assert np.array_equal(got, fb.reshape(-1, 3)[idx.astype(np.int64)])
    for name in ("frame", "frame_pixels", "rays"):
        assert np.array_equal(np.load(tmp_path / "s1" / f"{name}.npy"), np.load(tmp_path / "s2" / f"{name}.npy"))


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_frame(gpu, tmp_path):
    """A plain `bench.py --steps K --dump-outputs DIR` on config 2: the line
    carries the headline fields and none of the --full legs, K sets the timed
    steps, and the dumped frame and ray counts are what a render of the same
    scene returns in this (another) process, bit for bit."""
    import numpy as np

    import scenes

    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "2", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "a")], capture_output=True, text=True, timeout=120,
                       env=_clean_env(), cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    (line,) = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert (line["steps"], line["warmup"], line["n_gpus"], line["dtype"], line["unit"]) == (3, 1, 1, "f64", "Mrays/s")
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["full"] is False
    assert not {"roofline", "cpu_baseline", "fp32_fast_path"} & set(line)
    assert set(line["wall_clock_ms"]) == {"rng", "kernel", "gather"}

    text, mode = scenes.config_json(2)
    sc = gpu.load_scene_from_json_text(text)
    st = gpu.Stats()
    fb = gpu.Tracer(sc, sc.width, sc.height, mode).render(st)
    frame = np.load(tmp_path / "a" / "frame.npy")
    idx = np.load(tmp_path / "a" / "frame_pixels.npy").astype(np.int64)
    assert frame.dtype == np.float64 and line["dumped"]["of"] == sc.width * sc.height
    assert np.array_equal(frame, fb.reshape(-1, 3)[idx])
    rays = np.load(tmp_path / "a" / "rays.npy")
    assert list(rays[:2]) == [st.rays_intersect, st.rays_occluded]
    assert line["config"]["rays_per_frame"] == st.rays_intersect + st.rays_occluded


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 8])
def test_ranks_block_from_thread_ranks(gpu, world):
    """The same block from real rank splits: world concurrent ranks on one GPU
    through the product's dist_frame (rt_test_dist_threads)."""
    import numpy as np

    import scenes

    b = _bench_module()
    sc = gpu.load_scene_from_json_text(scenes.config_json(4, dpi=40)[0])
    W, H = sc.width, sc.height
    split = np.zeros((2, world, 10))
    out, rc, ms, msg = gpu.dist_threads(sc, W, H, 0, world, frames=2, split_out=split)
    assert (rc == 0).all(), msg
    last = split[1]
    blk = b.ranks_block([1.0] * world, [0.0] * world, [list(x) for x in last])
    _check_ranks_block(blk, world, H)
    assert blk["placement_ms"]["root_total"] > 0 and all(g > 0 for g in blk["gather_ms"]["per_rank"])
    assert all(c > 0 for c in blk["call_ms"])
