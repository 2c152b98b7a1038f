"""bench.py --dump-outputs and the plain / --full split.

CPU: dump_outputs writes a frame's pixel words as exact float32 channel values,
whole up to DUMP_MAX_PIXELS and as a fixed, seeded sample (with its pixel
indices) above; the option parser knows --full and --dump-outputs.
GPU: a plain run times exactly --steps frames, carries ms_per_step and the
headline keys and none of the --full measurements, and the frame it dumps is
the renderer's own frame of the same configuration (which test_gpu_rt.py
checks against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _words(n, seed=1):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _pack(chan):
    """float32 [..., 4] channel values (B, G, R, A) back to pixel words."""
    c = chan.astype(np.uint32)
    return c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16) | (c[..., 3] << 24)


def test_dump_whole_frame_is_exact(tmp_path):
    import bench
    w, h = 48, 40
    frame = _words(w * h).reshape(h, w)
    info = bench.dump_outputs(str(tmp_path / "d"), frame, w, h)
    got = np.load(tmp_path / "d" / "framebuffer.npy")
    assert got.dtype == np.float32 and got.shape == (h, w, 4) == tuple(info["framebuffer"])
    assert not info["sampled"] and not (tmp_path / "d" / "framebuffer_index.npy").exists()
    assert np.array_equal(_pack(got), frame)


def test_dump_large_frame_is_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_PIXELS", 1000)
    w, h = 64, 33
    frame = _words(w * h, seed=2)
    a = bench.dump_outputs(str(tmp_path / "a"), frame, w, h)
    bench.dump_outputs(str(tmp_path / "b"), frame, w, h)
    got = np.load(tmp_path / "a" / "framebuffer.npy")
    idx = np.load(tmp_path / "a" / "framebuffer_index.npy")
    assert a["sampled"] and got.dtype == np.float32 and got.shape == (1000, 4)
    assert idx.dtype == np.float64 and idx.shape == (1000,)
    i = idx.astype(np.int64)
    assert np.all(np.diff(i) > 0) and i[0] >= 0 and i[-1] < w * h      # distinct pixels of the frame
    assert np.array_equal(_pack(got), frame[i])
    # the same sample from run to run
    assert np.array_equal(idx, np.load(tmp_path / "b" / "framebuffer_index.npy"))
    assert np.array_equal(got, np.load(tmp_path / "b" / "framebuffer.npy"))


def test_dump_stays_within_64_mb_at_config5():
    import bench
    side = bench.CONFIG5_SIDE
    assert side * side > bench.DUMP_MAX_PIXELS
    assert bench.DUMP_MAX_PIXELS * (4 * 4 + 8) <= 64 * 1000 * 1000     # channels + indices
    assert 1024 * 1024 <= bench.DUMP_MAX_PIXELS                          # the N = 1 frame goes whole


def test_bench_help_lists_the_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_frame(tmp_path):
    from skybox_rt_amd import rt
    import bench
    side, steps = 128, 7
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                          "--warmup", "2", "--size", str(side), "--dump-outputs", str(tmp_path / "o")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout
    res = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res, key
    assert res["steps"] == steps and res["full"] is False
    assert res["ms_per_step"] > 0 and res["unit"] == "Mrays/s" and res["higher_is_better"] is True
    # value = rays of a frame per ms_per_step (the line rounds ms_per_step to 1e-5 ms)
    rays = res["config"]["rays_per_frame"]
    tol = 0.5e-5 / res["ms_per_step"] + 1e-5
    assert abs(res["value"] - rays / (res["ms_per_step"] * 1e-3) / 1e6) <= tol * res["value"]
    # nothing of --full
    assert res["series"] == {} and res["roofline"] is None and res["cpu_baseline"] is None
    assert res["config"]["kernel_ms"] is None and res["config"]["bvh_rebuild_ms"] is None
    got = np.load(tmp_path / "o" / "framebuffer.npy")
    assert got.dtype == np.float32 and got.shape == (side, side, 4)
    scene = rt.Scene.load(bench.SCENE)
    r = rt.Renderer(scene)
    try:
        r.configure(side, side, shadows=True, light=rt.DEFAULT_LIGHT, counters=False)
        r.render()
        assert np.array_equal(_pack(got), r.framebuffer())
    finally:
        r.close()
        scene.close()
