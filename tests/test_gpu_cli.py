"""The drop-in CLI end to end on the GPU: `ray <scene.json> <out.png> [--paper]`
(raytracer/src/main.cpp:42-94) renders through librtamd and writes an 8-bit
PNG; the image must equal the CPU oracle's framebuffer after the reference's
toByte (core.h:313-316), up to rounding flips of channels that sit within
1e-5 of a .5 boundary (8-bit comparison is not a stable parity
check, so the bar is <= 1 level and >= 99.9 % exact)."""
import json
import os
import subprocess

import numpy as np
import pytest

import fp32_bars as B
import scenes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY = os.path.join(REPO, "raytracing-project_amd", "bin", "ray")


def _png(path):
    from PIL import Image

    return np.asarray(Image.open(path).convert("RGB"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["penguin", "pokeballs", "snorlax"])
@pytest.mark.parametrize("paper", [False, True])
def test_cli_png_matches_oracle(gpu, tmp_path, name, paper):
    scene = scenes.with_dpi(scenes.load_example(name), 24)
    js = tmp_path / f"{name}.json"
    js.write_text(json.dumps(scene))
    out = tmp_path / f"{name}.png"
    args = [RAY, str(js), str(out)] + (["--paper"] if paper else []) + ["--threads", "4"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    sc = gpu.load_scene_from_json_text(json.dumps(scene))
    W, H = sc.width, sc.height
    assert f"Wrote {out} ({W}x{H})" in r.stdout
    assert ("(paper mode)" in r.stdout) == paper
    img = _png(out)
    assert img.shape == (H, W, 3)
    ref, _ = gpu.oracle_render(sc, W, H, 1 if paper else 0, threads=8)
    want = gpu.to_rgb8(ref)
    d = np.abs(img.astype(int) - want.astype(int))
    assert d.max() <= 1
    assert float(np.mean(d == 0)) >= 0.999


@pytest.mark.gpu
def test_cli_fp32_option(gpu, tmp_path):
    scene = scenes.with_dpi(scenes.load_example("penguin"), 24)
    js = tmp_path / "p.json"
    js.write_text(json.dumps(scene))
    out = tmp_path / "p.png"
    r = subprocess.run([RAY, str(js), str(out), "--fp32", "--stats"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    sc = gpu.load_scene_from_json_text(json.dumps(scene))
    ref, _ = gpu.oracle_render(sc, sc.width, sc.height, 0, threads=8)
    d = np.abs(_png(out).astype(int) - gpu.to_rgb8(ref).astype(int))
    assert float(np.mean(d <= 1)) >= 0.99   # non-parity fast path: near, not equal
    # ... and pixel by pixel: each byte within its pixel's stability bar (tests/fp32_bars.py), one level for
    # toByte's own rounding, on every pixel the bar constrains
    _, bar, unconstrained = B.standard_bars(gpu, json.dumps(scene), None, B.seed_of("small/penguin"))
    over = (d.max(axis=2) > np.ceil(255 * bar) + 1) & ~unconstrained
    print(f"  ray --fp32 penguin: {over.size} pixels, {float(unconstrained.mean()):.4%} unconstrained, {int(over.sum())} over "
          f"ceil(255 bar) + 1, largest byte difference on a constrained pixel {int(d.max(axis=2)[~unconstrained].max())}")
    assert not over.any(), np.argwhere(over)[:6].tolist()
