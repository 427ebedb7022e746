"""bench.py's plain run and `--dump-outputs DIR`: the last timed step's outputs as DIR/<name>.npy (float32 / float64,
at most 64 MB in all, fixed seeded samples of what does not fit), the same inputs from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONTRACT_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _fake_step(n, h, w, seed=0):
    """CPU stand-ins for one step's outputs: render, alpha, FlatGaussianParams with gradients, info."""
    from freegaussian_amd.viewdp import FlatGaussianParams

    g = torch.Generator().manual_seed(seed)
    params = FlatGaussianParams(n, "cpu")
    params.flat_grad.copy_(torch.randn(params.flat_grad.shape, generator=g))
    render = torch.rand(1, h, w, 3, generator=g)
    alpha = torch.rand(1, h, w, 1, generator=g)
    means2d = torch.zeros(1, n, 2)
    means2d.absgrad = torch.rand(1, n, 2, generator=g)
    info = {"means2d": means2d, "radii": torch.randint(0, 40, (1, n, 2), generator=g, dtype=torch.int32)}
    return render, alpha, params, info


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_writes_everything_whole_when_it_fits(tmp_path):
    import bench

    render, alpha, params, info = _fake_step(500, 24, 40)
    bench.dump_outputs(str(tmp_path), render, alpha, params, info)
    out = _load(tmp_path)
    assert "pixel_ids" not in out and "gaussian_ids" not in out
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    np.testing.assert_array_equal(out["render"], render[0].numpy())
    np.testing.assert_array_equal(out["alpha"], alpha[0].numpy())
    for name, v in params.grad_views.items():
        np.testing.assert_array_equal(out["grad_" + name], v.numpy())
    np.testing.assert_array_equal(out["means2d_absgrad"], info["means2d"].absgrad[0].numpy())
    np.testing.assert_array_equal(out["radii"], info["radii"][0].float().numpy())


def test_dump_samples_within_the_budget_and_repeats_its_sample(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    n, h, w = 4000, 120, 160
    for run in ("a", "b"):
        render, alpha, params, info = _fake_step(n, h, w)
        bench.dump_outputs(str(tmp_path / run), render, alpha, params, info)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= 200_000
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    pix, gid = a["pixel_ids"].astype(np.int64), a["gaussian_ids"].astype(np.int64)
    assert 0 < len(pix) < h * w and 0 < len(gid) < n
    assert (np.diff(pix) > 0).all() and (np.diff(gid) > 0).all()
    np.testing.assert_array_equal(a["render"], render[0].reshape(h * w, 3).numpy()[pix])
    np.testing.assert_array_equal(a["grad_colors"], params.grad_views["colors"].numpy()[gid])
    np.testing.assert_array_equal(a["radii"], info["radii"][0].float().numpy()[gid])


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    """Two plain runs with the same small arguments: the contract line (the requested number of timed steps, no --full
    extras) and outputs that agree run to run (identical inputs; the backward's atomics may reorder fp32 sums)."""
    outs = []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--settle-s", "0.2",
               "--n-gauss", "50000", "--width", "640", "--height", "360", "--dump-outputs", str(tmp_path / run)]  # fmt: skip
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-3000:]
        line = json.loads(res.stdout.strip().splitlines()[-1])
        assert all(k in line for k in CONTRACT_KEYS) and line["steps"] == 7 and line["ms_per_step"] > 0
        assert not {"roofline", "cpu_baseline", "clustered_layouts", "graphed", "stage_ms"} & line.keys()
        outs.append(_load(tmp_path / run))
    a, b = outs
    assert a.keys() == b.keys() and {"render", "alpha", "grad_means", "grad_colors", "radii"} <= a.keys()
    assert a["render"].shape == (360, 640, 3) and a["grad_means"].shape == (50000, 3)
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert float(np.abs(a["render"]).max()) > 0 and float(np.abs(a["grad_means"]).max()) > 0
    np.testing.assert_array_equal(a["radii"], b["radii"])
    for k in a:
        scale = max(float(np.abs(b[k]).max()), 1e-30)
        assert float(np.abs(a[k] - b[k]).max()) / scale < 1e-4, k
