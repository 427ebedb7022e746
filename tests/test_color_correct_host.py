"""The fused colour correction (csrc/color_correct.hip, ops.color_correct, FG_FUSED_COLOR_CORRECT) and the evaluation
metrics built on it (FreeGaussianModel.get_image_metrics_and_images, harness.eval_image / average_image_metrics), as far as
a machine without a GPU can check them: the float64 restatement the GPU tests compare against is pinned to the torch path
on the CPU; the threshold semantics are decided against the torch path; the symbols are declared, bound and exported; the
query and the argument validation answer before any launch; the knob parses and CPU tensors never reach the fused call;
the solver the kernel runs is checked on the host against numpy's least squares."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import color_correct_restatement as R
from freegaussian_amd import _lib, bilagrid, harness, ops
from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fg_color_correct_workspace_bytes", "fg_color_correct")
INVALID, WORKSPACE, UNSUPPORTED = -1, -3, -4


@pytest.mark.parametrize("kind,H,W,seed,iters", [("natural", 3, 5, 2, 5), ("natural", 17, 23, 2, 5), ("natural", 64, 64, 2, 2),
                                                 ("natural", 135, 240, 2, 5), ("half_clipped", 64, 64, 2, 5)])  # fmt: skip
def test_restatement_matches_the_torch_path_on_the_cpu(monkeypatch, kind, H, W, seed, iters):
    """Full-rank regime: within 1e-6, ten times the 1.2e-7 measured when the contract was drawn up."""
    monkeypatch.delenv("FG_FUSED_COLOR_CORRECT", raising=False)
    c = R.case(kind, H, W, seed, iters)
    assert int(c["rank"].min()) == 10
    out = bilagrid.color_correct(c["img"], c["ref"], num_iters=iters)
    err = float((out - c["out"]).abs().max())
    print(f"restatement against the torch path, {kind} {H}x{W} x{iters}: {err:.3e}, margin {c['margin']:.3e}")
    assert err <= 1e-6


def _threshold_pixels(eps):
    """40 pixels in the open middle of the range, then single pixels whose red value sits at lo, at hi and at their fp32
    neighbours on both sides, with a red ref far off the trend: including one visibly moves the red fit."""
    rng = np.random.default_rng(7)
    ref = rng.uniform(0.2, 0.8, (40, 3)).astype(np.float32)
    img = (0.9 * ref + 0.03 + rng.normal(0, 0.005, (40, 3))).astype(np.float32)
    lo, hi = np.float32(eps), np.float32(1.0 - eps)
    zero, two = np.float32(0), np.float32(2)
    edges = [lo, np.nextafter(lo, zero), np.nextafter(lo, two), hi, np.nextafter(hi, zero), np.nextafter(hi, two)]
    cases = []
    for e in edges:
        i, r = img.copy(), ref.copy()
        i[7, 0], r[7, 0] = e, 0.5 if e < 0.5 else 0.05  # (the trend wants ~0 at lo and ~1 at hi)
        cases.append((torch.from_numpy(i), torch.from_numpy(r)))
    return cases


def test_thresholds_are_fp32_comparisons_against_the_rounded_scalars(monkeypatch):
    """Decides `unclipped`: torch compares a float32 tensor with a Python scalar in fp32, against the scalar rounded to
    fp32.  The default eps cannot tell (its lo rounds up and its hi rounds down, so fp32 and float64 comparisons agree on
    every fp32 value); eps values whose lo rounds DOWN or whose hi rounds UP can, and there the float64 counter-model
    visibly differs from the torch path while the fp32 restatement matches it."""
    monkeypatch.delenv("FG_FUSED_COLOR_CORRECT", raising=False)
    told = 0
    for eps in (0.5 / 255, 0.01, 0.003, 0.02, 0.004, 0.1):
        tells = float(np.float32(eps)) < eps or float(np.float32(1.0 - eps)) > 1.0 - eps
        for img, ref in _threshold_pixels(eps):
            want = bilagrid.color_correct(img, ref, num_iters=1, eps=eps)
            got = R.restate(img, ref, 1, eps)["out"]
            assert float((got - want).abs().max()) <= 1e-6, eps
        if tells:
            worst = max(float((R.restate(i, r, 1, eps, compare="fp64")["out"] - bilagrid.color_correct(i, r, num_iters=1, eps=eps)).abs().max())
                        for i, r in _threshold_pixels(eps))  # fmt: skip
            print(f"eps {eps}: the float64-comparison model is off the torch path by {worst:.3e}")
            assert worst > 1e-3
            told += 1
    assert told >= 2


def test_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "fgraster.h")).read()
    assert "#define FG_ABI_VERSION 14" in text and "#define FG_ABI_MINOR 1 " in text
    assert _lib.ABI_VERSION == 14 and _lib.ABI_MINOR == 1
    by_name = text[text.index("BY NAME") : text.index("#define FG_COUNT_OUT_WORDS")]
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    exported = set(re.findall(r" T (fg_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)))
    for name in NAMES:
        assert name in by_name, name
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _lib.SIGNATURES and name in exported and getattr(lib, name) is not None
    assert "fg_debug_color_correct_solve" in _lib._EXTRA and "fg_debug_color_correct_solve" in exported
    assert "fg_debug_color_correct_solve" not in text
    for macro, want in (("FG_COLOR_CORRECT_MAX_ITERS", "8"), ("FG_COLOR_CORRECT_CHUNK_PIXELS", "4096"), ("FG_COLOR_CORRECT_MAX_CHUNKS", "2048"),
                        ("FG_COLOR_CORRECT_RCOND", "1e-12")):  # fmt: skip
        m = re.search(rf"^#define {macro} (\S+)", text, flags=re.M)
        assert m and m.group(1) == want, macro
    assert _lib.COLOR_CORRECT_MAX_ITERS == 8 and R.RCOND == 1e-12
    srcs = re.search(r"^SRCS := (.*)$", open(os.path.join(ROOT, "freegaussian_amd", "csrc", "Makefile")).read(), flags=re.M).group(1)
    assert "color_correct.hip" in srcs.split()


def _want_bytes(P):
    return 2048 + min(-(-P // 4096), 2048) * 3 * 128 * 8


def test_workspace_query_is_pure_monotone_and_zero_outside_the_range():
    q = _lib.load().fg_color_correct_workspace_bytes
    sizes = [1, 2, 3, 4, 255, 4095, 4096, 4097, 8192, 8193, 480 * 270, 1920 * 1080, 4096 * 2048, 4096 * 2048 + 1, 3 * 4096 * 2048 + 17,
             16384 * 16384 - 1, 16384 * 16384]  # fmt: skip
    last = 0
    for P in sizes:
        for iters in (1, 5, 8):
            assert q(P, iters) == q(P, iters) == _want_bytes(P), (P, iters)
        assert q(P, 5) >= last
        last = q(P, 5)
    assert q(4096, 5) == 2048 + 3072 and q(4097, 5) == 2048 + 2 * 3072 and q(1920 * 1080, 5) == 2048 + 507 * 3072
    assert q(16384 * 16384, 5) == 2048 + 2048 * 3072  # the chunk count stops at FG_COLOR_CORRECT_MAX_CHUNKS
    for P, iters in ((0, 5), (-1, 5), (-(1 << 40), 5), (16384 * 16384 + 1, 5), (1 << 40, 5), (100, 0), (100, -1), (100, 9), (100, 1 << 30)):
        assert q(P, iters) == 0, (P, iters)


def test_argument_validation_answers_before_any_launch():
    lib = _lib.load()
    cc, q = lib.fg_color_correct, lib.fg_color_correct_workspace_bytes
    big = 1 << 40
    img, ref, out, warps, rank, ws = (4096 + (i << 24) for i in range(6))  # (addresses nobody reads: every call returns first)
    P, eps = 37 * 53, 0.5 / 255
    image, need = P * 12, q(P, 5)
    assert cc(P, None, ref, 5, eps, out, warps, rank, ws, big, None) == INVALID
    assert cc(P, img, None, 5, eps, out, warps, rank, ws, big, None) == INVALID
    assert cc(P, img, ref, 5, eps, None, warps, rank, ws, big, None) == INVALID
    for bad_P in (0, -1, 16384 * 16384 + 1, 1 << 40):
        assert cc(bad_P, img, ref, 5, eps, out, warps, rank, ws, big, None) == UNSUPPORTED
    for bad_iters in (0, -1, 9, 1 << 30):
        assert cc(P, img, ref, bad_iters, eps, out, warps, rank, ws, big, None) == UNSUPPORTED
    for bad_eps in (0.0, -0.1, 0.5, 0.75, float("nan"), float("inf")):
        assert cc(P, img, ref, 5, bad_eps, out, warps, rank, ws, big, None) == UNSUPPORTED
    assert cc(P, img, ref, 5, eps, img, warps, rank, ws, big, None) == INVALID  # out is img
    assert cc(P, img, ref, 5, eps, ref, warps, rank, ws, big, None) == INVALID  # out is ref
    assert cc(P, img, ref, 5, eps, img + image - 4, warps, rank, ws, big, None) == INVALID  # ... by the last float
    assert cc(P, img, ref, 5, eps, ref - image + 4, warps, rank, ws, big, None) == INVALID
    assert cc(P, img, ref, 5, eps, out, warps, rank, None, big, None) == INVALID
    assert cc(P, img, ref, 5, eps, out, warps, rank, ws + 8, big, None) == INVALID  # misaligned
    assert cc(P, img, ref, 5, eps, out, warps, rank, out, big, None) == INVALID  # the workspace is out
    assert cc(P, img, ref, 5, eps, out, warps, rank, out - need + 16, big, None) == INVALID  # ... by its last bytes
    assert cc(P, img, ref, 5, eps, out, warps, rank, img, big, None) == INVALID  # the workspace is an input
    assert cc(P, img, ref, 5, eps, out, out, rank, ws, big, None) == INVALID  # warps inside out
    assert cc(P, img, ref, 5, eps, out, warps, ws, ws, big, None) == INVALID  # rank inside the workspace
    assert cc(P, img, ref, 5, eps, out, warps, warps, ws, big, None) == INVALID  # rank is warps
    for nbytes in (0, 1, need - 1):
        assert cc(P, img, ref, 5, eps, out, warps, rank, ws, nbytes, None) == WORKSPACE
    # the order: a null pointer before the range, the range before the workspace
    assert cc(0, None, ref, 0, eps, out, None, None, None, 0, None) == INVALID
    assert cc(0, img, ref, 5, eps, out, None, None, None, 0, None) == UNSUPPORTED


def test_knob_parses_and_cpu_tensors_never_take_the_fused_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("ops.color_correct reached")

    img, ref = R.natural(9, 7, 3)
    monkeypatch.delenv("FG_FUSED_COLOR_CORRECT", raising=False)
    assert bilagrid.fused_color_correct() is False
    base = bilagrid.color_correct(img, ref)
    with pytest.raises(_lib.FgRasterError):
        ops.color_correct(img, ref)
    with pytest.raises(ValueError):
        ops.color_correct(img[..., :2], ref[..., :2])
    with pytest.raises(ValueError):
        ops.color_correct(img, ref[:4])
    monkeypatch.setattr(ops, "color_correct", boom)
    for knob, want in (("0", False), ("1", True)):
        monkeypatch.setenv("FG_FUSED_COLOR_CORRECT", knob)
        assert bilagrid.fused_color_correct() is want
        assert bilagrid.fused_color_correct_applies(img, ref, 5, 0.5 / 255) is False  # CPU tensors
        assert torch.equal(bilagrid.color_correct(img, ref), base)
    for bad in ("", "yes", "2", "true", " 1"):
        monkeypatch.setenv("FG_FUSED_COLOR_CORRECT", bad)
        with pytest.raises(ValueError, match="FG_FUSED_COLOR_CORRECT"):
            bilagrid.fused_color_correct()
        with pytest.raises(ValueError, match="FG_FUSED_COLOR_CORRECT"):
            bilagrid.color_correct(img, ref)
    assert ops.color_correct_supported(300, 5, 0.5 / 255) and not ops.color_correct_supported(300, 9, 0.5 / 255)
    assert not ops.color_correct_supported(300, 5, 0.5) and not ops.color_correct_supported(300, 5.0, 0.1)


# ---- the solver the solve kernel runs, on the host ---------------------------------------------------------------------
def _solve(G, r):
    G, r = np.ascontiguousarray(G, dtype=np.float64), np.ascontiguousarray(r, dtype=np.float64)
    w, rank = np.zeros(10), ctypes.c_int32(-7)
    rc = _lib.load().fg_debug_color_correct_solve(G.ctypes.data, r.ctypes.data, w.ctypes.data, ctypes.addressof(rank))
    assert rc == 0
    return w, rank.value


def _rows(n, seed, zero_channel=False):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.05, 0.95, (n, 3))
    if zero_channel:
        x[:, 0] = 0.0
    A = R.features(torch.from_numpy(x)).numpy()
    return A, rng.uniform(0.05, 0.95, n)


@pytest.mark.parametrize("name,n,zero,want_rank", [("full rank", 50, False, 10), ("zero columns", 50, True, 6), ("no rows", 0, False, 0),
                                                   ("1 row", 1, False, 1), ("4 rows", 4, False, 4), ("9 rows", 9, False, 9)])  # fmt: skip
def test_host_solver_against_numpy_least_squares(name, n, zero, want_rank):
    """fg_cc_solve on the Gram against numpy.linalg.lstsq on the rows, float64: the fitted values A w agree to 1e-9 (they
    are what every least-squares solution shares) and the ranks are equal."""
    A, b = _rows(n, 11 + n, zero)
    w, rank = _solve(A.T @ A, A.T @ b)
    if n == 0:
        assert rank == 0 and not w.any()
        return
    w_np, _, rank_np, _ = np.linalg.lstsq(A, b, rcond=None)
    err = float(np.abs(A @ w - A @ w_np).max())
    print(f"{name}: fitted values within {err:.3e}, rank {rank} (numpy {rank_np})")
    assert rank == rank_np == want_rank == R.numerical_rank(torch.from_numpy(A))
    assert err <= 1e-9
    if zero:
        assert not w[[0, 1, 2, 6]].any()  # the zero columns: x0 x0, x0 x1, x0 x2, x0


def _normal_equation_model(img, ref, num_iters):
    """The kernel's arithmetic restated on the host: fp32 features, float64 Gram of the unmasked rows, the library's own
    solver, fp32 weights, fp32 apply."""
    x, y = img.reshape(-1, 3), ref.reshape(-1, 3)
    lo, hi = R.thresholds(0.5 / 255)
    unclipped = lambda z: (z >= lo) & (z <= hi)  # noqa: E731
    mask0 = unclipped(x)
    ranks = torch.zeros(num_iters, 3, dtype=torch.int64)
    for k in range(num_iters):
        A = R.features(x)
        W = torch.zeros(10, 3)
        for ch in range(3):
            m = mask0[:, ch] & unclipped(x[:, ch]) & unclipped(y[:, ch])
            rows, b = A[m].double().numpy(), y[m, ch].double().numpy()
            w, ranks[k, ch] = _solve(rows.T @ rows, rows.T @ b)
            W[:, ch] = torch.from_numpy(w).float()
        x = torch.clamp(A @ W, 0, 1)
    return x.reshape(img.shape), ranks


@pytest.mark.parametrize("kind,H,W,seed", [("natural", 64, 64, 3), ("half_clipped", 64, 64, 3), ("natural", 1, 1, 2), ("natural", 1, 4, 2),
                                           ("natural", 3, 3, 2), ("zero_img_channel", 17, 23, 2), ("saturated_ref_channel", 17, 23, 2),
                                           ("constant", 17, 23, 2)])  # fmt: skip
def test_normal_equation_model_matches_the_restatement(kind, H, W, seed):
    """Normal equations + the library's solver against the gelsd restatement, in the full-rank and in the exactly deficient
    regime: equal ranks, and images ten times inside the 1e-4 parity bar."""
    c = R.case(kind, H, W, seed, 5)
    out, ranks = _normal_equation_model(c["img"], c["ref"], 5)
    err = float((out - c["out"]).abs().max())
    print(f"normal-equation model against the restatement, {kind} {H}x{W}: {err:.3e}, ranks {ranks.tolist()}")
    assert torch.equal(ranks, c["rank"])
    assert err <= 1e-5


# ---- the model method and the harness functions, on a CPU model ---------------------------------------------------------
def _cpu_model(cc: bool):
    cfg = FreeGaussianModelConfig(color_corrected_metrics=cc, num_downscales=0, background_color="black")
    return FreeGaussianModel(cfg, num_points=16, init_scales=-4.0)


def _view(seed, H=16, W=20):
    img, ref = R.natural(H, W, seed)
    cam = Camera(torch.eye(4)[None, :3], 10.0, 10.0, W / 2, H / 2, W, H, times=torch.zeros(1, 1))
    return cam, {"rgb": img, "background": torch.zeros(3)}, {"image": ref}


@pytest.mark.parametrize("cc", [False, True])
def test_get_image_metrics_and_images_on_a_cpu_model(monkeypatch, cc):
    monkeypatch.delenv("FG_FUSED_COLOR_CORRECT", raising=False)
    m = _cpu_model(cc)
    _, outputs, batch = _view(5)
    metrics, images = m.get_image_metrics_and_images(outputs, batch)
    assert set(metrics) == ({"psnr", "ssim", "cc_psnr", "cc_ssim"} if cc else {"psnr", "ssim"})
    assert all(type(v) is float for v in metrics.values())
    assert not any("lpips" in k for k in metrics)
    pred, gt = outputs["rgb"], batch["image"]
    chw = lambda t: t.permute(2, 0, 1)[None]  # noqa: E731
    assert metrics["psnr"] == float(harness.psnr(pred, gt)) == float(m.get_metrics_dict(outputs, batch)["psnr"])
    assert metrics["ssim"] == float(harness.ssim(chw(gt), chw(pred)))
    if cc:
        fixed = bilagrid.color_correct(pred, gt)
        assert metrics["cc_psnr"] == float(harness.psnr(fixed, gt)) and metrics["cc_ssim"] == float(harness.ssim(chw(gt), chw(fixed)))
        assert metrics["cc_psnr"] > metrics["psnr"] + 3
    assert set(images) == {"img"} and tuple(images["img"].shape) == (16, 40, 3)
    assert torch.equal(images["img"][:, :20], gt) and torch.equal(images["img"][:, 20:], pred)
    # an alpha channel is composited over the step's background first
    rgba = torch.cat([gt, torch.full((16, 20, 1), 0.5)], dim=-1)
    over = m.get_image_metrics_and_images({"rgb": pred, "background": torch.ones(3)}, {"image": rgba})[0]
    assert over["psnr"] == float(harness.psnr(pred, 0.5 * gt + 0.5))


def test_control_model_inherits_the_method():
    from freegaussian_amd.model import FreeGaussianControlModel

    assert FreeGaussianControlModel.get_image_metrics_and_images is FreeGaussianModel.get_image_metrics_and_images


def test_harness_eval_image_and_average_image_metrics(monkeypatch):
    monkeypatch.delenv("FG_FUSED_COLOR_CORRECT", raising=False)
    m = _cpu_model(True)
    views, rendered, modes = [], {}, []
    for seed in (5, 6, 7):
        cam, outputs, batch = _view(seed)
        rendered[id(cam)] = outputs
        views.append((cam, batch))

    def canned(camera):  # (a CPU model has no rasteriser: the render is canned, the mode it is asked in recorded)
        modes.append(m.training)
        return rendered[id(camera)]

    monkeypatch.setattr(m, "get_outputs_for_camera", canned)
    m.train()
    per_view = [harness.eval_image(m, cam, batch) for cam, batch in views]
    assert m.training and modes == [False] * 3
    for (metrics, images), (cam, batch) in zip(per_view, views):
        assert metrics["num_rays"] == 16 * 20 and tuple(images["img"].shape) == (16, 40, 3)
        assert {k: v for k, v in metrics.items() if k != "num_rays"} == m.get_image_metrics_and_images(rendered[id(cam)], batch)[0]
    avg = harness.average_image_metrics(m, views)
    assert m.training and modes == [False] * 6
    assert set(avg) == {"psnr", "ssim", "cc_psnr", "cc_ssim", "num_rays_per_sec", "fps"}
    for key in ("psnr", "ssim", "cc_psnr", "cc_ssim"):
        assert avg[key] == float(torch.mean(torch.tensor([p[0][key] for p in per_view])))
    assert avg["num_rays_per_sec"] > 0 and avg["fps"] > 0
    m.eval()
    both = harness.average_image_metrics(m, views, get_std=True)
    assert m.training  # (the reference ends in train(), whatever the mode was)
    assert set(both) == set(avg) | {f"{k}_std" for k in avg}
    for key in ("psnr", "ssim", "cc_psnr", "cc_ssim"):
        std, mean = torch.std_mean(torch.tensor([p[0][key] for p in per_view]))
        assert both[key] == float(mean) and both[f"{key}_std"] == float(std)
    with pytest.raises(AssertionError):
        harness.average_image_metrics(m, [])
