"""The fused colour correction on the GPU (csrc/color_correct.hip through ops.color_correct and FG_FUSED_COLOR_CORRECT) against
the float64 restatement of its contract (color_correct_restatement.py) and, where every fit has full rank, against the
torch function it stands in for.  The bar is the project's one: 1e-4, absolute on values in [0, 1].

Regimes.  FULL RANK (natural and half-clipped images of 15 pixels and more): parity with both, conditioned -- before the GPU
is touched -- on every compared value lying at least 1e-5 from the two thresholds (a hundred times the fp32 apply error: no
pixel can then change its mask between implementations).  EXACTLY DEFICIENT (fewer than 10 pixels, a zero channel of img, a
saturated channel of ref, a constant image): parity with the restatement only, and equal ranks.  GREY (r = g = b: rank 3,
then near-deficient at noise level): no two solvers agree there, so properties only.  Everywhere: two runs are bit for bit
equal in out, warps and rank, and the inputs are unchanged."""
import pytest
import torch

import color_correct_restatement as R
import helpers
from freegaussian_amd import bilagrid, harness, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BAR = 1e-4
MARGIN = 1e-5


def _abs_err(a, b) -> float:
    v = float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())
    helpers._record("abs_err", v)
    return v


def _run(c, iters):
    """The fused call twice on fresh device copies: bit-equal runs, untouched inputs, the input's shape kept."""
    img, ref = c["img"].to(DEV), c["ref"].to(DEV)
    out, info = ops.color_correct(img, ref, num_iters=iters, return_info=True)
    again, info2 = ops.color_correct(img, ref, num_iters=iters, return_info=True)
    assert out.shape == c["img"].shape and out.dtype == torch.float32
    assert torch.equal(out, again) and torch.equal(info["warps"], info2["warps"]) and torch.equal(info["rank"], info2["rank"])
    assert torch.equal(img.cpu(), c["img"]) and torch.equal(ref.cpu(), c["ref"])
    assert tuple(info["warps"].shape) == (iters, 10, 3) and tuple(info["rank"].shape) == (iters, 3) and info["rank"].dtype == torch.int32
    assert torch.equal(ops.color_correct(img, ref, num_iters=iters), out)  # (without the info: the same image)
    return out.cpu(), info["warps"].cpu(), info["rank"].cpu().long()


# shapes: P = 15, 63, 64, 65, 255, 256, 257, 391, 4096, 33 x 130 and 4100 (two partial-sum chunks of 4096 pixels); the seeds
# are the first from 2 whose restatement meets the margin
FULL_RANK = [("natural", 3, 5, 2, 5), ("natural", 7, 9, 2, 5), ("natural", 8, 8, 2, 5), ("natural", 5, 13, 2, 5), ("natural", 15, 17, 2, 5),
             ("natural", 16, 16, 2, 5), ("natural", 1, 257, 2, 5), ("natural", 17, 23, 2, 5), ("natural", 64, 64, 3, 5),
             ("natural", 33, 130, 3, 5), ("natural", 41, 100, 2, 5), ("natural", 17, 23, 2, 1), ("natural", 17, 23, 2, 2),
             ("natural", 64, 64, 3, 1), ("natural", 64, 64, 3, 2), ("half_clipped", 7, 9, 2, 5), ("half_clipped", 17, 23, 2, 5),
             ("half_clipped", 64, 64, 3, 5), ("half_clipped", 64, 64, 3, 2), ("half_clipped", 41, 100, 2, 5)]  # fmt: skip


@pytest.mark.parametrize("kind,H,W,seed,iters", FULL_RANK)
def test_full_rank_parity_with_the_restatement_and_the_torch_function(monkeypatch, kind, H, W, seed, iters):
    monkeypatch.delenv("FG_FUSED_COLOR_CORRECT", raising=False)
    c = R.case(kind, H, W, seed, iters)
    assert c["margin"] >= MARGIN and int(c["rank"].min()) == 10  # the condition, on the restatement alone
    out, warps, rank = _run(c, iters)
    e_r = _abs_err(out, c["out"])
    e_t = _abs_err(out, bilagrid.color_correct(c["img"], c["ref"], num_iters=iters))  # (the torch function, on the host)
    print(f"{kind} {H}x{W} x{iters}: restatement {e_r:.3e}, torch {e_t:.3e}, margin {c['margin']:.3e}")
    assert torch.equal(rank, c["rank"])
    assert e_r <= BAR and e_t <= BAR


DEFICIENT = [("natural", 1, 1, 2, 5), ("natural", 1, 4, 2, 5), ("natural", 3, 3, 2, 5), ("natural", 1, 4, 2, 1), ("zero_img_channel", 17, 23, 2, 5),
             ("zero_img_channel", 41, 100, 3, 5), ("saturated_ref_channel", 17, 23, 2, 5), ("saturated_ref_channel", 41, 100, 2, 2),
             ("constant", 17, 23, 2, 5), ("constant", 41, 100, 2, 5)]  # fmt: skip


@pytest.mark.parametrize("kind,H,W,seed,iters", DEFICIENT)
def test_exactly_deficient_parity_with_the_restatement(kind, H, W, seed, iters):
    c = R.case(kind, H, W, seed, iters)
    assert c["margin"] >= MARGIN and int(c["rank"].min()) < 10
    out, warps, rank = _run(c, iters)
    e_r = _abs_err(out, c["out"])
    print(f"{kind} {H}x{W} x{iters}: restatement {e_r:.3e}, ranks {rank.tolist()}")
    assert torch.equal(rank, c["rank"])
    assert e_r <= BAR
    if kind == "zero_img_channel":  # no unmasked pixel in red: w = 0 there, and the zero columns carry no weight elsewhere
        assert not warps[:, :, 0].any() and not warps[:, [0, 1, 2, 6], :].any() and not out[..., 0].any()
    if kind == "saturated_ref_channel":
        assert not warps[:, :, 1].any() and not out[..., 1].any()


@pytest.mark.parametrize("H,W,seed", [(17, 23, 2), (41, 100, 3)])
def test_grey_image_properties(H, W, seed):
    c = R.case("grey", H, W, seed, 5)
    out, warps, rank = _run(c, 5)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(warps).all())
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    assert rank[0].tolist() == [3, 3, 3] and int(rank.min()) >= 1 and int(rank.max()) <= 10


def test_layouts_knob_and_argument_errors(monkeypatch):
    c = R.case("natural", 17, 23, 2, 5)
    img, ref = c["img"].to(DEV), c["ref"].to(DEV)
    base = ops.color_correct(img, ref)
    # a non-contiguous input gives the contiguous result; any leading shape
    wide = torch.zeros(17, 23, 4, device=DEV)
    wide[..., :3] = img
    assert not wide[..., :3].is_contiguous() and torch.equal(ops.color_correct(wide[..., :3], ref), base)
    assert torch.equal(ops.color_correct(img, ref.permute(1, 0, 2).contiguous().permute(1, 0, 2)), base)
    flat = ops.color_correct(img.reshape(-1, 3), ref.reshape(-1, 3))
    assert tuple(flat.shape) == (391, 3) and torch.equal(flat.reshape(17, 23, 3), base)
    assert torch.equal(ops.color_correct(img[None], ref[None])[0], base)
    # the knob: unset = the torch ops (ops.color_correct is not reached), 1 = the fused call
    monkeypatch.setenv("FG_FUSED_COLOR_CORRECT", "1")
    assert bilagrid.fused_color_correct_applies(img, ref, 5, 0.5 / 255)
    assert torch.equal(bilagrid.color_correct(img, ref), base)
    assert not bilagrid.fused_color_correct_applies(img, ref.cpu(), 5, 0.5 / 255) and not bilagrid.fused_color_correct_applies(img.double(), ref.double(), 5, 0.5 / 255)
    assert not bilagrid.fused_color_correct_applies(img, ref, 9, 0.5 / 255) and not bilagrid.fused_color_correct_applies(img, ref, 5, 0.5)
    wants = img.clone().requires_grad_(True)
    assert not bilagrid.fused_color_correct_applies(wants, ref, 5, 0.5 / 255)
    with torch.no_grad():
        assert bilagrid.fused_color_correct_applies(wants, ref, 5, 0.5 / 255)
    monkeypatch.setattr(ops, "color_correct", None)  # (not callable: reaching it would raise)
    monkeypatch.delenv("FG_FUSED_COLOR_CORRECT")
    assert _abs_err(bilagrid.color_correct(img, ref), base) <= BAR
    monkeypatch.undo()
    for bad in (dict(num_iters=0), dict(num_iters=9), dict(eps=0.0), dict(eps=0.5), dict(num_iters=2.0)):
        with pytest.raises(ValueError):
            ops.color_correct(img, ref, **bad)
    with pytest.raises(ValueError):
        ops.color_correct(img.double(), ref.double())
    with pytest.raises(ValueError):
        ops.color_correct(img[..., :2], ref[..., :2])


def test_model_metrics_with_the_knob_on(monkeypatch):
    """A tiny scene (300 Gaussians, 48 x 64) rendered on the GPU; cc_psnr and cc_ssim of get_image_metrics_and_images with the
    knob on against the values computed from the restatement's image: |delta mse| <= 2 x 1e-4 x mean|cc - gt| + 1e-8 (the
    parity bar carried through the MSE: d(e^2) = 2 |e| de), cc_ssim within 1e-4."""
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    W, H, n = 64, 48, 300
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, color_corrected_metrics=True)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-2.2)
    with torch.no_grad():
        model.gauss_params["scales"].fill_(-2.2)
    model.step = 4000
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1  # OpenCV -> OpenGL camera axes
    cam = Camera(c2w[None, :3], 56.0, 60.0, W / 2, H / 2, W, H, times=torch.tensor([[0.4]]))
    model = model.to(DEV)
    monkeypatch.setenv("FG_FUSED_COLOR_CORRECT", "1")
    model.eval()
    outputs = model.get_outputs_for_camera(cam)
    rgb = outputs["rgb"].detach().cpu()
    assert float(rgb.std()) > 0.02  # (something was rendered)
    noise = torch.randn(H, W, 3, generator=torch.Generator().manual_seed(1)) * 0.01
    gt = torch.clamp(rgb @ torch.tensor([[0.9, 0.05, 0.0], [0.02, 0.85, 0.03], [0.0, 0.04, 0.8]]).T + 0.04 + 0.05 * rgb * rgb + noise, 0, 1)
    batch = {"image": gt.to(DEV)}
    metrics, images = model.get_image_metrics_and_images(outputs, batch)
    assert set(metrics) == {"psnr", "ssim", "cc_psnr", "cc_ssim"} and tuple(images["img"].shape) == (H, 2 * W, 3)
    want = R.restate(rgb, gt, 5)
    cc = want["out"]
    mse_want, mse_got = float(((cc - gt).double() ** 2).mean()), 10.0 ** (-metrics["cc_psnr"] / 10.0)
    bound = 2 * BAR * float((cc - gt).abs().mean()) + 1e-8
    chw = lambda t: t.permute(2, 0, 1)[None]  # noqa: E731
    ssim_want = float(harness.ssim(chw(gt), chw(cc)))
    print(f"cc mse {mse_got:.6e} against {mse_want:.6e} (bound {bound:.3e}); cc_ssim {metrics['cc_ssim']:.6f} against {ssim_want:.6f}; "
          f"margin {want['margin']:.3e}, ranks {want['rank'].tolist()}")  # fmt: skip
    helpers._record("abs_err", abs(mse_got - mse_want))
    assert abs(mse_got - mse_want) <= bound
    assert abs(metrics["cc_ssim"] - ssim_want) <= BAR
    assert metrics["cc_psnr"] > metrics["psnr"]
    # the harness functions around it: the same numbers, num_rays, and training mode again
    model.train()
    one, _ = harness.eval_image(model, cam, batch)
    assert model.training and one["num_rays"] == H * W and one["cc_psnr"] == pytest.approx(metrics["cc_psnr"], abs=1e-5) and one["cc_ssim"] == pytest.approx(metrics["cc_ssim"], abs=1e-6)
    avg = harness.average_image_metrics(model, [(cam, batch)] * 2, get_std=True)
    assert model.training and avg["cc_psnr"] == pytest.approx(metrics["cc_psnr"], abs=1e-5) and avg["cc_psnr_std"] < 1e-4 and avg["fps"] > 0
