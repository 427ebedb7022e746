"""The fused bilateral-grid slice on the GPU (csrc/bilagrid.hip through ops.bilagrid_apply and bilagrid.apply_to_render with
FG_FUSED_BILAGRID=1) against the float64 restatement of tests/bilagrid_restatement.py, at the project's one bar:
max |a - b| / max |b| <= 1e-4 per array.  Inputs: a seeded draw repaired before any path sees it (no pixel within 1e-3 of
a level node), with exactly black, exactly white and out-of-range pixels placed on purpose; no pixel is excluded from any
comparison.  Shapes: the smallest at which the kernels can still go wrong (see each test)."""
import functools

import numpy as np
import pytest
import torch

import bilagrid_restatement as R
from freegaussian_amd import _lib, bilagrid, ops
from freegaussian_amd.bilagrid import BilateralGrid
from helpers import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _t(a, **kw):
    return torch.from_numpy(np.array(a)).to(DEV, **kw)


def _run(c, want_rgb=True, want_grids=True, grids=None):
    """ops.bilagrid_apply forward + backward on a case's inputs -> (out, v_rgb or None, v_grids or None)."""
    grids = _t(c["grids"] if grids is None else grids).requires_grad_(want_grids)
    rgb = _t(c["rgb"]).requires_grad_(want_rgb)
    out = ops.bilagrid_apply(grids, c["cam"], rgb)
    if want_rgb or want_grids:
        out.backward(_t(c["v_out"]))
    return out.detach(), rgb.grad, grids.grad


def _check(c, out, v_rgb, v_grids):
    errs = {"out": rel_err(out, _t(c["out"]))}
    if v_rgb is not None:
        errs["v_rgb"] = rel_err(v_rgb, _t(c["v_rgb"]))
    if v_grids is not None:
        errs["v_grid"] = rel_err(v_grids[c["cam"]], _t(c["v_grid"]))
        for i in range(v_grids.shape[0]):
            if i != c["cam"]:
                assert float(v_grids[i].abs().max()) == 0.0  # exactly zero: the other cameras' blocks
    print("fused against float64:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(e <= REL_TOL for e in errs.values()), errs


@functools.lru_cache(maxsize=None)
def _multi_partial_shape():
    """The smallest odd square-ish image whose backward forms MORE THAN ONE partial block per grid node and takes its second
    pass over several chunks, for the grid (X 4, Y 3, W 3): found from the workspace query, whose size is (chunks of the
    largest cell) x GL x 48 x cells x 4 bytes -- a cell's pixels are summed in chunks of FG_BILAGRID_CHUNK_PIXELS.  A coarse
    grid keeps the image small: the search ends at 65 x 97, where the three x cells are 32, 32 and 33 pixels wide and the
    two y cells 32 and 33 high (far below the 540 x 960 the default grid would need) -- the 32 x 32 cell has exactly one
    full chunk, the others (1056 and 1089 pixels) a full one and a nearly empty second one."""
    lib = _lib.load()
    GX, GY, GL = 4, 3, 3
    per_chunk = GL * 48 * (GX - 1) * (GY - 1) * 4
    for H in range(33, 541, 2):
        W = (3 * H // 2) | 1  # (odd too)
        if lib.fg_bilagrid_bwd_workspace_bytes(H, W, GX, GY, GL) // per_chunk >= 2:
            assert H <= 540 and W <= 960
            return H, W, GX, GY, GL
    raise AssertionError("no multi-partial shape below 540 x 960")


def test_odd_image_odd_grid_camera_one_of_three():
    """37 x 53, grid (X 5, Y 4, W 3), camera 1 of 3 non-identity grids: everything odd, nothing a multiple of anything.  The
    other two blocks of the grids' gradient are exactly zero, and the result does not depend on the other cameras' grids."""
    c = R.case(37, 53, 5, 4, 3, 3, 1)
    assert R.clear_of_knife_edges(c["rgb"], 3)
    out, v_rgb, v_grids = _run(c)
    _check(c, out, v_rgb, v_grids)
    other = np.array(c["grids"])
    other[0] += 5.0
    other[2] = -other[2]
    out2, v_rgb2, v_grids2 = _run(c, grids=other)
    assert torch.equal(out, out2) and torch.equal(v_rgb, v_rgb2) and torch.equal(v_grids, v_grids2)


def test_default_grid():
    """96 x 160 with the default grid (16, 16, 8): cells of 10-11 x 6-7 pixels, one chunk each, a row segment spans every x
    node."""
    c = R.case(96, 160, 16, 16, 8)
    assert R.clear_of_knife_edges(c["rgb"], 8)
    _check(c, *_run(c))


def test_fewer_pixels_than_grid_nodes():
    """12 x 14 with the grid (16, 16, 8): cells without a pixel, nodes no pixel reaches -- exactly 0.0 there, the bar
    elsewhere."""
    c = R.case(12, 14, 16, 16, 8)
    out, v_rgb, v_grids = _run(c)
    _check(c, out, v_rgb, v_grids)
    unreached = _t((np.array(c["v_grid"]) == 0.0).all(axis=0))  # [GL,GY,GX]: nodes whose twelve sums are all empty
    assert int(unreached.sum()) > 0 and bool((v_grids[0][:, unreached] == 0.0).all())
    # (14 pixels over 15 x cells, 12 over 15 y cells: cells without a pixel exist -- their workgroups write no partial block
    # and the sum pass reads none)
    x_cells = {min(px * 15 // 13, 14) for px in range(14)}
    y_cells = {min(py * 15 // 11, 14) for py in range(12)}
    assert len(x_cells) < 15 and len(y_cells) < 15


def test_multi_partial_shape_takes_the_second_pass():
    """See _multi_partial_shape: more than one chunk per cell, added in chunk order by the second launch."""
    H, W, GX, GY, GL = _multi_partial_shape()
    print("multi-partial shape:", (H, W), "grid", (GX, GY, GL))
    c = R.case(H, W, GX, GY, GL)
    assert R.clear_of_knife_edges(c["rgb"], GL)
    _check(c, *_run(c))


def test_channel_view_of_a_four_channel_render():
    c = R.case(37, 53, 5, 4, 3, 3, 1)
    render = torch.cat([_t(c["rgb"]), torch.rand(37, 53, 1, device=DEV)], dim=-1).requires_grad_(True)
    grids = _t(c["grids"]).requires_grad_(True)
    view = render[..., :3]
    assert not view.is_contiguous()
    out = ops.bilagrid_apply(grids, 1, view)
    out.backward(_t(c["v_out"]))
    _check(c, out.detach(), render.grad[..., :3], grids.grad)
    assert float(render.grad[..., 3].abs().max()) == 0.0


def test_only_the_gradients_that_are_wanted():
    c = R.case(37, 53, 5, 4, 3, 3, 1)
    out, v_rgb, v_grids = _run(c, want_grids=False)
    assert v_grids is None
    _check(c, out, v_rgb, None)
    out, v_rgb, v_grids = _run(c, want_rgb=False)
    assert v_rgb is None
    _check(c, out, None, v_grids)
    out, v_rgb, v_grids = _run(c, want_rgb=False, want_grids=False)
    assert not out.requires_grad and v_rgb is None and v_grids is None
    _check(c, out, None, None)


@pytest.mark.parametrize("which", ["default", "multi_partial"])
def test_run_to_run(which):
    """No atomics, one order of addition: two calls on the same inputs are bit for bit equal."""
    c = R.case(96, 160, 16, 16, 8) if which == "default" else R.case(*_multi_partial_shape())
    a, b = _run(c), _run(c)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def _module(grids):
    num, _, GL, GY, GX = grids.shape
    m = BilateralGrid(num=num, grid_X=GX, grid_Y=GY, grid_W=GL).to(DEV)
    with torch.no_grad():
        m.grids.copy_(_t(grids))
    return m


def test_apply_to_render_dispatch(monkeypatch):
    """With the knob set apply_to_render is the fused call, bit for bit; a grid shape outside the supported range takes the
    torch path and raises nothing."""
    c = R.case(37, 53, 5, 4, 3, 3, 1)
    m = _module(c["grids"])
    rgb = _t(c["rgb"])
    monkeypatch.setenv("FG_FUSED_BILAGRID", "1")
    assert bilagrid.fused_applies(m, rgb.unsqueeze(0))
    with torch.no_grad():
        fused = bilagrid.apply_to_render(m, rgb.unsqueeze(0), 1, 37, 53)
        assert fused.shape == (1, 37, 53, 3) and torch.equal(fused[0], ops.bilagrid_apply(m.grids, 1, rgb))
    wide = BilateralGrid(num=1, grid_X=5, grid_Y=4, grid_W=17).to(DEV)  # 17 levels: beyond the kernels' range
    with torch.no_grad():
        wide.grids.add_(0.3 * torch.randn_like(wide.grids))
    assert not _lib.load().fg_bilagrid_supported(5, 4, 17) and not bilagrid.fused_applies(wide, rgb.unsqueeze(0))
    with pytest.raises(ValueError):
        ops.bilagrid_apply(wide.grids, 0, rgb)
    seen = []
    monkeypatch.setattr(ops, "bilagrid_apply", lambda *a, **k: seen.append(a))
    with torch.no_grad():
        with_knob = bilagrid.apply_to_render(wide, rgb.unsqueeze(0), 0, 37, 53)
        monkeypatch.delenv("FG_FUSED_BILAGRID")
        without = bilagrid.apply_to_render(wide, rgb.unsqueeze(0), 0, 37, 53)
    assert not seen and torch.equal(with_knob, without)


def test_model_step_agrees_with_the_torch_path(monkeypatch):
    """The tiny scene of tests/test_bilagrid.py's GPU test (160 x 96, grid (8, 8, 4), two training images): one get_outputs +
    get_loss_dict + backward from the same state with the knob set and unset; the slice's output, the grids' gradient and
    the means' gradient (which passes through v_rgb and the whole raster backward) agree at the bar."""
    from freegaussian_amd.model import FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import room_scene
    from scripts.train_e2e import camera_from_viewmat, render_ground_truth

    W, H = 160, 96
    scene, _ = room_scene(6000, W, H, n_views=40, seed=2)
    scene.viewmats, scene.Ks = scene.viewmats[:1], scene.Ks[:1]
    rgba = render_ground_truth(scene, DEV)[0].float() / 255.0
    gt = rgba[..., :3] * rgba[..., 3:]
    torch.manual_seed(0)
    cfg = FreeGaussianModelConfig(use_bilateral_grid=True, grid_shape=(8, 8, 4), background_color="black", num_downscales=0,
                                  warm_up=10**9, refine_every=10**9, num_random=4000, random_scale=3.0)  # fmt: skip
    m = FreeGaussianModel(cfg, num_train_data=2).to(DEV).train()
    with torch.no_grad():
        m.bil_grids.grids.add_(0.1 * torch.randn_like(m.bil_grids.grids))
    m.step_cb(1)

    def step(knob):
        monkeypatch.setenv("FG_FUSED_BILAGRID", knob)
        for p in m.parameters():
            p.grad = None
        cam = camera_from_viewmat(scene.viewmats[0].clone(), scene.Ks[0], W, H, 0.0)
        cam.metadata["cam_idx"] = 1
        out = m.get_outputs(cam)
        ld = m.get_loss_dict(out, {"image": gt})
        (ld["main_loss"] + ld["scale_reg"] + ld["tv_loss"]).backward()
        return out["rgb"].detach().clone(), m.bil_grids.grids.grad.clone(), m.gauss_params["means"].grad.clone()

    calls = []
    real = ops.bilagrid_apply
    monkeypatch.setattr(ops, "bilagrid_apply", lambda *a: calls.append(1) or real(*a))
    torch_path = step("0")
    assert not calls
    fused = step("1")
    assert len(calls) == 1
    errs = {n: rel_err(a, b) for n, a, b in zip(("rgb", "grids.grad", "means.grad"), fused, torch_path)}
    print("model step, fused against torch:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert float(torch_path[1][0].abs().max()) > 0  # (camera 0's block: the tv term alone)
    assert all(e <= REL_TOL for e in errs.values()), errs
