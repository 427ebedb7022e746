"""Adaptive density control: the product's HIP passes, and the torch
restatement of the reference's op sequence (tests/densify_torch_sequence.py), against the CPU
restatement in oracle/ (itself pinned to the reference's own methods: tests/golden/g_densify.npz)."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from densify_torch_sequence import refine_torch  # noqa: E402

from freegaussian_amd.densify import PARAM_NAMES, refinement_after
from freegaussian_amd.model import FreeGaussianModel, FreeGaussianModelConfig
from oracle import densify_oracle as DO


def _setup(n=6000, step=3500, seed=0, device="cpu", **cfg_kw):
    torch.manual_seed(seed)
    cfg = FreeGaussianModelConfig(num_downscales=0, **cfg_kw)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        gp = model.gauss_params
        # sizes straddle densify_size_thresh (0.01) AND its 1.6x band (the split-then-duplicate quirk),
        # a few beyond cull_scale_thresh (0.5); opacities straddle cull_alpha_thresh (0.1)
        gp["scales"].copy_(torch.log(torch.exp(torch.randn(n, 3, generator=g) * 0.9 - 4.6)))
        gp["scales"][:20] = 0.2
        gp["opacities"].copy_(torch.randn(n, 1, generator=g) * 2.0)
        gp["quats"].mul_(1.0 + torch.rand(n, 1, generator=g))
        gp["features_rest"].normal_(0, 0.1, generator=g)
    model.step = step
    model.last_size = (96, 160)
    model.xys_grad_norm = torch.rand(n, generator=g) * 4e-5
    model.vis_counts = torch.randint(1, 5, (n,), generator=g).float()
    model.max_2Dsize = torch.rand(n, generator=g) * 0.2
    model = model.to(device)
    for k in ("xys_grad_norm", "vis_counts", "max_2Dsize"):
        setattr(model, k, getattr(model, k).to(device))
    opts = {k: torch.optim.Adam([model.gauss_params[k]], lr=1e-3) for k in PARAM_NAMES}
    for k, o in opts.items():  # one step so that the moments exist and are not trivial
        model.gauss_params[k].grad = torch.randn(model.gauss_params[k].shape, generator=g).to(device)
        o.step()
        o.zero_grad(set_to_none=True)
    return model, opts


def _oracle_inputs(model, opts):
    params = {k: model.gauss_params[k].detach().cpu().clone() for k in PARAM_NAMES}
    moments = {}
    for k, o in opts.items():
        st = o.state[o.param_groups[0]["params"][0]]
        moments[k] = {m: st[m].detach().cpu().clone() for m in ("exp_avg", "exp_avg_sq")}
    stats = {"xys_grad_norm": model.xys_grad_norm.cpu(), "vis_counts": model.vis_counts.cpu(),
             "max_2Dsize": model.max_2Dsize.cpu(), "last_size": model.last_size}  # fmt: skip
    return params, moments, stats


def _n_splits(model, step):
    cfg = model.config
    avg = (model.xys_grad_norm / model.vis_counts) * 0.5 * max(model.last_size)
    high = avg > cfg.densify_grad_thresh
    s = (model.gauss_params["scales"].exp().max(-1).values > cfg.densify_size_thresh) & high
    if step < cfg.stop_screen_size_at:
        s = s | (model.max_2Dsize > cfg.split_screen_size)
    return int(s.sum())


def _check(model, opts, ref_params, ref_moments, exact):
    for k in PARAM_NAMES:
        a, b = model.gauss_params[k].detach().cpu(), ref_params[k]
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if exact and k != "means":  # the product's quat_to_rotmat orders its products differently
            assert torch.equal(a, b), k
        else:
            tol = 1e-5 if k == "means" else 2e-6  # children move by R (exp(s) z): products of O(1) terms
            assert torch.allclose(a, b, rtol=tol, atol=tol / 10), (k, (a - b).abs().max())
        o = opts[k]
        p = o.param_groups[0]["params"][0]
        assert p is model.gauss_params[k] and len(o.state) == 1
        for m in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(o.state[p][m].cpu(), ref_moments[k][m]), (k, m)


# ------------------------------------------------------------------------------------------------
# the oracle pinned to the reference's own methods (tests/golden/g_densify.npz: the reference's
# refinement_after / split_gaussians / dup_gaussians / cull_gaussians / *_in_optim executed from AST
# slices with a stub `self`, tests/golden/make_golden.py::gen_densify)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
from make_golden import DENSIFY_CASES, DENSIFY_CFG  # noqa: E402  (tables only; nothing reads /root/reference)


def _max_ulp(a, b):
    """Largest distance in units in the last place between two float32 tensors of one shape."""
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32
    if a.numel() == 0:
        return 0
    ia, ib = (x.contiguous().view(torch.int32).long() for x in (a, b))
    ia, ib = (torch.where(x < 0, -(x & 0x7FFFFFFF), x) for x in (ia, ib))  # sign-magnitude bits -> one ordered line
    return int((ia - ib).abs().max())


@pytest.mark.parametrize("case", DENSIFY_CASES, ids=[c[0] for c in DENSIFY_CASES])
def test_densify_oracle_matches_the_references_own_methods(case):
    import types

    import numpy as np

    tag, step, over, n, k_rest, special = case
    z = np.load(os.path.join(GOLD, "g_densify.npz"))
    t = lambda k: torch.from_numpy(z[f"{tag}.{k}"])  # noqa: E731
    params = {k: t(f"in.{k}") for k in PARAM_NAMES}
    moments = {k: {m: t(f"in.{k}.{m}") for m in ("exp_avg", "exp_avg_sq")} for k in PARAM_NAMES}
    stats = {"xys_grad_norm": t("in.xys_grad_norm"), "vis_counts": t("in.vis_counts"), "max_2Dsize": t("in.max_2Dsize"),
             "last_size": (96, 160)}  # fmt: skip
    cfg = types.SimpleNamespace(**{**DENSIFY_CFG, **over})
    meta = t("meta").tolist()
    assert meta[0] == step and meta[1] == n == params["means"].shape[0]
    new_p, new_m, info = DO.refinement_after(params, moments, stats, cfg, step, 60, samples=t("samples"))
    assert new_p["means"].shape[0] == meta[2]
    assert t("samples").shape[0] == cfg.n_split_samples * info["n_splits"]
    for k in PARAM_NAMES:
        # same torch ops in the same order on the same values: exact, except the rotated offsets
        if k == "means":
            assert torch.allclose(new_p[k], t(f"out.{k}"), rtol=1e-6, atol=1e-7), k
        elif k == "scales":
            # the split's log(exp(s) / 1.6): bit-exact on the host the vectors were made on; another x86 CPU's exp / log
            # rounds a few of them one ulp the other way (whatever ATen's SIMD level or thread count)
            assert _max_ulp(new_p[k], t(f"out.{k}")) <= 1, k
        else:
            assert torch.equal(new_p[k], t(f"out.{k}")), k
        for m in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(new_m[k][m], t(f"out.{k}.{m}")), (k, m)
    if special == "quirk":
        assert info["n_splits"] == 1 and info["n_dups"] == 1
    if special == "dup_only":
        assert info["n_splits"] == 0 and info["n_dups"] > 0


def test_after_train_iter_matches_the_references_own_method():
    """S1 (:369-392): the model's statistics update against the reference method run on a stub."""
    import numpy as np

    z = np.load(os.path.join(GOLD, "g_densify.npz"))
    t = lambda k: torch.from_numpy(z[f"s1.{k}"])  # noqa: E731
    m = FreeGaussianModel(FreeGaussianModelConfig(), num_points=40)
    m.last_size = (96, 160)
    for it in range(2):
        m.step = 700 + it
        m.radii = t(f"radii{it}")
        m.xys = torch.zeros(1, 40, 2)
        m.xys.absgrad = t(f"absgrad{it}")
        m.after_train_iter(m.step)
        assert torch.equal(m.xys_grad_norm, t(f"xys_grad_norm{it}"))
        assert torch.equal(m.vis_counts, t(f"vis_counts{it}")) and torch.equal(m.max_2Dsize, t(f"max_2Dsize{it}"))


CASES = [
    (3500, {}),  # densify, screen-size tests on, too-big culling on
    (4500, {}),  # densify, screen-size tests off
    (900, {"refine_start": 500}),  # densify before refine_every*reset_alpha_every: no too-big culling
    (15100, {}),  # past stop_split_at: cull only
    (3100, {}),  # step % reset_interval == refine_every: opacity reset, no densification
    (100, {}),  # before refine_start: nothing
]


@pytest.mark.parametrize("step,cfg_kw", CASES)
def test_reference_op_sequence_matches_oracle_on_cpu(step, cfg_kw):
    model, opts = _setup(step=step, **cfg_kw)
    params, moments, stats = _oracle_inputs(model, opts)
    z = torch.randn(model.config.n_split_samples * _n_splits(model, step), 3, generator=torch.Generator().manual_seed(5))
    ref_p, ref_m, info = DO.refinement_after(params, moments, stats, model.config, step, 60, samples=z)
    out = refinement_after(model, opts, step, 60, samples=z, refine=refine_torch)
    if step < model.config.refine_start:
        assert out is None
    else:
        assert out["densified"] == info["densified"] and out["opacity_reset"] == info["opacity_reset"]
        assert model.xys_grad_norm is None and model.max_2Dsize is None
    if step == 3500:
        assert info["n_splits"] > 50 and info["n_dups"] > 50 and ref_p["means"].shape[0] != 6000
    _check(model, opts, ref_p, ref_m, exact=True)


def test_split_then_duplicate_quirk_is_reproduced():
    """`dups` is evaluated after split_gaussians shrank the split rows in place: a Gaussian between
    densify_size_thresh and 1.6x that, with high gradient, is split AND duplicated (shrunk copy)."""
    model, opts = _setup(n=64, step=3500)
    with torch.no_grad():
        model.gauss_params["scales"].fill_(-9.0)
        model.gauss_params["scales"][7] = torch.log(torch.tensor(0.013))  # 0.01 < 0.013 < 0.016
        model.gauss_params["opacities"].fill_(2.0)
    model.xys_grad_norm = torch.zeros(64)
    model.xys_grad_norm[7] = 1.0
    model.vis_counts = torch.ones(64)
    model.max_2Dsize = torch.zeros(64)
    params, moments, stats = _oracle_inputs(model, opts)
    z = torch.randn(2, 3, generator=torch.Generator().manual_seed(1))
    ref_p, ref_m, info = DO.refinement_after(params, moments, stats, model.config, 3500, 60, samples=z)
    assert info["n_splits"] == 1 and info["n_dups"] == 1 and ref_p["means"].shape[0] == 63 + 2 + 1
    assert torch.allclose(ref_p["scales"][-1].exp(), torch.full((3,), 0.013 / 1.6))  # the duplicate is shrunk
    assert torch.equal(ref_p["means"][-1], params["means"][7])  # ... and not moved
    refinement_after(model, opts, 3500, 60, samples=z, refine=refine_torch)
    _check(model, opts, ref_p, ref_m, exact=True)


@pytest.mark.gpu
@pytest.mark.parametrize("step,cfg_kw", CASES[:5])
def test_hip_densify_matches_oracle(step, cfg_kw):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (no CPU fallback exists)")
    model, opts = _setup(n=50_000, step=step, device="cuda", **cfg_kw)
    plain, plain_opts = copy.deepcopy(model), None
    params, moments, stats = _oracle_inputs(model, opts)
    z = torch.randn(model.config.n_split_samples * _n_splits(model, step), 3, generator=torch.Generator().manual_seed(5))
    ref_p, ref_m, info = DO.refinement_after(params, moments, stats, model.config, step, 60, samples=z)
    out = refinement_after(model, opts, step, 60, samples=z)
    assert out["after"] == ref_p["means"].shape[0] and out["densified"] == info["densified"]
    # expf / logf / the 3x3 product differ from torch's CPU kernels in the last bit: the rows a
    # threshold decides are compared exactly through the shapes, the values within 2e-6
    _check(model, opts, ref_p, ref_m, exact=False)
    # and the torch op sequence on the GPU gives the same set
    plain_opts = {k: torch.optim.Adam([plain.gauss_params[k]], lr=1e-3) for k in PARAM_NAMES}
    for k, o in plain_opts.items():
        st = opts_state = moments[k]
        o.state[o.param_groups[0]["params"][0]] = {"step": torch.tensor(1.0), "exp_avg": st["exp_avg"].cuda(),
                                                    "exp_avg_sq": st["exp_avg_sq"].cuda()}  # fmt: skip
    refinement_after(plain, plain_opts, step, 60, samples=z, refine=refine_torch)
    for k in PARAM_NAMES:
        assert plain.gauss_params[k].shape == model.gauss_params[k].shape
        assert torch.allclose(plain.gauss_params[k], model.gauss_params[k], rtol=1e-5, atol=1e-6), k


def _dup_only_setup(device):
    """Every Gaussian small (no size split), past stop_screen_size_at (no screen-size split), some
    with a high gradient: duplicates only -- n_split == 0, n_dup > 0 (the HIP path then
    has no sample buffer to hand to fg_split_children)."""
    model, opts = _setup(n=4000, step=4500, device=device)
    with torch.no_grad():
        model.gauss_params["scales"].fill_(-7.0)  # exp(-7) = 9e-4 < densify_size_thresh
        model.gauss_params["opacities"].fill_(2.0)
    model.xys_grad_norm = (torch.arange(4000) % 7 == 0).float().to(device)
    model.vis_counts = torch.ones(4000, device=device)
    model.max_2Dsize = torch.zeros(4000, device=device)
    return model, opts


def test_duplicates_only_refinement_oracle_and_torch_sequence():
    model, opts = _dup_only_setup("cpu")
    assert _n_splits(model, 4500) == 0
    params, moments, stats = _oracle_inputs(model, opts)
    z = torch.zeros(0, 3)
    ref_p, ref_m, info = DO.refinement_after(params, moments, stats, model.config, 4500, 60, samples=z)
    assert info["n_splits"] == 0 and info["n_dups"] == 572 and ref_p["means"].shape[0] == 4572
    refinement_after(model, opts, 4500, 60, samples=z, refine=refine_torch)
    _check(model, opts, ref_p, ref_m, exact=True)


@pytest.mark.gpu
def test_hip_duplicates_only_refinement():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (no CPU fallback exists)")
    model, opts = _dup_only_setup("cuda")
    params, moments, stats = _oracle_inputs(model, opts)
    ref_p, ref_m, info = DO.refinement_after(params, moments, stats, model.config, 4500, 60, samples=torch.zeros(0, 3))
    out = refinement_after(model, opts, 4500, 60)  # draws its own (empty) sample tensor, as training does
    assert out["after"] == 4572 and info["n_splits"] == 0
    _check(model, opts, ref_p, ref_m, exact=False)


def test_product_refuses_cpu_tensors():
    from freegaussian_amd._lib import FgRasterError

    model, opts = _setup(n=100, step=3500)
    with pytest.raises(FgRasterError):
        refinement_after(model, opts, 3500, 60)


@pytest.mark.gpu
def test_training_with_densification_through_the_harness():
    """A short optimisation run with refinement every 10 steps, once with the HIP passes and once
    with the reference's torch op sequence: same Gaussian counts at every step, same losses, and
    every optimizer keeps tracking the replaced parameter.  (The loss itself jumps at every
    refinement -- duplicates double their opacity contribution -- so it is not asserted to fall.)"""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(__file__))
    from test_gpu_parity import _model_and_camera

    import freegaussian_amd.densify as D
    from freegaussian_amd import harness as Hn

    runs = []
    for refine in (None, refine_torch):
        torch.manual_seed(123)
        model, _, cam = _model_and_camera(n=3000, W=128, H=96, step=20, training=True)
        c = model.config
        c.warm_up, c.refine_start, c.refine_every, c.reset_alpha_every = 10**9, 20, 10, 3
        c.densify_grad_thresh, c.stop_screen_size_at, c.sh_degree_interval = 1e-4, 0, 1
        with torch.no_grad():  # opacities well away from the cull threshold's knife edge
            model.gauss_params["opacities"].copy_(torch.randn(3000, 1, generator=torch.Generator().manual_seed(3)).cuda() * 1.5)
        target = copy.deepcopy(model)
        with torch.no_grad():
            target.gauss_params["features_dc"].add_(0.3)
        target.eval()
        with torch.no_grad():
            gt = target.get_outputs(copy.deepcopy(cam))["rgb"].clamp(0, 1)
        opts = Hn.build_optimizers(model)
        orig = D.refinement_after
        D.refinement_after = lambda m, o, s, n, refine=refine: orig(m, o, s, n, refine=refine)
        try:
            torch.manual_seed(7)
            hist = [Hn.train_step(model, opts, copy.deepcopy(cam), gt, 20 + i, num_train_data=2) for i in range(45)]
        finally:
            D.refinement_after = orig
        runs.append((hist, model, opts))
    (h1, m1, o1), (h0, m0, o0) = runs
    counts1, counts0 = [h["gaussian_count"] for h in h1], [h["gaussian_count"] for h in h0]
    assert len(set(counts1)) >= 2 and counts1[-1] != 3000  # the set was rebuilt
    # float atomics in the raster backward make two runs differ in the last bits; after a few Adam
    # steps a handful of Gaussians sit on the other side of a threshold: counts agree to <1%, and
    # exactly up to the first refinement
    # (the exact equivalence of one refinement is pinned by the oracle tests above; this run only
    # has to show that both implementations drive the same training trajectory)
    assert counts1[0] == counts0[0]
    assert all(abs(a - b) <= 0.03 * b for a, b in zip(counts1, counts0))
    for a, b in zip(h1, h0):
        assert abs(a["loss"] - b["loss"]) <= 0.1 * abs(b["loss"]) + 1e-7
    for k in PARAM_NAMES:
        p = o1[k].param_groups[0]["params"][0]
        assert p is m1.gauss_params[k] and p.shape[0] == counts1[-1]
        assert o1[k].state[p]["exp_avg"].shape == p.shape and len(o1[k].state) == 1
