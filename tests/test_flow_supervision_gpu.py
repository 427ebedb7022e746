"""Flow-supervised training on the GPU: ``ops.flow_displacement`` (csrc/flow_disp.hip), ``ops.flow_l1`` (csrc/flow_loss.hip)
and the model's flow branch.

DISPLACEMENT, PER ROW AND REGIME:  |x_hip - x64|_2 / |x64|_2  <=  F_DISP * E32(regime, array, mode) for ``disp``, ``g_means_t``,
``g_means_0`` over the 4096 rows of tests/flow_supervision_restatement.py's ``disp_case`` (four depth classes, three motion
classes, one camera and two); the rows that are invalid by construction are exact zeros.  In the two small-motion regimes the
naive torch fp32 form (project twice, subtract; on the GPU, through autograd) is recorded beside it: reported, not asserted.
SHAPES: the first N = 1, 63, 64, 65, 257 rows (a workgroup is 256 rows) give the bits of the 4096-row call, with contiguous
means and with the two sets as columns 0..2 and 3..5 of an [N,7] block read in place.  EXACT: a second run, each gradient alone,
permuted rows.
LOSS, PER ELEMENT: the value over its absolute accumulation and every gradient element over its own magnitude <= F_LOSS * E32,
over renders of 1 x 1, 7 x 5, 16 x 16, 33 x 17 at d = 1, 2, 4, 8 with nonzero remainders, every mask dtype and none, NaN and inf
source pixels; ``pred`` contiguous and as channels 4..5 of a 6-channel block; one all-invalid case; two runs, the same bits.
MODEL: 2 000 Gaussians at 64 x 64 behind ``warm_up``, ``cameras0`` a small step away in pose and time: (a) the fused branch
against the existing composition within 1e-4, both front ends, both ``flow_camera_motion`` values; (b) weight 0 or no
``cameras0``: the parent's bits, the new ops never called; (c) ``flow_frame0_grad=False``: the same forward bits, another
gradient; (d) 20 ``train_step``s with ``flows=`` lower the flow loss.

``PYTHONPATH=. python tests/test_flow_supervision_gpu.py REPORT.jsonl`` turns the records of a run under FG_PARITY_REPORT into
the tables of profiles/flow_supervision_parity.md.
"""
import copy
import functools
import sys

import pytest
import torch

import flow_supervision_restatement as R
import helpers
import parity_common as P
from freegaussian_amd import ops
from parity_common import need_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = (1, 63, 64, 65, 257)

# ---------------------------------------------------------------------------------------------------------------------
# displacement


def _run_disp(mode="same", n=R.ROWS, want=(True, True), block=False, perm=None):
    """One forward and backward of ops.flow_displacement over the first n rows -> (disp, g_means_t, g_means_0) on the CPU, None
    where not asked for.  ``block``: the means are columns 0..2 and 3..5 of an [n,7] tensor."""
    c = R.disp_case(0)
    mt, m0, g = (c[k][:n] if perm is None else c[k][perm] for k in ("mt", "m0", "g"))
    if block:
        both = torch.full((n, 7), float("nan"))
        both[:, :3], both[:, 3:6] = mt, m0
        both = both.to(DEV)
        mt, m0 = both[:, :3].requires_grad_(want[0]), both[:, 3:6].requires_grad_(want[1])
        assert n == 1 or (mt.stride() == (7, 1) and m0.data_ptr() == mt.data_ptr() + 12)
    else:
        mt, m0 = mt.to(DEV).requires_grad_(want[0]), m0.to(DEV).requires_grad_(want[1])
    V0 = None if mode == "same" else c["V0"].to(DEV)
    disp = ops.flow_displacement(mt, m0, c["Vt"].to(DEV), V0, c["K"].to(DEV), R.WIDTH, R.HEIGHT, R.NEAR, R.MARGIN)
    if any(want):
        disp.backward(g.to(DEV))
    torch.cuda.synchronize()
    return tuple(None if a is None else a.detach().cpu() for a in (disp, mt.grad, m0.grad))


_first = functools.lru_cache(maxsize=None)(_run_disp)  # the joint 4096-row call per mode, once


def _naive_torch(mode):
    """mu = K p / z twice and subtract, fp32 torch ops on the GPU, through autograd."""
    c = R.disp_case(0)
    mt, m0 = c["mt"].to(DEV).requires_grad_(True), c["m0"].to(DEV).requires_grad_(True)
    Vt, K = c["Vt"].to(DEV), c["K"].to(DEV)
    V0 = Vt if mode == "same" else c["V0"].to(DEV)
    mu_t, mu_0 = (mt @ Vt[:3, :3].T + Vt[:3, 3]) @ K.T, (m0 @ V0[:3, :3].T + V0[:3, 3]) @ K.T
    disp = mu_t[:, :2] / mu_t[:, 2:3] - mu_0[:, :2] / mu_0[:, 2:3]
    disp = torch.where(c[mode]["r64"]["valid"].to(DEV)[:, None], disp, torch.zeros((), device=DEV))
    disp.backward(c["g"].to(DEV))
    return tuple(a.detach().cpu() for a in (disp, mt.grad, m0.grad))


@pytest.mark.parametrize("mode", R.MODES)
def test_displacement_every_row_by_regime(mode):
    c = R.disp_case(0)[mode]
    hip, naive = dict(zip(R.DISP_ARRAYS, _first(mode))), dict(zip(R.DISP_ARRAYS, _naive_torch(mode)))
    failures = []
    for name in R.DISP_ARRAYS:  # every ratio is recorded before anything is asserted
        assert hip[name].shape == (R.ROWS, 3 - (name == "disp")) and hip[name].dtype == torch.float32
        d = P.distance(hip[name], c["r64"][name], c["r64"][name], rows=True)
        P.check(f"{name}|{mode}|{{regime}}", c["masks"], d, c["e32"][name], R.F_DISP, failures)
        dn = P.distance(naive[name], c["r64"][name], c["r64"][name], rows=True)
        for regime, (ratio, _) in P.worst_ratios({k: c["masks"][k] for k in R.SMALL_MOTION}, dn, c["e32"][name]).items():
            helpers._record(f"naive_ratio|{name}|{mode}|{regime}", ratio, 1)
            print(f"{name} {mode} {regime}: naive torch fp32 form {ratio:.3g} x E32")
        broken = P.exact_zero_rule(hip[name], c["r64"][name])
        assert not bool(broken.any()), (name, broken.nonzero().flatten().tolist()[:8])
        assert bool(torch.isfinite(hip[name]).all()), name
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("block", [False, True], ids=["contiguous", "columns-of-7"])
@pytest.mark.parametrize("n", SHAPES + (R.ROWS,))
def test_displacement_shapes_give_the_bits_of_the_full_call(n, block, mode):
    """(n = 4096, contiguous: a second run of the same call gives the same bits.)"""
    for name, a, b in zip(R.DISP_ARRAYS, _run_disp(mode, n, block=block), _first(mode)):
        assert a.shape[0] == n and torch.equal(a, b[:n]), name


@pytest.mark.parametrize("mode", R.MODES)
def test_displacement_permuted_rows_give_permuted_bits(mode):
    perm = torch.randperm(R.ROWS, generator=torch.Generator().manual_seed(5))
    for name, a, b in zip(R.DISP_ARRAYS, _run_disp(mode, perm=perm), _first(mode)):
        assert torch.equal(a, b[perm]), name


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("which", [0, 1, None])
def test_displacement_each_gradient_alone_gives_the_bits_of_the_joint_call(which, mode):
    want = tuple(i == which for i in range(2))
    got, joint = _run_disp(mode, want=want), _first(mode)
    assert torch.equal(got[0], joint[0])
    for i in range(2):
        assert (got[1 + i] is None) == (i != which)
        if i == which:
            assert torch.equal(got[1 + i], joint[1 + i])


def test_displacement_margin_inf_switches_the_rectangle_test_off():
    c = R.disp_case(0)
    mt, m0 = c["mt"].to(DEV), c["m0"].to(DEV)
    disp = ops.flow_displacement(mt, m0, c["Vt"].to(DEV), None, c["K"].to(DEV), R.WIDTH, R.HEIGHT, R.NEAR).cpu()
    r64 = R.restate_disp(c["mt"], c["m0"], c["Vt"], None, c["K"], c["g"], torch.float64, margin=float("inf"))
    outside = torch.tensor([k in ("outside_t", "outside_0") for k in c["kind"]])
    behind = torch.tensor([k in ("behind_t", "behind_0") for k in c["kind"]])
    assert bool(r64["valid"][outside].all()) and bool((disp[outside] != 0).any(dim=1).all()) and not bool(disp[behind].any())
    d = P.distance(disp, r64["disp"], r64["disp"], rows=True)
    assert float(d[outside].max()) <= 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# loss


def _run_loss(c, strided=False):
    """-> (loss, g_pred) on the CPU.  ``strided``: pred is channels 4..5 of an [H,W,6] block."""
    pred = c["pred"]
    if strided:
        block = torch.full(pred.shape[:2] + (6,), float("nan"))
        block[..., 4:] = pred
        leaf = block.to(DEV).requires_grad_(True)
        view = leaf[..., 4:]
    else:
        leaf = pred.to(DEV).requires_grad_(True)
        view = leaf
    mask = None if c["mask"] is None else c["mask"].to(DEV)
    loss = ops.flow_l1(view, c["flows"].to(DEV), mask, c["d"])
    loss.backward()
    torch.cuda.synchronize()
    g = leaf.grad[..., 4:] if strided else leaf.grad
    if strided:
        assert not bool(leaf.grad[..., :4].any())
    return loss.detach().cpu(), g.detach().cpu()


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "channels-4-5-of-6"])
@pytest.mark.parametrize("H,W,d,kind", R.loss_cases())
def test_loss_value_and_every_gradient_element(H, W, d, kind, strided):
    c = R.loss_case(H, W, d, kind)
    loss, g = _run_loss(c, strided)
    r64 = c["r64"]
    key = f"{H}x{W}|d{d}|{kind}|{'strided' if strided else 'contiguous'}"
    failures = []
    assert loss.shape == () and g.shape == (H, W, 2) and bool(torch.isfinite(loss)) and bool(torch.isfinite(g).all())
    if float(r64["loss"]) == 0.0:
        assert float(loss) == 0.0
    else:
        dv = float(P.distance(loss.reshape(1), r64["loss"].reshape(1), r64["A"].reshape(1))[0])
        P.check_cell(f"value|{key}", dv / c["e32_value"], c["e32_value"], R.F_LOSS, failures, "the loss")
    dg = P.distance(g, r64["g_pred"], r64["g_pred"].abs())
    P.check(f"g_pred|{key}|{{regime}}", c["masks"], dg, c["e32"], R.F_LOSS, failures)
    assert not bool(g[r64["g_pred"] == 0].any())  # exact zeros stay exact: no weight, or pred on the target
    assert not failures, "\n".join(failures)
    loss2, g2 = _run_loss(c, strided)  # two runs, the same bits
    assert torch.equal(loss, loss2) and torch.equal(g, g2)


@pytest.mark.parametrize("kind", [None, "float32"])
def test_loss_all_invalid_is_zero_with_a_zero_gradient(kind):
    c = R.loss_case(7, 5, 2, kind, bad="all")
    loss, g = _run_loss(c)
    assert float(loss) == 0.0 and not bool(g.any())
    # and a mask of zeros over finite flows
    c = dict(R.loss_case(7, 5, 2, "uint8", bad="none"))
    c["mask"] = torch.zeros_like(c["mask"])
    loss, g = _run_loss(c)
    assert float(loss) == 0.0 and not bool(g.any())


# ---------------------------------------------------------------------------------------------------------------------
# model level


def _scene(n=2000, W=64, H=64, **cfg):
    """A model behind ``warm_up`` whose Gaussians lie in a slab in front of both cameras and inside both images, the camera and
    its ``cameras0`` a small step away in pose and time."""
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    config = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000, **cfg)
    pts = (torch.rand(n, 3) - 0.5) * torch.tensor([1.2, 1.2, 1.0])
    model = FreeGaussianModel(config, seed_points=pts, init_scales=-3.0)
    with torch.no_grad():
        model.gauss_params["scales"].fill_(-3.0)
        model.gauss_params["features_rest"].normal_(0, 0.1)
        # motion between the two times of a hundredth of the depth and more: about half a pixel, far above the rounding of the
        # composition's two projected centres (whose difference the comparison below takes as the reference)
        for p in list(model.deform.branch_w.parameters()) + list(model.deform.branch_v.parameters()):
            p.mul_(3.0)
    model.step = 4000
    model.train(True)

    def cam(eye, t):
        c2w = torch.linalg.inv(look_at_viewmat(torch.tensor(eye), torch.zeros(3)))
        c2w[:3, 1:3] *= -1  # OpenCV -> OpenGL camera axes
        f = W / 160.0
        return Camera(c2w[None, :3], 140.0 * f, 150.0 * f, W / 2, H / 2, W, H, times=torch.tensor([[t]]))

    camera, cam0 = cam([0.3, -0.2, -3.0], 0.4), cam([0.27, -0.17, -3.02], 0.3)
    camera.metadata["cameras0"] = cam0
    return model, camera, cam0


def _bar(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _composition(model, camera, cam0, flows, moving):
    """The existing statement of the flow term: the deformed means at both times, two ``ops.project`` passes, the ``where``,
    ``rasterization(extra_channels=...)`` and the torch statement of the loss."""
    from freegaussian_amd.rasterization import rasterization
    from freegaussian_amd.utils import get_viewmat

    viewmat, K, W, H = model._camera_setup(camera)
    viewmat0 = get_viewmat(cam0.camera_to_worlds.to(model.device)) if moving else viewmat
    means_t, d_rot, d_scale = model._deformed(model.means, camera.times)
    means_0 = model._deformed(model.means, cam0.times)[0]
    scales = torch.exp(model.scales) + d_scale
    quats = model.quats / model.quats.norm(dim=-1, keepdim=True) + d_rot
    r0, mu0, _, _, _, _ = ops.project(means_0, quats, scales, viewmat0[0], K[0], W, H)
    rt, mut, _, _, _, _ = ops.project(means_t, quats, scales, viewmat[0], K[0], W, H)
    assert bool((r0 > 0).all()) and bool((rt > 0).all())  # the shared premise: this op's validity rule and radii > 0 coincide
    disp = torch.where(((r0 > 0) & (rt > 0)).unsqueeze(-1), mut - mu0, torch.zeros_like(mut))
    colors, sh_degree = model._colors_and_degree()
    render, _, _ = rasterization(means_t, quats, scales, torch.sigmoid(model.opacities).squeeze(-1), colors, viewmat, K, W, H,
                                 sh_degree=sh_degree, packed=False, render_mode="RGB", absgrad=True, extra_channels=disp)  # fmt: skip
    flow = render[0, :, :, 3:]
    finite = torch.isfinite(flows).all(-1, keepdim=True)
    w = finite.float()
    loss = (w * (flow - torch.where(finite, flows, torch.zeros_like(flows))).abs()).sum() / (2 * w.sum())
    return flow, model.config.flow_loss_weight * loss


@pytest.mark.parametrize("moving", [False, True], ids=["interflow", "camera-motion"])
@pytest.mark.parametrize("front_end", [True, False], ids=["fused-front-end", "torch-front-end"])
def test_model_flow_branch_against_the_existing_composition(front_end, moving):
    base, camera, cam0 = _scene(flow_loss_weight=0.7, flow_camera_motion=moving, fused_front_end=front_end)
    # the shared premise, asserted first: every Gaussian in front of and inside both images at both times
    from freegaussian_amd.utils import get_viewmat

    with torch.no_grad():
        for cam, t in ((camera, camera.times), (cam0, cam0.times), (camera, cam0.times)):
            p = base._deformed(base.means, t)[0] @ get_viewmat(cam.camera_to_worlds)[0, :3, :3].T + get_viewmat(cam.camera_to_worlds)[0, :3, 3]
            u, v = cam.fx * p[:, 0] / p[:, 2] + cam.cx, cam.fy * p[:, 1] / p[:, 2] + cam.cy
            assert float(p[:, 2].min()) > 0.5 and 1 < float(u.min()) and float(u.max()) < 63 and 1 < float(v.min()) and float(v.max()) < 63
    gen = torch.Generator().manual_seed(3)
    flows = torch.randn(64, 64, 2, generator=gen) * 0.5
    flows[5:9, 7:30, 0] = float("nan")
    flows = flows.to(DEV)
    results = {}
    for which in ("fused", "composition"):
        model = copy.deepcopy(base).to(DEV)
        if which == "fused":
            out = model.get_outputs(camera)
            flow, loss = out["flow"], model.get_loss_dict(out, {"image": torch.rand(64, 64, 3, device=DEV), "flows": flows})["flow_loss"]
            assert flow.shape == (64, 64, 2) and flow.stride(2) == 1 and flow._base is not None and out["rgb"].shape == (64, 64, 3)
        else:
            flow, loss = _composition(model, camera, cam0, flows, moving)
        loss.backward()
        torch.cuda.synchronize()
        results[which] = (flow.detach().cpu(), float(loss.detach()), {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None})
    (f1, l1, g1), (f0, l0, g0) = results["fused"], results["composition"]
    assert float(f0.abs().max()) > 0.05 and set(g0) == set(g1) and "gauss_params.means" in g0 and any(k.startswith("deform.") for k in g0)
    worst = {"flow": _bar(f1, f0), "flow_loss": abs(l1 - l0) / abs(l0)}
    for k in g0:
        if float(g0[k].abs().max()) > 0:
            worst[k] = _bar(g1[k], g0[k])
        else:
            assert not bool(g1[k].any()), k
    for k, v in worst.items():
        helpers._record(f"model_bar|{'front' if front_end else 'torch'}|{'moving' if moving else 'interflow'}|{k}", v, 1)
    print({k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) <= helpers.REL_TOL, worst


def _boom(*a, **k):
    raise AssertionError("a flow op called without an active flow branch")


@pytest.mark.parametrize("how", ["weight-0", "no-cameras0"])
def test_model_without_the_branch_is_the_parent_bit_for_bit(monkeypatch, how):
    """Against the path the parent took for the same step -- ``_outputs_from`` with the parent's five arguments and the loss
    dict of a batch without flows -- with the new ops replaced by something that raises.  (The forward is bit-repeatable;
    the raster backward's float atomics are not, profiles/step_repeatability.md, so no gradient is compared here.)"""
    base, camera, cam0 = _scene(flow_loss_weight=0.0 if how == "weight-0" else 0.7)
    if how == "no-cameras0":
        camera.metadata.pop("cameras0")
    monkeypatch.setattr(ops, "flow_displacement", _boom)
    monkeypatch.setattr(ops, "flow_l1", _boom)
    image, flows = torch.rand(64, 64, 3, device=DEV), torch.zeros(64, 64, 2, device=DEV)
    runs = []
    for parent in (False, True):
        model = copy.deepcopy(base).to(DEV)
        if parent:
            viewmat, K, W, H = model._camera_setup(camera)
            out = model._bilateral(model._outputs_from(viewmat, K, W, H, camera.times), camera)
            losses = model.get_loss_dict(out, {"image": image})
        else:
            out = model.get_outputs(camera)
            losses = model.get_loss_dict(out, {"image": image, "flows": flows})
        torch.cuda.synchronize()
        runs.append((out, losses))
    (out, losses), (out_p, losses_p) = runs
    assert set(out) == set(out_p) == {"rgb", "depth", "accumulation", "background"} and set(losses) == set(losses_p) == {"main_loss", "scale_reg"}
    for k in ("rgb", "accumulation"):
        assert torch.equal(out[k], out_p[k]), k
    for k in losses:
        assert torch.equal(losses[k], losses_p[k]), k


def test_model_frame0_without_gradient_same_forward_other_gradient():
    results = {}
    flows = (torch.randn(64, 64, 2, generator=torch.Generator().manual_seed(4)) * 0.5).to(DEV)
    for grad0 in (True, False):
        base, camera, _ = _scene(flow_loss_weight=0.7, flow_frame0_grad=grad0)
        model = base.to(DEV)
        out = model.get_outputs(camera)
        loss = model.get_loss_dict(out, {"image": torch.rand(64, 64, 3, device=DEV), "flows": flows})["flow_loss"]
        loss.backward()
        torch.cuda.synchronize()
        results[grad0] = (out["flow"].detach().cpu(), loss.detach().cpu(), {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None})
    (f1, l1, g1), (f0, l0, g0) = results[True], results[False]
    assert torch.equal(f1, f0) and torch.equal(l1, l0)
    assert all(bool(torch.isfinite(g).all()) for g in g0.values())
    k = "gauss_params.means"
    assert not torch.equal(g1[k], g0[k]) and float(g0[k].abs().max()) > 0


def test_train_steps_with_flows_lower_the_flow_loss():
    from freegaussian_amd import harness

    base, camera, _ = _scene(flow_loss_weight=1.0)
    # the target: the flow of a second model whose deformation net is perturbed; the image: the model's own first render, so
    # that the main loss starts at its minimum and the flow term alone moves the parameters
    other = copy.deepcopy(base)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(11)
        # (the two motion heads by half their size: a target flow a tenth of a pixel and more from the model's own, far above
        #  what one Adam step moves the flow by -- Adam's first steps have the size of the learning rate whatever the
        #  gradient's, so a target closer than that is overshot)
        for p in list(other.deform.branch_w.parameters()) + list(other.deform.branch_v.parameters()):
            p.add_(torch.randn(p.shape, generator=gen) * 0.5 * float(p.abs().max() + 1e-3))
    other = other.to(DEV)
    with torch.no_grad():
        flows = other.get_outputs(camera)["flow"].detach().clone().contiguous()
        image = copy.deepcopy(base).to(DEV).get_outputs(camera)["rgb"].detach().clone()
    assert float(flows.abs().max()) > 1e-3
    model = copy.deepcopy(base).to(DEV)
    opts = harness.build_optimizers(model)
    losses = []
    for i in range(20):
        r = harness.train_step(model, opts, camera, image, 4000 + i, flows=flows)
        assert "flow_loss" in r and "loss" in r
        losses.append(r["flow_loss"])
    print([f"{v:.4g}" for v in losses])
    assert losses[-1] < losses[0]
    # without flows=: no flow_loss
    plain = copy.deepcopy(base).to(DEV)
    r = harness.train_step(plain, harness.build_optimizers(plain), camera, image, 4000)
    assert "flow_loss" not in r and "loss" in r


# ---------------------------------------------------------------------------------------------------------------------


def _report(path):
    """Markdown of a run's records (FG_PARITY_REPORT)."""
    import json

    ratio, e32 = P.read_records(path, "test_flow_supervision_gpu")
    disp = {k: v for k, v in ratio.items() if k[0] in R.DISP_ARRAYS}
    loss = {k: v for k, v in ratio.items() if k[0] in ("value", "g_pred")}
    worst = max(disp, key=disp.get)
    print(f"displacement: worst ratio {disp[worst]:.2f} at {' | '.join(worst)}; {len(disp)} cells.\n")
    cols = R.DEPTH_NAMES + R.MOTION_NAMES
    print("| array | mode | " + " | ".join(cols) + " |\n|---|---|" + "---|" * len(cols))
    for a in R.DISP_ARRAYS:
        for mode in R.MODES:
            print(f"| {a} | {mode} | " + " | ".join(f"{ratio[(a, mode, c)]:.2f} ({e32[(a, mode, c)]:.1e})" for c in cols) + " |")
    other = {}
    for line in open(path):
        r = json.loads(line)
        if r["kind"].startswith(("naive_ratio|", "model_bar|")):
            other[r["kind"]] = max(other.get(r["kind"], 0.0), r["value"])
    print("\n| array | mode | motion | fused (x E32) | naive torch fp32 form on the GPU (x E32) |\n|---|---|---|---|---|")
    for a in R.DISP_ARRAYS:
        for mode in R.MODES:
            for c in R.SMALL_MOTION:
                print(f"| {a} | {mode} | {c} | {ratio[(a, mode, c)]:.2f} | {other[f'naive_ratio|{a}|{mode}|{c}']:.3g} |")
    worst = max(loss, key=loss.get)
    print(f"\nloss: worst ratio {loss[worst]:.2f} at {' | '.join(worst)}; {len(loss)} cells.\n")
    print("| case | value | g_pred, full weight | g_pred, partial weight |\n|---|---|---|---|")
    cases = sorted({k[1:4] + (k[4],) for k in loss if k[0] == "value"} | {k[1:5] for k in loss if k[0] == "g_pred"})
    for case in cases:
        cell = lambda key: f"{loss[key]:.2f} ({e32[key]:.1e})" if key in loss else "-"  # noqa: E731
        print(f"| {' '.join(case)} | {cell(('value',) + case)} | {cell(('g_pred',) + case + ('full weight',))} | "
              f"{cell(('g_pred',) + case + ('partial weight',))} |")  # fmt: skip
    print("\n| model level: the flow branch against the existing composition | max abs difference / max abs |\n|---|---|")
    for k, v in other.items():
        if k.startswith("model_bar|"):
            print(f"| {' '.join(k.split('|')[1:])} | {v:.1e} |")


if __name__ == "__main__":
    _report(sys.argv[1])
