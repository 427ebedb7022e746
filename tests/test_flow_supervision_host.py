"""Flow-supervised training, everything that is decided without a GPU: the float64 restatements of
tests/flow_supervision_restatement.py are torch's float64 autograd of the naive formulas (mu = K p / z twice and subtract;
resize, mask, abs, mean); every regime occurs; the bound of the GPU tests catches each wrong restatement, and that caps F; the
config defaults leave ``get_loss_dict`` as it was; the ops refuse by the argument's name; the header declares the five entry
points, found BY NAME, with the ABI numbers unchanged; and the stand-alone ``flow-check`` program builds and passes."""
import inspect
import math
import os
import re
import subprocess

import pytest
import torch

import flow_supervision_restatement as R
import parity_common as P
from freegaussian_amd import _lib, harness, ops
from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_BOUND = 1e-12  # max |restatement - autograd| / max |autograd| over an array, both float64


# ---------------------------------------------------------------------------------------------------------------------
# displacement


def _naive64(c, mode):
    """float64 autograd of the textbook statement: project both frames with K p / z, subtract, select the valid rows."""
    mt, m0 = c["mt"].double().requires_grad_(True), c["m0"].double().requires_grad_(True)
    Vt, K = c["Vt"].double(), c["K"].double()
    V0 = Vt if mode == "same" else c["V0"].double()
    pt, p0 = mt @ Vt[:3, :3].T + Vt[:3, 3], m0 @ V0[:3, :3].T + V0[:3, 3]
    mu_t, mu_0 = pt @ K.T, p0 @ K.T
    disp = mu_t[:, :2] / mu_t[:, 2:3] - mu_0[:, :2] / mu_0[:, 2:3]
    disp = torch.where(c[mode]["r64"]["valid"][:, None], disp, torch.zeros((), dtype=torch.float64))
    (disp * c["g"].double()).sum().backward()
    return {"disp": disp.detach(), "g_means_t": mt.grad, "g_means_0": m0.grad}


@pytest.mark.parametrize("mode", R.MODES)
def test_displacement_restatement_is_float64_autograd_of_the_naive_form(mode):
    """The gradients to 1e-12 of the array's largest element.  The value needs a word: the naive form's OWN float64 rounding is
    2^-52 of the two pixel coordinates it subtracts (up to ~1e3 pixels: 2e-13 pixels), which at a motion of 1e-6 of the depth is
    no longer 1e-12 of a row; the value is therefore held row by row to 1e-12 of the row + 8 x 2^-52 x the coordinates'
    magnitude, and to 1e-12 of the array's largest element."""
    c = R.disp_case(0)
    a64, r64 = _naive64(c, mode), c[mode]["r64"]
    for name in R.DISP_ARRAYS:
        rel = float((r64[name] - a64[name]).abs().max() / a64[name].abs().max())
        print(f"{mode} {name}: float64 restatement against float64 autograd of the naive form, {rel:.2e} of the largest element")
        assert rel <= TORCH_BOUND, (name, rel)
    row_err = (r64["disp"] - a64["disp"]).norm(dim=-1)
    own = 8 * 2.0**-52 * (R.WIDTH + R.HEIGHT + 2 * R.MARGIN)
    assert bool((row_err <= TORCH_BOUND * a64["disp"].norm(dim=-1) + own).all()), float(row_err.max())


def test_displacement_census_every_regime_and_every_invalid_kind_occurs():
    c = R.disp_case(0)
    assert len(c["depth"]) == R.ROWS == 4096 and c["mt"].dtype == c["m0"].dtype == torch.float32
    for mode in R.MODES:
        m = c[mode]
        count = {k: int(v.sum()) for k, v in m["masks"].items()}
        invalid = {k: int(sum(1 for i, kk in enumerate(c["kind"]) if kk == k and not bool(m["r64"]["valid"][i]))) for k in R.INVALID_KINDS}
        print(mode, count, invalid, "live", int(m["live"].sum()))
        assert all(count[n] >= 100 for n in R.DEPTH_NAMES + R.MOTION_NAMES), count
        assert all(v >= R.INVALID_PER_KIND // 2 for v in invalid.values()), invalid
        if mode == "same":  # by construction: every live row valid, every other row invalid, each for its own reason
            assert all(v == R.INVALID_PER_KIND for v in invalid.values())
            assert int(m["r64"]["valid"].sum()) == R.ROWS - R.INVALID_PER_KIND * len(R.INVALID_KINDS)
            pt = c["mt"].double() @ c["Vt"].double()[:3, :3].T + c["Vt"].double()[:3, 3]
            p0 = c["m0"].double() @ c["Vt"].double()[:3, :3].T + c["Vt"].double()[:3, 3]
            for i, k in enumerate(c["kind"]):
                if k in ("behind_t", "behind_0"):
                    assert float((pt if k == "behind_t" else p0)[i, 2]) <= R.NEAR and float((p0 if k == "behind_t" else pt)[i, 2]) > R.NEAR
        # rows are clear of every edge: float32 arithmetic decides validity as float64 does
        assert torch.equal(m["r32"]["valid"], m["r64"]["valid"]) and torch.equal(m["naive32"]["valid"], m["r64"]["valid"])
        # invalid rows are exact zeros in every array, live rows are finite
        for a in R.DISP_ARRAYS:
            assert not bool(m["r64"][a][~m["r64"]["valid"]].any()) and bool(torch.isfinite(m["r64"][a]).all())
            for name, e in m["e32"][a].items():
                assert R.FLOOR <= e < 1e-2, (mode, a, name, e)
    # the point of the closed form: in one-camera mode at small motion the fp32 yardstick stays at fp32 rounding, where the
    # naive fp32 form loses the row
    same = c["same"]
    naive = P.distance(same["naive32"]["disp"], same["r64"]["disp"], same["r64"]["disp"], rows=True)
    small = same["masks"][R.MOTION_NAMES[0]]
    print(f"smallest motions: closed form E32 {same['e32']['disp'][R.MOTION_NAMES[0]]:.2e}, naive fp32 worst row {float(naive[small].max()):.2e}")
    assert same["e32"]["disp"][R.MOTION_NAMES[0]] < 1e-5 < float(naive[small].max())


def test_displacement_mutants_are_caught_and_cap_F():
    caps = R.disp_mutant_caps(0)
    assert {m for m, _, _ in caps} == set(R.DISP_MUTANTS)
    for key, cap in caps.items():
        print(f"{' | '.join(key)}: caps F at {cap:.3g}")
    smallest = min(caps.values())
    print(f"the cap on F_DISP: {smallest:.3g}")
    assert smallest >= 4
    assert R.F_DISP is None or R.F_DISP <= smallest


# ---------------------------------------------------------------------------------------------------------------------
# loss


def resize_image(image, d):
    """``utils.resize_image``'s strided average pooling, kept in float64 (the original rounds its input to float32)."""
    return torch.nn.functional.avg_pool2d(image.permute(2, 0, 1).unsqueeze(0), kernel_size=d, stride=d).squeeze(0).permute(1, 2, 0)


def _naive_loss64(c):
    """float64 autograd of the torch statement: resize (``utils.resize_image``'s strided pooling) / d, the mask resized the same
    way, the non-finite blocks out, abs, weighted mean."""
    pred = c["pred"].double().requires_grad_(True)
    d, flows, mask = c["d"], c["flows"].double(), c["mask"]
    finite = torch.isfinite(flows).all(-1, keepdim=True)
    clean = torch.where(finite, flows, torch.zeros((), dtype=torch.float64))
    target = (resize_image(clean, d) if d > 1 else clean) / d
    ok = (resize_image(finite.double(), d) if d > 1 else finite.double()) == 1
    w = torch.ones_like(ok, dtype=torch.float64)
    if mask is not None:
        m = mask.reshape(mask.shape[0], mask.shape[1], 1).double()
        w = resize_image(m, d) if d > 1 else m
    w = torch.where(ok, w, torch.zeros((), dtype=torch.float64))
    loss = (w * (pred - target).abs()).sum() / (2 * w.sum().clamp(min=R.TINY))
    loss.backward()
    return loss.detach(), pred.grad


@pytest.mark.parametrize("H,W,d,kind", R.loss_cases())
def test_loss_restatement_is_float64_autograd_of_the_torch_statement(H, W, d, kind):
    c = R.loss_case(H, W, d, kind)
    assert c["flows"].shape[0] // d == H and c["flows"].shape[1] // d == W
    assert d == 1 or (c["flows"].shape[0] % d and c["flows"].shape[1] % d)
    loss, grad = _naive_loss64(c)
    r64 = c["r64"]
    assert abs(float(r64["loss"] - loss)) <= TORCH_BOUND * max(float(r64["A"]), 1e-300) or float(loss) == float(r64["loss"]) == 0
    assert float((r64["g_pred"] - grad).abs().max()) <= TORCH_BOUND * max(float(grad.abs().max()), 1e-300)
    assert torch.equal(r64["g_pred"] == 0, grad == 0)


def test_loss_census_every_regime_occurs():
    seen = {"full weight": 0, "partial weight": 0, "zero weight": 0, "non-finite block": 0, "masks": set(), "d": set(), "sizes": set()}
    for H, W, d, kind in R.loss_cases():
        c = R.loss_case(H, W, d, kind)
        for name in R.LOSS_REGIMES:
            seen[name] += int(c["masks"][name].sum())
        seen["zero weight"] += int((c["r64"]["w"] == 0).sum())
        blocks = c["flows"][: H * d, : W * d].reshape(H, d, W, d, 2)
        seen["non-finite block"] += int((~torch.isfinite(blocks).all(dim=4).all(dim=3).all(dim=1)).sum())
        seen["masks"].add(kind), seen["d"].add(d), seen["sizes"].add((H, W))
        assert R.FLOOR <= c["e32_value"] < 1e-4 and all(R.FLOOR <= e < 1e-4 for e in c["e32"].values())
    print(seen)
    assert seen["masks"] == set(R.MASK_KINDS) and seen["d"] == set(R.LOSS_DOWNSCALES) and seen["sizes"] == set(R.LOSS_SIZES)
    assert min(seen[k] for k in ("full weight", "partial weight", "zero weight", "non-finite block")) >= 50
    # the all-invalid case: loss 0, gradient 0, no NaN
    c = R.loss_case(7, 5, 2, "float32", bad="all")
    assert float(c["r64"]["loss"]) == 0.0 and not bool(c["r64"]["g_pred"].any()) and float(c["r32"]["loss"]) == 0.0


def test_loss_mutants_are_caught_and_cap_F():
    caps = R.loss_mutant_caps()
    assert set(caps) == set(R.LOSS_MUTANTS)
    for key, cap in caps.items():
        print(f"{key}: caps F at {cap:.3g}")
    smallest = min(caps.values())
    assert smallest >= 4
    assert R.F_LOSS is None or R.F_LOSS <= smallest


def test_F_is_set_from_the_committed_table():
    """F = 4 x the worst recorded ratio, rounded up to a power of two; the tables are in profiles/flow_supervision_parity.md."""
    assert R.F_DISP is not None and R.F_LOSS is not None
    text = open(os.path.join(ROOT, "profiles", "flow_supervision_parity.md")).read()
    for F, what in ((R.F_DISP, "displacement"), (R.F_LOSS, "loss")):
        worst = float(re.search(r"%s: worst ratio ([0-9.]+)" % what, text).group(1))
        want = 1.0
        while want < 4 * worst:
            want *= 2
        assert F == want, (what, F, worst, want)


# ---------------------------------------------------------------------------------------------------------------------
# model, harness, ops, library


def _tiny_model(**cfg):
    torch.manual_seed(0)
    return FreeGaussianModel(FreeGaussianModelConfig(num_downscales=0, **cfg), num_points=50, init_scales=-3.0)


def test_config_defaults_leave_the_loss_dict_keys_unchanged():
    cfg = FreeGaussianModelConfig()
    assert (cfg.flow_loss_weight, cfg.flow_camera_motion, cfg.flow_frame0_grad) == (0.0, False, True)
    model = _tiny_model()
    outputs = {"rgb": torch.rand(16, 16, 3, requires_grad=True), "background": torch.ones(3)}
    batch = {"image": torch.rand(16, 16, 3), "flows": torch.zeros(16, 16, 2)}
    assert set(model.get_loss_dict(outputs, batch)) == {"main_loss", "scale_reg"}  # (no "flow" in the outputs: the key is absent)
    assert model._flow_loss({"flow": torch.zeros(16, 16, 2)}, {"image": batch["image"]}) is None  # (no "flows" in the batch)


def test_the_flow_branch_is_taken_only_where_the_issue_says():
    c2w = torch.eye(4)[None, :3]
    cam0 = Camera(c2w, 50.0, 50.0, 8.0, 8.0, 16, 16, times=torch.tensor([[0.1]]))
    cam = Camera(c2w, 50.0, 50.0, 8.0, 8.0, 16, 16, times=torch.tensor([[0.2]]), metadata={"cameras0": cam0})
    on = _tiny_model(flow_loss_weight=0.5, warm_up=10)
    on.step = 20
    assert on.flow_camera0(cam) is cam0
    on.step = 5  # before the warm-up: only with the camera's motion in the flows
    assert on.flow_camera0(cam) is None
    moving = _tiny_model(flow_loss_weight=0.5, warm_up=10, flow_camera_motion=True)
    moving.step = 5
    assert moving.flow_camera0(cam) is cam0
    on.step = 20
    assert on.eval().flow_camera0(cam) is None and on.train().flow_camera0(cam) is cam0
    off = _tiny_model(warm_up=10)
    off.step = 20
    assert off.flow_camera0(cam) is None
    alone = Camera(c2w, 50.0, 50.0, 8.0, 8.0, 16, 16, times=torch.tensor([[0.2]]))
    assert on.flow_camera0(alone) is None
    alone.metadata["cameras0"] = alone  # (what get_outputs puts there itself)
    assert on.flow_camera0(alone) is None
    timeless = Camera(c2w, 50.0, 50.0, 8.0, 8.0, 16, 16, times=torch.tensor([[0.2]]), metadata={"cameras0": Camera(c2w, 50.0, 50.0, 8.0, 8.0, 16, 16)})
    assert on.flow_camera0(timeless) is None


def test_train_step_takes_flows_and_the_docs_name_the_fields():
    assert inspect.signature(harness.train_step).parameters["flows"].default is None
    readme = open(os.path.join(ROOT, "README.md")).read()
    for field in ("flow_loss_weight", "flow_camera_motion", "flow_frame0_grad"):
        assert field in readme, field
    assert "Flow supervision" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_ops_refuse_by_the_arguments_name():
    a, V, K = torch.randn(5, 3), torch.eye(4), torch.eye(3)
    with pytest.raises(_lib.FgRasterError, match="means_t is a CPU tensor"):
        ops.flow_displacement(a, a.clone(), V, None, K, 64, 48)
    with pytest.raises(ValueError, match="means_0"):
        ops.flow_displacement(a, torch.randn(4, 3), V, None, K, 64, 48)
    with pytest.raises(ValueError, match="viewmat_0"):
        ops.flow_displacement(a, a.clone(), V, torch.eye(3), K, 64, 48)
    with pytest.raises(NotImplementedError, match="viewmat_t requires a gradient"):
        ops.flow_displacement(a, a.clone(), V.clone().requires_grad_(True), None, K, 64, 48)
    with pytest.raises(NotImplementedError, match="viewmat_0 requires a gradient"):
        ops.flow_displacement(a, a.clone(), V, V.clone().requires_grad_(True), K, 64, 48)
    with pytest.raises(NotImplementedError, match="K requires a gradient"):
        ops.flow_displacement(a, a.clone(), V, None, K.clone().requires_grad_(True), 64, 48)
    pred, flows = torch.randn(8, 6, 2), torch.randn(17, 13, 2)
    with pytest.raises(_lib.FgRasterError, match="pred is a CPU tensor"):
        ops.flow_l1(pred, flows, None, 2)
    with pytest.raises(ValueError, match="pred"):
        ops.flow_l1(torch.randn(8, 6, 3), flows, None, 2)
    with pytest.raises(ValueError, match="pred"):
        ops.flow_l1(pred.double(), flows, None, 2)
    with pytest.raises(ValueError, match="pred is .* flows at downscale 2 is"):
        ops.flow_l1(torch.randn(9, 6, 2), flows, None, 2)
    with pytest.raises(ValueError, match="flows"):
        ops.flow_l1(pred, flows.double(), None, 2)
    with pytest.raises(ValueError, match="flows"):
        ops.flow_l1(pred, torch.randn(13, 17, 2).transpose(0, 1), None, 2)
    with pytest.raises(ValueError, match="downscale"):
        ops.flow_l1(pred, flows, None, 3)
    with pytest.raises(ValueError, match="mask"):
        ops.flow_l1(pred, flows, torch.ones(17, 13, dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="mask"):
        ops.flow_l1(pred, flows, torch.ones(8, 6), 2)


def test_header_declares_the_symbols_by_name_and_abi_numbers_stay():
    text = open(os.path.join(ROOT, "include", "fgraster.h")).read()
    assert re.search(r"#define FG_ABI_VERSION 14\b", text) and re.search(r"#define FG_ABI_MINOR 1\b", text)
    assert (_lib.ABI_VERSION, _lib.ABI_MINOR) == (14, 1)
    note = text[text.index("#define FG_ABI_MINOR") : text.index("#define FG_COUNT_OUT_WORDS")]
    names = ("fg_flow_disp_fwd", "fg_flow_disp_bwd", "fg_flow_l1_workspace_bytes", "fg_flow_l1_fwd", "fg_flow_l1_bwd")
    lib = _lib.load()
    for name in names:
        assert name in note and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"^(int|size_t) %s\(" % name, text, re.M), name
    for section, words in (("/* ---- FD ", ("VALIDITY RULE", "CANCELLATION-FREE FORM", "DETERMINISM")),
                           ("/* ---- FL ", ("TARGET AND WEIGHT", "DETERMINISM"))):  # fmt: skip
        body = text[text.index(section) :].split("*/")[0]
        assert "found BY NAME" in body and all(w in body for w in words), section
    assert lib.fg_abi_version() == 14 and lib.fg_abi_minor() == 1
    makefile = open(os.path.join(ROOT, "freegaussian_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", makefile, re.M).group(1).split()
    assert "flow_disp.hip" in srcs and "flow_loss.hip" in srcs


def test_argument_validation_returns_before_any_launch():
    """Through ctypes, without a GPU: every call here is refused (or has nothing to do) before it would launch."""
    lib = _lib.load()
    OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -4, -3
    at = lambda i: (1 << 30) + (i << 26)  # noqa: E731  addresses nobody reads, 64 MiB apart
    inf = math.inf
    dfwd = lambda *a: lib.fg_flow_disp_fwd(*a, None)  # noqa: E731
    dbwd = lambda *a: lib.fg_flow_disp_bwd(*a, None)  # noqa: E731
    N = 1000
    assert dfwd(0, at(0), 3, at(1), 3, at(2), None, at(4), 64, 48, 0.01, inf, at(5)) == OK
    assert dfwd(-1, at(0), 3, at(1), 3, at(2), None, at(4), 64, 48, 0.01, inf, at(5)) == INVALID
    assert dfwd(2**38 + 1, at(0), 3, at(1), 3, at(2), None, at(4), 64, 48, 0.01, inf, at(5)) == UNSUPPORTED
    assert dfwd(N, at(0), 2, at(1), 3, at(2), None, at(4), 64, 48, 0.01, inf, at(5)) == INVALID
    assert dfwd(N, at(0), 3, at(1), 3, None, None, at(4), 64, 48, 0.01, inf, at(5)) == INVALID
    assert dfwd(N, at(0), 3, at(1), 3, at(2), None, at(4), 64, 48, -1.0, inf, at(5)) == INVALID
    assert dfwd(N, at(0), 3, at(1), 3, at(2), None, at(4), 64, 48, 0.01, math.nan, at(5)) == INVALID
    assert dfwd(N, at(0), 3, at(1), 3, at(2), None, at(4), 64, 48, 0.01, inf, at(1)) == INVALID  # disp on means_0
    assert dbwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01, inf, at(5), None, None) == OK  # nothing asked for
    assert dbwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01, inf, at(5), at(6), at(6)) == INVALID
    assert dbwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01, inf, at(5), at(3), None) == INVALID  # on viewmat_0
    assert lib.fg_flow_l1_workspace_bytes(67, 35, 2) == 64 and lib.fg_flow_l1_workspace_bytes(67, 35, 3) == 0
    lfwd = lambda *a: lib.fg_flow_l1_fwd(*a, None)  # noqa: E731
    lbwd = lambda *a: lib.fg_flow_l1_bwd(*a, None)  # noqa: E731
    assert lfwd(33, 17, at(0), 6, 102, 67, 35, 2, at(1), None, 0, at(3), 0, at(4)) == WORKSPACE
    assert lfwd(33, 17, at(0), 6, 102, 67, 35, 3, at(1), None, 0, at(3), 64, at(4)) == UNSUPPORTED
    assert lfwd(32, 17, at(0), 6, 102, 67, 35, 2, at(1), None, 0, at(3), 64, at(4)) == INVALID  # H != H0 // d
    assert lfwd(33, 17, at(0), 1, 102, 67, 35, 2, at(1), None, 0, at(3), 64, at(4)) == INVALID
    assert lfwd(33, 17, at(0), 6, 97, 67, 35, 2, at(1), None, 0, at(3), 64, at(4)) == INVALID
    assert lfwd(33, 17, at(0), 6, 102, 67, 35, 2, at(1), None, 0, at(1), 64, at(4)) == INVALID  # the workspace on flows
    assert lbwd(33, 17, at(0), 6, 102, 67, 35, 2, at(1), None, 0, at(3), at(4), at(0)) == INVALID  # g_pred on pred
    assert lbwd(33, 17, at(0), 6, 102, 67, 35, 2, at(1), None, 0, at(3), at(4), None) == INVALID


def test_the_flow_check_program_builds_and_passes(tmp_path):
    """``make flow-check``: the entry points' argument validation under the host sanitizers, in a program of its own."""
    csrc = os.path.join(ROOT, "freegaussian_amd", "csrc")
    run = subprocess.run(["make", "-C", csrc, "flow-check"], capture_output=True, text=True, timeout=600)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0 and "flow_args: ok" in run.stdout
