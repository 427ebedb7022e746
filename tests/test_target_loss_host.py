"""The fused training target's restatement (tests/target_loss_restatement.py), its cases and the Python side of the knob
``FG_FUSED_TARGET``, checked on the CPU.

    the float64 restatement is the model's present torch path in float64 (``get_gt_img`` + ``composite_with_background`` + the
        mask lines + ``harness.ssim`` + ``mse_loss``), values and gradient, to 1e-12 -- the new definition is tied to code that is
        already pinned to the reference.  ``utils.resize_image`` casts to float32 before it pools; its pooling call
        (``avg_pool2d(kernel_size=d, stride=d)``) is made here on the float64 image.  At d = 1 the image goes through
        ``get_gt_img`` itself.
    the g_loss.npz cases through the restatement, at the bars of tests/test_reference_goldens.py
    every mutant at least 4 * F * E32 away on three quarters of the elements it concerns: this caps F
    the knob, ``fused_target_applies``, the refusals of ``ops.target_loss``, and no call into it with the knob unset

``harness.ssim`` builds its window in fp32 (tests/test_loss_rows_host.py): the comparison with it hands the restatement the
harness's window, everything else uses the kernel's."""
import functools

import pytest
import torch
import torch.nn.functional as Fn

import loss_restatement as L
import parity_common as P
import target_loss_restatement as T
import test_reference_goldens as RG
from freegaussian_amd import _lib, harness, ops
from freegaussian_amd.model import FUSED_TARGET_KEY, FreeGaussianModel, FreeGaussianModelConfig

G, LOSS = RG.G, RG.LOSS

CASES = T.CASES


@functools.lru_cache(maxsize=None)
def case(i):
    return T.make_case(*CASES[i])


@functools.lru_cache(maxsize=None)
def evaluated(i, dtype, mutant=None):
    c = case(i)
    return T.evaluate(c["pred"], c["src"], c["bg"], c["mask"], c["d"], dtype, mutant)


def _model(d=1):
    cfg = FreeGaussianModelConfig(**{**G.OUTPUT_BASE, **G.LOSS_BASE, "num_downscales": {1: 0, 2: 1, 4: 2, 8: 3}[d]})
    m = FreeGaussianModel(cfg, num_points=G.LOSS_N, init_scales=0.0, num_train_data=G.BIL_NUM).train()
    m.step = 0
    assert m._get_downscale_factor() == d
    return m


def _torch_path64(m, pred, src, bg, mask, d, group):
    """The model's torch statement in float64 -> l1, ssim, mse, d (v_l1 l1 + v_ssim ssim) / d pred."""
    pool = lambda t: Fn.avg_pool2d(t.permute(2, 0, 1)[None], kernel_size=d, stride=d)[0].permute(1, 2, 0)  # noqa: E731
    img = src.double() / 255.0 if src.dtype == torch.uint8 else src.double()
    img = m.get_gt_img(img) if d == 1 else pool(img)
    gt = m.composite_with_background(img, bg.double())
    x = pred.double().requires_grad_(True)
    gt_m, x_m = gt, x
    if mask is not None:
        mk = mask.double() if d == 1 else pool(mask.double())
        gt_m, x_m = gt * mk, x * mk
    l1 = (gt_m - x_m).abs().mean()
    ss = harness.ssim(gt_m.permute(2, 0, 1)[None], x_m.permute(2, 0, 1)[None])
    mse = Fn.mse_loss(x, gt)
    v_l1, v_ssim = T.COTANGENTS[group]
    (v_l1 * l1 + v_ssim * ss).backward()
    return l1.detach(), ss.detach(), mse.detach(), x.grad


@pytest.mark.parametrize("i", range(len(CASES)))
def test_float64_restatement_is_the_models_torch_path(i):
    c = case(i)
    m = _model(1)  # (d = 1: get_gt_img hands the float64 image through; the other cases pool here, see the head of the file)
    r = T.evaluate(c["pred"], c["src"], c["bg"], c["mask"], c["d"], torch.float64, w2d=harness._gauss_window())
    for group in T.GROUPS:
        l1, ss, mse, g = _torch_path64(m, c["pred"], c["src"], c["bg"], c["mask"], c["d"], group)
        assert abs(float(r["l1"]) - float(l1)) <= 1e-12 and abs(float(r["ssim"]) - float(ss)) <= 1e-12
        assert abs(float(r["mse"]) - float(mse)) <= 1e-12
        live = r["grads"][group][1] > 0  # (A = 0: a masked-out pixel, or an L1 tie with no SSIM cotangent; both exactly zero)
        assert bool((g[~live] == 0).all()) and bool((r["grads"][group][0][~live] == 0).all())
        d = P.distance(r["grads"][group][0][live], g[live], r["grads"][group][1][live])
        assert float(d.max()) <= 1e-12, (group, float(d.max()))


def test_the_models_own_downscale_agrees_at_fp32():
    """``get_gt_img`` at d = 2 (``resize_image``: float32) against the restatement's float64 target: the reference's own bar."""
    c = case(1)
    gt = _model(2).composite_with_background(_model(2).get_gt_img(c["src"]), c["bg"])
    assert RG.rel_err(gt, T.target(c["src"], c["bg"], None, 2, torch.float64)[0]) < RG.REL_TOL


@pytest.mark.parametrize("tag,step,over,layout", G.LOSS_CASES, ids=[c[0] for c in G.LOSS_CASES])
def test_reference_loss_fixtures_through_the_restatement(tag, step, over, layout):
    """The g_loss.npz cases (the reference's own methods in float64): composited target, L1 / SSIM as the main loss, PSNR and
    the gradient of pred, at the bars of tests/test_reference_goldens.py."""
    d = int(LOSS[f"{tag}.meta"][1])
    pred, bg, image = LOSS[f"{tag}.in.pred"], LOSS[f"{tag}.in.background"], LOSS[f"{tag}.in.image"]
    mask = LOSS[f"{tag}.in.mask"] if f"{tag}.in.mask" in LOSS else None
    lam = {**G.LOSS_BASE, **over}["ssim_lambda"]
    r = T.evaluate(pred, image, bg, mask, d, torch.float64, groups=())
    assert RG.rel_err(r["gt"], LOSS[f"{tag}.composited"]) < RG.REL_TOL, tag
    main = (1 - lam) * r["l1"] + lam * (1 - r["ssim"])
    assert RG.rel_err(main.reshape(1), LOSS[f"{tag}.loss.main_loss"].reshape(1)) < RG.REL_TOL, tag
    assert RG.rel_err((-10.0 * torch.log10(r["mse"])).reshape(1), LOSS[f"{tag}.psnr"].reshape(1)) < RG.REL_TOL, tag
    xm, ym = (pred.double() * r["m"], r["gt"] * r["m"]) if mask is not None else (pred.double(), r["gt"])
    fwd = L.forward(xm, ym, torch.float64)
    grad, _ = L.backward(xm, ym, fwd, 1 - lam, -lam, torch.float64)
    grad = grad * r["m"] if mask is not None else grad
    assert RG.rel_l2(grad, LOSS[f"{tag}.grad_pred"]) < RG.REL_TOL, tag


def test_census_every_class_occurs_and_ties_are_exact():
    """Across the cases: every loss regime, every alpha class and every mask class; a fractional mask from a bool mask (a block
    that straddles an edge) and from a float one; exact ties of pred and target; and no decision that depends on rounding:
    sign(pred m - gt m) is the same in fp32 and float64 on every element."""
    seen = set()
    for i in range(len(CASES)):
        c, r32, r64 = case(i), evaluated(i, torch.float32), evaluated(i, torch.float64)
        seen |= set(T.label_masks(c))
        if c["mask"] is not None and bool((c["mask_class"] == 2).any()):
            seen.add("frac_from_" + ("bool" if c["mask"].dtype == torch.bool else "float"))
        m32, m64 = (1.0, 1.0) if c["mask"] is None else (r32["m"], r64["m"])
        s32 = torch.sign(c["pred"] * m32 - r32["gt"] * m32)
        s64 = torch.sign(c["pred"].double() * m64 - r64["gt"] * m64)
        assert torch.equal(s32.double(), s64), CASES[i]
        if bool(((s64 == 0) & (torch.as_tensor(m64) != 0)).any()):
            seen.add("ties")
        H0, W0 = c["src"].shape[:2]
        assert (H0, W0) == (c["H"] * c["d"] + CASES[i][6][0], c["W"] * c["d"] + CASES[i][6][1])
    want = set(L.REGIMES) | set(T.ALPHA_CLASSES) | set(T.MASK_CLASSES) | {"frac_from_bool", "frac_from_float", "ties"}
    assert seen == want, want ^ seen
    # what the issue asks the ten cases to cover
    ds = {(c[2], c[4]) for c in CASES}
    assert {d for d, _ in ds} == {1, 2, 4, 8} and all((d, f) in ds for d in (2, 4, 8) for f in (False, True))
    assert {c[3] for c in CASES} == {3, 4} and {c[5] for c in CASES} == {None, "bool", "float"}
    assert any(c[6][0] > 0 and c[6][1] > 0 for c in CASES) and {(c[0], c[1]) for c in CASES} == set(L.SHAPES)


def element_e32(i, group):
    """-> (E32 per label of case i and group, [H,W,3] the LARGEST E32 among the labels an element carries: the loosest bound the
    GPU test holds it to)."""
    c, r32, r64 = case(i), evaluated(i, torch.float32), evaluated(i, torch.float64)
    masks = T.label_masks(c)
    e32 = P.yardstick(masks, P.distance(r32["grads"][group][0], *r64["grads"][group]), T.FLOOR)
    per = torch.zeros(c["H"], c["W"], dtype=torch.float64)
    for name, mk in masks.items():
        per = torch.where(mk, torch.clamp_min(per, e32[name]), per)
    return e32, per[..., None].expand(c["H"], c["W"], 3)


SSIM_GROUPS = ("ssim", "both")
FLAT = ("white_equal", "black_equal", "flat_offset")
# (mutant, case index, what it concerns, the cotangent groups that drive it)
MUTANT_CASES = [
    ("composite_before_downscale", 1, "alpha_frac", SSIM_GROUPS),
    ("composite_before_downscale", 5, "alpha_frac", SSIM_GROUPS),
    # (a uniform 0.4 % of the target hardly moves the SSIM gradient; what / 256 breaks on every element is a tie with a target
    #  above zero: the L1 sign goes from 0 to 1 -- and it moves the first and the third value, below)
    ("div_256", 0, "ties above zero", ("l1", "both")),
    ("div_256", 4, "ties above zero", ("l1", "both")),
    ("mask_on_pred_only", 1, "mask_frac", SSIM_GROUPS),
    ("mask_on_pred_only", 5, "mask_frac", SSIM_GROUPS),
    ("mask_first_pixel", 1, "mask_frac", SSIM_GROUPS),
    ("mask_first_pixel", 5, "mask_frac", SSIM_GROUPS),
    ("alpha_complement_dropped", 3, "alpha below 1", SSIM_GROUPS),
    ("remainder_rows_in_last_block", 3, "last row", SSIM_GROUPS),
    ("remainder_rows_in_last_block", 6, "last row", SSIM_GROUPS),
]


def _concerned(i, what):
    c = case(i)
    if what == "ties above zero":
        gt = evaluated(i, torch.float64)["gt"]
        return (c["pred"].double() == gt) & (gt > 0)
    if what == "alpha_frac":
        sel = c["alpha_class"] == 2
    elif what == "mask_frac":
        sel = c["mask_class"] == 2
    elif what == "alpha below 1":
        sel = (c["alpha_class"] == 0) | (c["alpha_class"] == 2)
    else:  # the last output row
        sel = torch.zeros(c["H"], c["W"], dtype=torch.bool)
        sel[-1] = True
    if c["mask"] is not None:
        sel = sel & (c["mask_class"] != 0)  # (where the mask is 0 the gradient is exactly zero, whatever the target)
    if what != "last row":  # (as in tests/test_loss_rows_host.py: on the flat blocks the SSIM gradient all but vanishes in its A)
        sel = sel & ~sum((c["regime"] == L.REGIMES.index(n)) for n in FLAT).bool()
    return sel[..., None].expand(c["H"], c["W"], 3)


def mutant_cells():
    """-> {(mutant, case, group): (elements, cap)}; cap: the largest F at which three quarters of the concerned gradient
    elements are still 4 * F * E32 of their accumulation from the true gradient."""
    out = {}
    for mutant, i, what, groups in MUTANT_CASES:
        r64, rm = evaluated(i, torch.float64), evaluated(i, torch.float64, mutant)
        sel = _concerned(i, what)
        for group in groups:
            _, per = element_e32(i, group)
            d = P.distance(rm["grads"][group][0], *r64["grads"][group])
            ratios = (d / per)[sel]
            out[(mutant, i, group)] = (ratios.numel(), P.three_quarter_cap(ratios))
    return out


def test_mutants_are_caught():
    """Every mutant's float64 gradient is at least 4 * F * E32 of the element's accumulation from the true one on three quarters
    of the elements it concerns (E32: the largest of the element's labels, the loosest bound it is held to); ``mse_on_masked``
    concerns one number, the third value, and is that far from it; ``div_256`` moves the first and the third value as well.
    The smallest cap bounds F."""
    assert {c[0] for c in MUTANT_CASES} | {"mse_on_masked"} == set(T.MUTANTS)
    factor = 1.0 if T.F is None else T.F
    cells = mutant_cells()
    for (mutant, i, group), (n, cap) in cells.items():
        print(f"{mutant} case {i} {group}: {n} elements; caps F at {cap:.1f}")
    caps = [v[1] for v in cells.values()]
    for mutant, i, keys in (("mse_on_masked", 1, ("mse",)), ("mse_on_masked", 5, ("mse",)), ("div_256", 0, ("l1", "mse")),
                            ("div_256", 4, ("l1", "mse"))):  # fmt: skip
        r32, r64, rm = evaluated(i, torch.float32), evaluated(i, torch.float64), evaluated(i, torch.float64, mutant)
        for k in keys:
            e32 = max(float(P.distance(r32[k], r64[k], r64[k + "_acc"])), T.FLOOR)
            ratio = float(P.distance(rm[k], r64[k], r64[k + "_acc"])) / e32
            print(f"{mutant} case {i}: the value {k} is {ratio:.1f} x E32 ({e32:.2e}) away; caps F at {ratio / 4:.1f}")
            caps.append(ratio / 4)
    print(f"the cap on F: {min(caps):.1f}")
    assert all(n > 0 for n, _ in cells.values())
    assert min(caps) >= factor, min(caps)
    assert T.F is None or T.F <= min(caps)


def test_yardsticks_are_floored_and_finite():
    for i in range(len(CASES)):
        r32, r64 = evaluated(i, torch.float32), evaluated(i, torch.float64)
        for group in T.GROUPS:
            assert bool(torch.isfinite(r64["grads"][group][0]).all()) and bool((r64["grads"][group][1] >= 0).all())
            for name, e in element_e32(i, group)[0].items():
                assert T.FLOOR <= e < 1e-2, (CASES[i], group, name, e)
        for k in T.VALUES:
            assert float(P.distance(r32[k], r64[k], r64[k + "_acc"])) < 1e-4, (CASES[i], k)
        if case(i)["mask"] is not None:  # the exact-zero rule has something to hold
            dead = (r64["m"] == 0).expand_as(r64["grads"]["both"][0])
            assert bool(dead.any()) and bool((r64["grads"]["both"][0][dead] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# the Python side


def test_knob_parsing(monkeypatch):
    monkeypatch.delenv("FG_FUSED_TARGET", raising=False)
    assert harness.fused_target() is False
    monkeypatch.setenv("FG_FUSED_TARGET", "0")
    assert harness.fused_target() is False
    monkeypatch.setenv("FG_FUSED_TARGET", "1")
    assert harness.fused_target() is True
    for bad in ("", "2", "on", "true", " 1"):
        monkeypatch.setenv("FG_FUSED_TARGET", bad)
        with pytest.raises(ValueError, match="FG_FUSED_TARGET"):
            harness.fused_target()


def _good():
    return torch.zeros(20, 30, 3), torch.zeros(41, 61, 4, dtype=torch.uint8), torch.zeros(41, 61, 1, dtype=torch.bool), 2


def test_fused_target_applies():
    pred, image, mask, d = _good()
    ok = harness.target_shapes_supported
    assert ok(pred, image, mask, d) and ok(pred, image, None, d) and ok(pred, image.float(), mask.float()[..., 0], d)
    assert ok(pred, image[..., :3].contiguous(), mask.to(torch.uint8), d)
    # a host-resident batch keeps the torch path, whatever its shapes
    assert not harness.fused_target_applies(pred, image, mask, d) and not harness.fused_target_applies(pred, image, None, d)
    assert not ok(pred[:19], image, mask, d) and not ok(pred[:, :29], image, mask, d)  # a wrong pred size
    assert not ok(pred, image, mask, 3) and not ok(torch.zeros(41, 61, 3), image, mask, 0) and not ok(pred, image, mask, 16)
    assert not ok(pred, image.double(), mask, d) and not ok(pred.double(), image, mask, d) and not ok(pred, image, mask.double(), d)
    assert not ok(pred, image[..., :2].contiguous(), mask, d) and not ok(pred, image[..., :3], mask, d)  # channels; a view
    assert not ok(pred, image, mask[:40], d) and not ok(pred[..., :2], image, mask, d)
    assert not ok(torch.zeros(10, 30, 3), torch.zeros(20, 60, 3), None, 2)  # below the SSIM window


def test_target_loss_refusals():
    pred, image, mask, d = _good()
    bg = torch.zeros(3)
    with pytest.raises(_lib.FgRasterError, match="composite_with_background"):  # CPU tensors: names the torch statement
        ops.target_loss(pred, image, bg, mask, d)
    with pytest.raises(_lib.FgRasterError, match="GPU only"):
        ops.target_loss(pred, image[..., :3].contiguous(), None, None, d)
    for args in ((pred.double(), image, bg, mask, d), (pred[..., :2], image, bg, mask, d), (pred, image.double(), bg, mask, d),
                 (pred, image[..., :2].contiguous(), bg, mask, d), (pred, image[..., :3], None, mask, d),
                 (pred, image, bg, mask, 3), (pred, image, bg, mask, 16), (pred[:19], image, bg, mask, d),
                 (torch.zeros(10, 30, 3), torch.zeros(20, 60, 3), None, None, 2), (pred, image, None, mask, d),
                 (pred, image, bg.double(), mask, d), (pred, image, torch.zeros(4), mask, d), (pred, image, bg, mask.double(), d),
                 (pred, image, bg, mask[:40], d)):  # fmt: skip
        with pytest.raises(ValueError):
            ops.target_loss(*args)


@pytest.mark.parametrize("knob", [None, "0", "1"])
def test_no_fused_call_on_the_torch_path(monkeypatch, knob):
    """With the knob unset or 0, ``get_loss_dict`` / ``get_metrics_dict`` never reach ``ops.target_loss``; with the knob set a
    host-resident batch does not either (``fused_target_applies``).  The values are those of the torch statement."""

    def boom(*a, **k):
        raise AssertionError("ops.target_loss was called")

    monkeypatch.setattr(ops, "target_loss", boom)
    if knob is None:
        monkeypatch.delenv("FG_FUSED_TARGET", raising=False)
    else:
        monkeypatch.setenv("FG_FUSED_TARGET", knob)
    c = case(1)
    m = _model(2)
    outputs = {"rgb": c["pred"].clone().requires_grad_(True), "background": c["bg"]}
    batch = {"image": c["src"], "mask": c["mask"]}
    metrics = m.get_metrics_dict(outputs, batch)
    loss = m.get_loss_dict(outputs, batch)
    assert FUSED_TARGET_KEY not in outputs
    r = evaluated(1, torch.float64)
    want = 0.8 * r["l1"] + 0.2 * (1 - r["ssim"])
    assert RG.rel_err(loss["main_loss"].reshape(1), want.reshape(1)) < RG.REL_TOL
    assert RG.rel_err(metrics["psnr"].reshape(1), (-10.0 * torch.log10(r["mse"])).reshape(1)) < RG.REL_TOL
