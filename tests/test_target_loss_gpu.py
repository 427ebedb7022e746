"""The fused training target (csrc/target_loss.hip) in isolation and in the model: ``ops.target_loss`` -- fg_target_loss_fwd,
fg_target_loss_bwd -- on the cases of tests/target_loss_restatement.py, every gradient element and the three values compared
with the float64 restatement, one cotangent group at a time; then ``get_loss_dict`` / ``get_metrics_dict`` /
``harness.train_step`` under ``FG_FUSED_TARGET=1`` against the knob-unset path of the same process.

Output shapes are loss_restatement.SHAPES (tests/test_loss_rows_gpu.py says which tiling case of the 32 x 16 tile each one
reaches).  The ten cases (target_loss_restatement.CASES):
     58 x 106  d 1  RGBA uint8                       the plain blender batch: composite, no downscale
     58 x 106  d 2  RGBA uint8, bool mask,  +1 +1    a block that straddles a mask edge; remainder row and column
     58 x 106  d 2  RGB float32, float mask, +0 +1   a fractional float mask
     53 x 75   d 4  RGBA float32, bool mask, +3 +2   128-bit pixel loads; remainders
     53 x 75   d 4  RGB uint8,               +1 +3   byte loads at stride 3
     53 x 75   d 8  RGBA uint8, float mask,  +7 +5   the largest block, the largest remainders
     12 x 43   d 8  RGB float32, bool mask,  +3 +0
     11 x 11   d 1  RGB float32, float mask          one map pixel
     11 x 11   d 2  RGBA float32,            +1 +1
     12 x 43   d 1  RGBA uint8, bool mask

PER ELEMENT, every group:  |g_hip - g64| / A64  <=  F * E32(label, group) for each label the element carries -- its loss
    regime, its alpha class, its mask class -- no element left out; where the mask is 0 the gradient is EXACTLY zero (those
    elements take no part in a label's maximum).
THE THREE VALUES: within F x the fp32 restatement's own (floored) distance from float64; bit-identical on repetition, as is
    the gradient.
tests/parity_common.py has the protocol (A, E32, the floor, F); F and FLOOR are target_loss_restatement's, the recorded table
is in profiles/target_loss_parity.md.

``PYTHONPATH=. python tests/test_target_loss_gpu.py REPORT.jsonl`` turns the records of a run under FG_PARITY_REPORT into the
table of profiles/target_loss_parity.md.
"""
import copy
import functools
import sys

import pytest
import torch

import parity_common as P
import target_loss_restatement as T
import test_reference_goldens as RG
from freegaussian_amd import harness, ops
from freegaussian_amd.model import FUSED_TARGET_KEY, Camera, FreeGaussianModel, FreeGaussianModelConfig
from parity_common import need_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
G, LOSS = RG.G, RG.LOSS


def _tag(i):
    H, W, d, ch, f32, mask, rem, _ = T.CASES[i]
    return f"{H}x{W} d{d} {'rgba' if ch == 4 else 'rgb'} {'f32' if f32 else 'u8'} {mask or 'nomask'} +{rem[0]}+{rem[1]}"


@functools.lru_cache(maxsize=None)
def _reference(i):
    """The case, its label masks (live elements only), the float64 evaluation, E32 per group and per value; once per case."""
    c = T.make_case(*T.CASES[i])
    ev = lambda dtype: T.evaluate(c["pred"], c["src"], c["bg"], c["mask"], c["d"], dtype)  # noqa: E731
    r32, r64 = ev(torch.float32), ev(torch.float64)
    dead = torch.zeros(c["H"], c["W"], dtype=torch.bool) if c["mask"] is None else (r64["m"] == 0).reshape(c["H"], c["W"])
    masks = P.restrict(T.label_masks(c), ~dead)
    e32 = {g: P.yardstick(masks, P.distance(r32["grads"][g][0], *r64["grads"][g]), T.FLOOR) for g in T.GROUPS}
    e32_val = {k: max(float(P.distance(r32[k], r64[k], r64[k + "_acc"])), T.FLOOR) for k in T.VALUES}
    return c, masks, dead, r64, e32, e32_val


def _on_device(c):
    return c["src"].to(DEV), (c["bg"].to(DEV) if c["src"].shape[-1] == 4 else None), (None if c["mask"] is None else c["mask"].to(DEV))


def _run_hip(c, group):
    src, bg, mask = _on_device(c)
    x = c["pred"].to(DEV).requires_grad_(True)
    l1, ss, mse = ops.target_loss(x, src, bg, mask, c["d"])
    assert not mse.requires_grad
    v_l1, v_ssim = T.COTANGENTS[group]
    # a group's loss leaves the other output unused: autograd hands its cotangent over as None
    loss = v_l1 * l1 if group == "l1" else (v_ssim * ss if group == "ssim" else v_l1 * l1 + v_ssim * ss)
    loss.backward()
    torch.cuda.synchronize()
    return torch.stack([l1.detach(), ss.detach(), mse]).cpu(), x.grad.cpu()


@pytest.mark.parametrize("i", range(len(T.CASES)), ids=[_tag(i).replace(" ", "_") for i in range(len(T.CASES))])
def test_every_element(i):
    c, masks, dead, r64, e32, e32_val = _reference(i)
    tag = _tag(i)
    failures = []
    values = []
    for group in T.GROUPS:
        vals, g = _run_hip(c, group)
        values.append(vals)
        assert g.shape == c["pred"].shape
        broken = (g[dead] != 0) | torch.isnan(g[dead])
        if bool(broken.any()):
            failures.append(f"{tag} {group}: {int(broken.sum())} elements under a mask of 0 are not exactly zero")
        P.check(f"{tag}|{group}|{{regime}}", masks, P.distance(g, *r64["grads"][group]), e32[group], T.F, failures)
        if group == "both":  # bit for bit on repetition, forward and backward
            vals2, g2 = _run_hip(c, group)
            assert torch.equal(vals, vals2) and torch.equal(g, g2), "two runs differ"
    for vals in values[1:]:
        assert torch.equal(vals, values[0]), "the three values differ between two calls"
    for k, s in zip(T.VALUES, values[0]):
        ratio = float(P.distance(s, r64[k], r64[k + "_acc"])) / e32_val[k]
        P.check_cell(f"{tag}|value|{k}", ratio, e32_val[k], T.F, failures, f"{float(s)!r} for {float(r64[k])!r}")
    assert not failures, "\n".join(failures)


def test_F_is_set_below_the_mutant_caps():
    """F is not a free number: 4 x the worst recorded ratio, rounded up to a power of two (profiles/target_loss_parity.md), and
    at most the smallest mutant cap of tests/test_target_loss_host.py."""
    import test_target_loss_host as Hst

    caps = [cap for _, cap in Hst.mutant_cells().values()]
    assert T.F is None or T.F <= min(caps), (T.F, min(caps))


def test_forward_alone_keeps_no_maps():
    """A ``pred`` that needs no gradient (or a call under no_grad): the same three values, nothing saved for a backward."""
    c = _reference(1)[0]
    src, bg, mask = _on_device(c)
    x = c["pred"].to(DEV)
    want = torch.stack([v.detach() for v in ops.target_loss(x.clone().requires_grad_(True), src, bg, mask, c["d"])])
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    out = ops.target_loss(x, src, bg, mask, c["d"])
    assert all(not v.requires_grad and v.grad_fn is None for v in out)
    # (what stays allocated: the three values' own buffer, far below the 3 x 3 x 48 x 96 floats of the maps)
    assert torch.cuda.memory_allocated() - base < 3 * 3 * 48 * 96 * 4
    assert torch.equal(torch.stack(out), want)
    with torch.no_grad():
        out = ops.target_loss(x.clone().requires_grad_(True), src, bg, mask, c["d"])
    assert all(v.grad_fn is None for v in out) and torch.equal(torch.stack(out), want)


def test_applies_and_refusals_on_the_device():
    c = _reference(1)[0]
    src, bg, mask = _on_device(c)
    x = c["pred"].to(DEV)
    assert harness.fused_target_applies(x, src, mask, 2) and harness.fused_target_applies(x, src, None, 2)
    assert not harness.fused_target_applies(x, src.cpu(), mask, 2) and not harness.fused_target_applies(x, src, mask.cpu(), 2)
    assert not harness.fused_target_applies(x[:57], src, mask, 2) and not harness.fused_target_applies(x, src, mask, 4)
    assert not harness.fused_target_applies(x, src.double(), mask, 2) and not harness.fused_target_applies(x, src, mask, 3)
    for args in ((x, src, None, mask, 2), (x, src, bg, mask, 4), (x[:57], src, bg, mask, 2), (x, src.double(), bg, mask, 2)):
        with pytest.raises(ValueError):
            ops.target_loss(*args)


# ---------------------------------------------------------------------------------------------------------------------
# the model


def _model(d, **over):
    cfg = FreeGaussianModelConfig(**{**G.OUTPUT_BASE, **G.LOSS_BASE, "num_downscales": {1: 0, 2: 1, 4: 2, 8: 3}[d], **over})
    m = FreeGaussianModel(cfg, num_points=G.LOSS_N, init_scales=0.0, num_train_data=G.BIL_NUM).to(DEV).train()
    m.step = 0
    assert m._get_downscale_factor() == d
    return m


def _count_calls(monkeypatch):
    calls = []
    real = ops.target_loss

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "target_loss", counted)
    return calls


def _loss_and_metrics(m, pred, bg, batch, metrics_first, strict):
    """-> main loss, psnr, d main loss / d pred, the outputs dict; both methods on ONE outputs dict, in either order.
    ``strict``: with host synchronisation forbidden (the torch path's scalar constants are host-to-device copies: it cannot)."""
    x = pred.clone().requires_grad_(True)
    outputs = {"rgb": x, "background": bg}
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    if strict:
        torch.cuda.set_sync_debug_mode("error")
    try:
        if strict:
            with pytest.raises(RuntimeError):  # the canary: a read-back under the same mode must raise
                torch.ones(4, device=DEV).nonzero()
        if metrics_first:
            metrics = m.get_metrics_dict(outputs, batch)
        loss = m.get_loss_dict(outputs, batch)
        if not metrics_first:
            metrics = m.get_metrics_dict(outputs, batch)
        loss["main_loss"].backward()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    return loss["main_loss"].detach(), metrics["psnr"].detach(), x.grad, outputs


# (case index): an RGBA uint8 batch (d = 1) and an RGB float batch with a mask (d = 2)
@pytest.mark.parametrize("i,metrics_first", [(0, True), (0, False), (2, True), (2, False)])
def test_model_agrees_with_the_torch_path(monkeypatch, i, metrics_first):
    c = _reference(i)[0]
    m = _model(c["d"])
    src, _, mask = _on_device(c)
    bg, pred = c["bg"].to(DEV), c["pred"].to(DEV)
    batch = {"image": src} if mask is None else {"image": src, "mask": mask}
    calls = _count_calls(monkeypatch)
    monkeypatch.delenv("FG_FUSED_TARGET", raising=False)
    want = _loss_and_metrics(m, pred, bg, batch, metrics_first, strict=False)
    assert not calls and FUSED_TARGET_KEY not in want[3]
    monkeypatch.setenv("FG_FUSED_TARGET", "1")
    got = _loss_and_metrics(m, pred, bg, batch, metrics_first, strict=True)
    assert len(calls) == 1, "the second of the two methods made a fused call of its own"
    kept = got[3][FUSED_TARGET_KEY]
    assert kept[0] is batch["image"] and kept[1] is batch.get("mask")
    assert RG.rel_err(got[0].reshape(1), want[0].reshape(1)) < RG.REL_TOL
    assert RG.rel_err(got[1].reshape(1), want[1].reshape(1)) < RG.REL_TOL
    assert RG.rel_l2(got[2], want[2]) < RG.REL_TOL
    # another batch object on the same outputs is not served from the kept call
    m.get_metrics_dict(got[3], {**batch, "image": src.clone()})
    assert len(calls) == 2


def test_color_corrected_metrics_keep_the_torch_statement(monkeypatch):
    c = _reference(0)[0]
    m = _model(1, color_corrected_metrics=True)
    src, _, _ = _on_device(c)
    outputs = {"rgb": c["pred"].to(DEV).requires_grad_(True), "background": c["bg"].to(DEV)}
    calls = _count_calls(monkeypatch)
    monkeypatch.setenv("FG_FUSED_TARGET", "1")
    metrics = m.get_metrics_dict(outputs, {"image": src})
    assert not calls and "cc_psnr" in metrics
    m.get_loss_dict(outputs, {"image": src})
    assert len(calls) == 1  # (the loss is still fused)


@pytest.mark.parametrize("case", G.LOSS_CASES, ids=[c[0] for c in G.LOSS_CASES])
def test_reference_loss_fixtures_with_the_knob(monkeypatch, case):
    """tests/test_reference_goldens.py's loss cases with the batch tensors on the device and the knob set, at its bars: every
    case runs fused (uint8 or float32 images)."""
    tag = case[0]
    monkeypatch.setenv("FG_FUSED_TARGET", "1")
    calls = _count_calls(monkeypatch)
    moved = {k: (v.to(DEV) if k in (f"{tag}.in.image", f"{tag}.in.mask") else v) for k, v in LOSS.items()}
    monkeypatch.setattr(RG, "LOSS", moved)
    RG._run_loss(case, DEV)
    assert len(calls) == 2, (tag, len(calls))  # (_run_loss hands the two methods two outputs dicts)


def test_train_step_with_the_knob(monkeypatch):
    """One ``harness.train_step`` on a tiny RGBA scene, knob set against knob unset from the same state: the same loss and
    PSNR, one fused call, and the read-back takes the stored squared error (no target is composited)."""
    from freegaussian_amd.scenes import look_at_viewmat

    W, H = 64, 48
    torch.manual_seed(0)
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(800, 3) - 0.5) * 2.0, init_scales=-3.2)
    model.step = 1500
    model = model.to(DEV).train()
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1
    cam = Camera(c2w[None, :3], 56.0, 60.0, W / 2, H / 2, W, H, times=torch.tensor([[0.4]]))
    g = torch.Generator().manual_seed(3)
    rgba = (torch.rand(H, W, 4, generator=g) * 255).to(torch.uint8)
    rgba[: H // 2, :, 3] = 255
    rgba = rgba.to(DEV)
    res = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("FG_FUSED_TARGET", knob)
        mdl = copy.deepcopy(model)
        calls = _count_calls(monkeypatch)
        composited = []
        real = mdl.composite_with_background
        mdl.composite_with_background = lambda *a, **k: (composited.append(1), real(*a, **k))[1]
        res[knob] = harness.train_step(mdl, harness.build_optimizers(mdl), copy.deepcopy(cam), rgba, 1500)
        assert len(calls) == (1 if knob == "1" else 0)
        assert bool(composited) == (knob == "0")
        monkeypatch.undo()
    assert res["1"]["loss"] == res["1"]["loss"] and abs(res["1"]["loss"]) < float("inf")
    assert abs(res["1"]["loss"] - res["0"]["loss"]) <= RG.REL_TOL * abs(res["0"]["loss"])
    assert abs(res["1"]["psnr"] - res["0"]["psnr"]) <= RG.REL_TOL * abs(res["0"]["psnr"])


def _report(path):
    """Markdown of a run's records (FG_PARITY_REPORT): per case and group, per label, the HIP ratio and (E32)."""
    import loss_restatement as L

    ratio, e32 = P.read_records(path, "test_target_loss_gpu")
    worst = max(ratio, key=ratio.get)
    print(f"Target loss: worst ratio {ratio[worst]:.2f} at {' | '.join(worst)}; {len(ratio)} cells.\n")
    cols = list(L.REGIMES) + list(T.ALPHA_CLASSES) + list(T.MASK_CLASSES) + list(T.VALUES)
    print("| case | group | " + " | ".join(cols) + " |\n|---|---|" + "---|" * len(cols))
    for tag, what in dict.fromkeys(k[:2] for k in ratio):
        cells = [f"{ratio[(tag, what, c)]:.2f} ({e32[(tag, what, c)]:.1e})" if (tag, what, c) in ratio else "" for c in cols]
        print(f"| {tag} | {what} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    _report(sys.argv[1])
