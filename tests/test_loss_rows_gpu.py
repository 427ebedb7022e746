"""The image loss (csrc/loss.hip) in isolation: ``ops.l1_ssim`` -- fg_l1_ssim_fwd, fg_l1_ssim_bwd -- on the regime images of
tests/loss_restatement.py, every gradient element, every map pixel and both values compared with the float64 restatement,
one cotangent group at a time.

Shapes (the tile is 32 x 16 pixels):
    58 x 106   4 x 4 workgroups; the map (48 x 96) is exactly 3 x 3 tiles: the last tile row and column hold image pixels
               but no map pixel.  One, three and four channels.
    53 x 75    partial tiles on both axes, for the image and for the map
    11 x 11    one map pixel
    12 x 43    the map is 2 x 33: it crosses one tile column

PER ELEMENT, groups "ssim" and "both":  |g_hip - g64| / A64  <=  F * E32(regime, group), no element left out.
GROUP "l1" (the SSIM value unused: its cotangent arrives as None): every element is, bit for bit, the fp32 product
    float32(v) * float32(1 / (HWC)) * sign(pred - gt).
THE THREE MAPS (fg_l1_ssim_fwd called directly): per map pixel, each against its own accumulation, F * E32(regime, map).
THE TWO VALUES: within F x the fp32 restatement's own (floored) distance from float64; bit-identical on repetition.
tests/parity_common.py has the protocol (A, E32, the floor, F); F and FLOOR are loss_restatement's, the recorded table is in
profiles/loss_adam_flow_parity.md.

``PYTHONPATH=. python tests/test_loss_rows_gpu.py REPORT.jsonl`` turns the records of a run under FG_PARITY_REPORT into the table of
profiles/loss_adam_flow_parity.md.
"""
import functools
import sys

import pytest
import torch

import loss_restatement as L
import parity_common as P
from freegaussian_amd import _lib, ops
from parity_common import need_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (H, W, C, first regime of the image)
CASES = [(58, 106, 1, 0), (58, 106, 3, 0), (58, 106, 4, 0), (53, 75, 3, 1), (11, 11, 3, 0), (12, 43, 3, 5)]


@functools.lru_cache(maxsize=None)
def _reference(H, W, C, first):
    """pred, gt, regime, the float64 forward and gradients, E32 per group / map / value; computed once per case."""
    pred, gt, regime = L.regime_image(H, W, first)
    pred, gt = pred[..., :C].contiguous(), gt[..., :C].contiguous()
    f32, r32 = L.gradients(pred, gt, torch.float32)
    f64, r64 = L.gradients(pred, gt, torch.float64)
    masks, map_masks = P.masks_of_index(regime, L.REGIMES), P.masks_of_index(L.map_regime(regime), L.REGIMES)
    e32 = {g: P.yardstick(masks, P.distance(r32[g][0], *r64[g]), L.FLOOR) for g in L.GROUPS}
    e32_maps = {k: P.yardstick(map_masks, P.distance(f32["maps"][k], f64["maps"][k], f64["acc"][k]), L.FLOOR) for k in L.MAPS}
    e32_val = {k: max(float(P.distance(f32[k], f64[k], f64[k + "_acc"])), L.FLOOR) for k in ("l1", "ssim")}
    return pred, gt, masks, map_masks, f64, r64, e32, e32_maps, e32_val


def _run_hip(pred, gt, group):
    x = pred.to(DEV).requires_grad_(True)
    l1, ss = ops.l1_ssim(x, gt.to(DEV))
    v_l1, v_ssim = L.COTANGENTS[group]
    # a group's loss leaves the other output unused: autograd hands its cotangent over as None
    loss = v_l1 * l1 if group == "l1" else (v_ssim * ss if group == "ssim" else v_l1 * l1 + v_ssim * ss)
    loss.backward()
    torch.cuda.synchronize()
    return l1.detach().cpu(), ss.detach().cpu(), x.grad.cpu()


@pytest.mark.parametrize("H,W,C,first", CASES)
def test_every_element(H, W, C, first):
    pred, gt, masks, _, f64, r64, e32, _, e32_val = _reference(H, W, C, first)
    tag = f"{H}x{W}x{C}"
    failures = []
    values = []
    for group in L.GROUPS:
        l1, ss, g = _run_hip(pred, gt, group)
        values.append((l1, ss))
        assert g.shape == pred.shape
        if group == "l1":
            v = torch.tensor(L.COTANGENTS["l1"][0], dtype=torch.float32) * torch.tensor(1.0 / (float(H) * W * C)).float()
            want = v * torch.sign(pred - gt)
            same = g == want  # (NaN is not equal; a zero of either sign is a zero)
            if not bool(same.all()):
                bad = (~same).nonzero()
                failures.append(f"{tag} l1: {len(bad)} elements are not float32(v) * float32(1 / HWC) * sign, first {bad[0].tolist()}: "
                                f"{float(g[tuple(bad[0])])!r} for {float(want[tuple(bad[0])])!r}")  # fmt: skip
            continue
        P.check(f"{tag}|{group}|{{regime}}", masks, P.distance(g, *r64[group]), e32[group], L.F, failures)
    for l1, ss in values[1:]:
        assert torch.equal(l1, values[0][0]) and torch.equal(ss, values[0][1]), "the two values differ between two calls"
    for k, s in zip(("l1", "ssim"), values[0]):
        ratio = float(P.distance(s, f64[k], f64[k + "_acc"])) / e32_val[k]
        P.check_cell(f"{tag}|value|{k}", ratio, e32_val[k], L.F, failures, f"{float(s)!r} for {float(f64[k])!r}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("H,W,C,first", CASES)
def test_every_map_pixel(H, W, C, first):
    """fg_l1_ssim_fwd through ``_lib`` directly: the three saved maps D_mu (total), D_xx, D_xy."""
    pred, gt, _, map_masks, f64, _, _, e32_maps, _ = _reference(H, W, C, first)
    lib = _lib.load()
    x, y = pred.to(DEV), gt.to(DEV)
    n_ws = int(lib.fg_l1_ssim_workspace_floats(H, W, C))
    nb = ((W + 31) // 32) * ((H + 15) // 16) * C
    assert n_ws == 2 * nb
    maps = torch.full((3, C, H - 10, W - 10), float("nan"), device=DEV)
    ws, out = torch.empty(n_ws, device=DEV), torch.empty(2, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.fg_l1_ssim_fwd(H, W, C, x.data_ptr(), y.data_ptr(), maps.data_ptr(), ws.data_ptr(), n_ws, out.data_ptr(), stream),
               "fg_l1_ssim_fwd")  # fmt: skip
    torch.cuda.synchronize()
    maps = maps.cpu()
    l1, ss = ops.l1_ssim(x, y)
    assert torch.equal(out.cpu(), torch.stack([l1, ss]).cpu())
    failures = []
    for i, k in enumerate(L.MAPS):
        d = P.distance(maps[i], f64["maps"][k], f64["acc"][k])
        P.check(f"{H}x{W}x{C}|map {k}|{{regime}}", map_masks, d, e32_maps[k], L.F, failures)
    assert not failures, "\n".join(failures)


def test_wrapper_inputs():
    """A ``pred`` that is a non-contiguous view and a ``gt`` in float16 give what their contiguous fp32 copies give."""
    H, W, C, first = CASES[3]
    pred, gt, _ = L.regime_image(H, W, first)
    gt = gt[..., :C].half()  # (a float16 image: its fp32 copy is exact)
    wide = pred.to(DEV)  # [H,W,4]: the first three channels are a view with strides (4 W, 4, 1)
    view = wide[..., :C].detach().requires_grad_(True)
    assert not view.is_contiguous()
    copy = wide[..., :C].contiguous().detach().requires_grad_(True)
    res = []
    for x, y in ((view, gt.to(DEV)), (copy, gt.float().to(DEV))):
        l1, ss = ops.l1_ssim(x, y)
        (L.COTANGENTS["both"][0] * l1 + L.COTANGENTS["both"][1] * ss).backward()
        res.append((l1.detach(), ss.detach(), x.grad))
    assert res[0][2].shape == view.shape
    for a, b in zip(*res):
        assert torch.equal(a, b)


def _report(path):
    """Markdown of a run's records (FG_PARITY_REPORT): per case, (group / map / value) x regime, the HIP ratio and (E32)."""
    ratio, e32 = P.read_records(path, "test_loss_rows_gpu")
    worst = max(ratio, key=ratio.get)
    print(f"Loss: worst ratio {ratio[worst]:.2f} at {' | '.join(worst)}; {len(ratio)} cells.\n")
    cols = list(L.REGIMES) + ["l1", "ssim"]
    print("| case | group / map | " + " | ".join(cols) + " |\n|---|---|" + "---|" * len(cols))
    for tag, what in dict.fromkeys(k[:2] for k in ratio):
        cells = [f"{ratio[(tag, what, c)]:.2f} ({e32[(tag, what, c)]:.1e})" if (tag, what, c) in ratio else "" for c in cols]
        print(f"| {tag} | {what} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    _report(sys.argv[1])
