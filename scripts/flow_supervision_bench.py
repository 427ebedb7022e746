"""Measure the flow supervision (``ops.flow_displacement``, csrc/flow_disp.hip; ``ops.flow_l1``, csrc/flow_loss.hip; the model's
flow branch) and write profiles/flow_supervision.md.  This is not bench.py: it states what the capability costs.

    python scripts/flow_supervision_bench.py measure OUT_DIR      on an MI355X: OUT_DIR/flow_supervision.json
    python scripts/flow_supervision_bench.py render OUT_DIR > profiles/flow_supervision.md      anywhere with hipcc

Protocol (scripts/fused_bench_common.py): the two sides alternate call by call in one process, warm-up then timed calls between
device events, median (p10 .. p90) in ms.  A gain = medians apart with p10 .. p90 not overlapping.  No ratio is promised."""
import json
import os
import sys

import torch

from fused_bench_common import TIMED, WARM, alternate, cell, csrc, kernel_resources, verdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROWS = (33_000, 240_000, 1_000_000)
IMAGES = ((480, 270), (960, 540), (1920, 1080))  # (W0, H0) of the batch array
DOWNSCALES = (1, 2)


def _cams(W, H):
    from freegaussian_amd.scenes import look_at_viewmat

    Vt = look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3))
    V0 = look_at_viewmat(torch.tensor([0.27, -0.17, -3.02]), torch.zeros(3))
    K = torch.tensor([[0.78 * W, 0.0, W / 2], [0.0, 0.78 * W, H / 2], [0.0, 0.0, 1.0]])
    return Vt.float().cuda(), V0.float().cuda(), K.cuda()


def _displacement(n, W=960, H=540):
    """fwd + bwd to both sets of means: the fused op against the two-``ops.project`` composition of ``flow.render_with_flow``."""
    from freegaussian_amd import _lib, ops

    g = torch.Generator().manual_seed(n)
    m0 = ((torch.rand(n, 3, generator=g) - 0.5) * 2.0).cuda()
    mt = (m0 + torch.randn(n, 3, generator=g).cuda() * 0.01).requires_grad_(True)
    m0.requires_grad_(True)
    quats = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1).cuda()
    scales = torch.full((n, 3), 0.01).cuda()
    go = torch.randn(n, 2, generator=g).cuda()
    Vt, V0, K = _cams(W, H)

    def fused():
        mt.grad = m0.grad = None
        ops.flow_displacement(mt, m0, Vt, V0, K, W, H, margin=float(max(W, H))).backward(go)

    def composition():
        mt.grad = m0.grad = None
        r0, mu0, _, _, _, _ = ops.project(m0, quats, scales, V0, K, W, H)
        rt, mut, _, _, _, _ = ops.project(mt, quats, scales, Vt, K, W, H)
        both = ((r0 > 0) & (rt > 0)).unsqueeze(-1)
        torch.where(both, mut - mu0, torch.zeros_like(mut)).backward(go)

    res = {"n": n, "fwd_bwd_ms": alternate({"fused": fused, "composition": composition})}
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    disp, gt, g0 = torch.empty(n, 2, device="cuda"), torch.empty(n, 3, device="cuda"), torch.empty(n, 3, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    a, b = mt.detach(), m0.detach()
    inf = float("inf")
    kern = alternate({
        "fwd": lambda: lib.fg_flow_disp_fwd(n, p(a), 3, p(b), 3, p(Vt), p(V0), p(K), W, H, 0.01, inf, p(disp), s),
        "bwd": lambda: lib.fg_flow_disp_bwd(n, p(a), 3, p(b), 3, p(Vt), p(V0), p(K), W, H, 0.01, inf, p(go), p(gt), p(g0), s),
    })  # fmt: skip
    res["kernel_ms"] = kern
    res["kernel_GBps"] = {"fwd": n * 32 / kern["fwd"]["median"] / 1e6, "bwd": n * 56 / kern["bwd"]["median"] / 1e6}
    return res


def _torch_flow_l1(pred, flows, mask, d):
    """The torch statement of ``ops.flow_l1``: resize, / d, the mask resized the same way, non-finite blocks out, weighted mean."""
    from freegaussian_amd.utils import resize_image

    finite = torch.isfinite(flows).all(-1, keepdim=True)
    clean = torch.where(finite, flows, torch.zeros_like(flows))
    target = (resize_image(clean, d) if d > 1 else clean) / d
    w = (resize_image(finite.float(), d) if d > 1 else finite.float()) == 1
    m = resize_image(mask.float(), d) if d > 1 else mask.float()
    w = torch.where(w, m, torch.zeros_like(m))
    return (w * (pred - target).abs()).sum() / (2 * w.sum().clamp(min=1e-30))


def _loss(W0, H0, d):
    """fwd + bwd: ``pred`` the last two channels of a [1,H,W,5] render, a bool mask, a few NaN source pixels."""
    from freegaussian_amd import ops

    g = torch.Generator().manual_seed(W0 + d)
    H, W = H0 // d, W0 // d
    render = torch.randn(1, H, W, 5, generator=g).cuda().requires_grad_(True)
    flows = torch.randn(H0, W0, 2, generator=g) * 3
    flows[torch.rand(H0, W0, generator=g) < 0.01] = float("nan")
    flows = flows.cuda()
    mask = (torch.rand(H0, W0, 1, generator=g) < 0.9).cuda()

    def run(fn):
        render.grad = None
        fn(render[0, :, :, 3:], flows, mask, d).backward()

    return {"W0": W0, "H0": H0, "d": d, "fwd_bwd_ms": alternate({"fused": lambda: run(ops.flow_l1), "torch": lambda: run(_torch_flow_l1)})}


def _model_step():
    """One get_outputs + get_loss_dict + backward at 240 000 Gaussians, 960 x 540, behind ``warm_up``: weight 0 against weight
    > 0 with ``flow_frame0_grad`` on and off -- the cost of the feature."""
    import copy

    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    n, W, H = 240_000, 960, 540
    models = {}
    base = None
    for name, cfg in (("weight 0", {}), ("weight 0.1", {"flow_loss_weight": 0.1}),
                      ("weight 0.1, flow_frame0_grad=False", {"flow_loss_weight": 0.1, "flow_frame0_grad": False})):  # fmt: skip
        config = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000, **cfg)
        if base is None:
            base = FreeGaussianModel(config, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-4.5)
            with torch.no_grad():
                for q in base.deform.parameters():
                    q.mul_(0.3)
        m = copy.deepcopy(base)
        m.config = config
        m.step = 4000
        models[name] = m.cuda().train()

    def cam(eye, t):
        c2w = torch.linalg.inv(look_at_viewmat(torch.tensor(eye), torch.zeros(3)))
        c2w[:3, 1:3] *= -1
        return Camera(c2w[None, :3], 750.0, 750.0, W / 2, H / 2, W, H, times=torch.tensor([[t]]))

    camera = cam([0.3, -0.2, -3.0], 0.4)
    camera.metadata["cameras0"] = cam([0.27, -0.17, -3.02], 0.35)
    batch = {"image": torch.rand(H, W, 3, device="cuda"), "flows": torch.randn(H, W, 2, device="cuda")}

    def step(model):
        model.zero_grad(set_to_none=True)
        losses = model.get_loss_dict(model.get_outputs(camera), batch)
        sum(losses.values()).backward()
        return losses

    assert "flow_loss" not in step(models["weight 0"]) and "flow_loss" in step(models["weight 0.1"])
    res = {"n": n, "width": W, "height": H, "ms": alternate({k: (lambda m=m: step(m)) for k, m in models.items()}, warm=5, timed=30)}
    peak = {}
    for k, m in models.items():
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step(m)
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - before
    res["peak_bytes_above_resident"] = peak
    return res


def measure(out):
    os.makedirs(out, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "displacement": [_displacement(n) for n in ROWS],
           "loss": [_loss(W0, H0, d) for W0, H0 in IMAGES for d in DOWNSCALES], "model": _model_step()}  # fmt: skip
    json.dump(res, open(os.path.join(out, "flow_supervision.json"), "w"), indent=1)
    print(json.dumps(res), flush=True)


def render(out):
    r = json.load(open(os.path.join(out, "flow_supervision.json")))
    print("# Flow-supervised training: what the two fused ops and the model's flow branch cost\n")
    print(f"Measured on one {r['device']} by `scripts/flow_supervision_bench.py`; nothing about these ops had been measured before "
          f"this run.  Protocol: the sides alternate call by call in one process, {WARM} warm-up and {TIMED} timed calls between device "
          "events (the model step: 5 and 30), median (p10 .. p90) in ms.  A gain = medians apart with p10 .. p90 not overlapping.  "
          "This is a capability: its cost is stated, no ratio was promised.\n")
    print("## (a) `ops.flow_displacement`, forward + backward to both sets of means, two cameras\n")
    print("The baseline is the composition of the same build that `flow.render_with_flow` uses: two `ops.project` passes, the "
          "`where`, two `_Project` backwards.\n")
    print("| rows | fused ms | two-`ops.project` composition ms | outcome |\n|---|---|---|---|")
    for o in r["displacement"]:
        f, t = o["fwd_bwd_ms"]["fused"], o["fwd_bwd_ms"]["composition"]
        print(f"| {o['n']:,} | {cell(f)} | {cell(t)} | {verdict(f, t)} |")
    print("\nEach kernel alone, through the C ABI, from its algorithmic bytes (forward 24 B read + 8 B written per row, backward "
          "32 B read + 24 B written):\n")
    print("| rows | forward ms | forward GB/s | backward ms | backward GB/s |\n|---|---|---|---|---|")
    for o in r["displacement"]:
        k, g = o["kernel_ms"], o["kernel_GBps"]
        print(f"| {o['n']:,} | {cell(k['fwd'])} | {g['fwd']:.0f} | {cell(k['bwd'])} | {g['bwd']:.0f} |")
    print("\n## (b) `ops.flow_l1`, forward + backward, `pred` read in place from a 5-channel render, bool mask, 1 % NaN source pixels\n")
    print("The baseline is the torch statement (`resize_image`, the mask resized the same way, `where`, `abs`, weighted mean).\n")
    print("| batch array | d | fused ms | torch statement ms | outcome |\n|---|---|---|---|---|")
    for o in r["loss"]:
        f, t = o["fwd_bwd_ms"]["fused"], o["fwd_bwd_ms"]["torch"]
        print(f"| {o['W0']} x {o['H0']} | {o['d']} | {cell(f)} | {cell(t)} | {verdict(f, t)} |")
    m = r["model"]
    print(f"\n## (c) One model training step at {m['n']:,} Gaussians, {m['width']} x {m['height']}, behind `warm_up`\n")
    print("`get_outputs` + `get_loss_dict` + backward of the summed losses; the camera carries a `cameras0` in every column, the "
          "batch a `flows` array.  Weight 0 is the parent's step.\n")
    print("| config | ms | against weight 0 | peak bytes above the resident set, MB |\n|---|---|---|---|")
    base = m["ms"]["weight 0"]
    for k, v in m["ms"].items():
        rel = "-" if k == "weight 0" else f"{v['median'] / base['median']:.2f} x ({verdict(v, base)})"
        print(f"| {k} | {cell(v)} | {rel} | {m['peak_bytes_above_resident'][k] / 1e6:.0f} |")
    print("\n## (d) Resource usage (`-Rpass-analysis=kernel-resource-usage`, gfx950)\n")
    print("| kernel | SGPRs | VGPRs | scratch bytes / lane | occupancy, waves / SIMD | LDS bytes / workgroup |\n|---|---|---|---|---|---|")
    for unit in ("flow_disp.hip", "flow_loss.hip"):
        for k in kernel_resources(csrc(unit)):
            print(f"| `{k['kernel']}` | {k['TotalSGPRs']} | {k['VGPRs']} | {k['ScratchSize']} | {k['Occupancy']} | {k['LDS']} |")


if __name__ == "__main__":
    {"measure": measure, "render": render}[sys.argv[1]](sys.argv[2])
