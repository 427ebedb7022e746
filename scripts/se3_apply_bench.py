"""Measure the fused SE(3) transform of the means (``ops.se3_apply``, csrc/se3_apply.hip) against the torch ops of the same build
and write profiles/se3_apply_fused.md.

    python scripts/se3_apply_bench.py measure OUT_DIR      on an MI355X: OUT_DIR/se3_apply.json
    python scripts/se3_apply_bench.py render OUT_DIR > profiles/se3_apply_fused.md      anywhere with hipcc (the resource table)
``render`` prints sections (a) .. (e); (f) and the reading of the numbers in the committed file were written by hand.

Protocol: the two sides alternate call by call in one process, 10 warm-up and 50 timed calls between device events, median
(p10 .. p90).  A gain = medians apart with p10 .. p90 not overlapping; default-on would need <= 0.8 x at every size."""
import json
import os
import sys

import torch

from fused_bench_common import TIMED, WARM, alternate, cell, csrc, kernel_resources, verdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZES = (33_000, 240_000, 1_000_000)
KNOB = "FG_FUSED_SE3"
FWD_BYTES, BWD_BYTES = 36 + 12, 36 + 12 + 36  # per row: w, v, pts -> out;  w, v, pts, g_out -> g_w, g_v, g_pts


def _inputs(n):
    g = torch.Generator().manual_seed(n)
    w = torch.randn(n, 3, generator=g) * 0.2
    v = torch.randn(n, 3, generator=g) * 0.2
    x = torch.rand(n, 3, generator=g) * 2 - 1
    go = torch.randn(n, 3, generator=g)
    return [t.cuda() for t in (w, v, x, go)]


def _op(n):
    from freegaussian_amd import _lib, ops
    from freegaussian_amd.deform import FreeGaussianDeformableModel as D
    from freegaussian_amd.utils import transform_points

    w, v, x, go = _inputs(n)
    leaves = [t.requires_grad_(True) for t in (w, v, x)]

    def run(fn):
        for t in leaves:
            t.grad = None
        fn(*leaves).backward(go)

    sides = {"fused": lambda: run(ops.se3_apply), "torch": lambda: run(lambda w, v, x: transform_points(D._se3(w, v), x))}
    res = {"n": n, "fwd_bwd_ms": alternate(sides)}
    peak = {}
    for k, fn in sides.items():
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - before
    res["peak_bytes_above_inputs"] = peak
    # each kernel alone, through the C ABI, into buffers made once
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    out, gw, gv, gx = (torch.empty(n, 3, device="cuda") for _ in range(4))
    p = lambda t: t.data_ptr()  # noqa: E731
    wd, vd, xd = (t.detach() for t in leaves)
    kern = alternate({
        "fwd": lambda: lib.fg_se3_apply_fwd(n, p(wd), 3, p(vd), 3, p(xd), p(out), s),
        "bwd": lambda: lib.fg_se3_apply_bwd(n, p(wd), 3, p(vd), 3, p(xd), p(go), p(gw), 3, p(gv), 3, p(gx), s),
    })
    res["kernel_ms"] = kern
    res["kernel_GBps"] = {"fwd": n * FWD_BYTES / kern["fwd"]["median"] / 1e6, "bwd": n * BWD_BYTES / kern["bwd"]["median"] / 1e6}
    return res


def _model_step():
    from freegaussian_amd import ops
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    n, W, H = 240_000, 960, 540
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-4.5)
    with torch.no_grad():
        for q in model.deform.parameters():
            q.mul_(0.3)
    model.step = 4000
    model = model.cuda().train()
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1
    cam = Camera(c2w[None, :3], 750.0, 750.0, W / 2, H / 2, W, H, times=torch.tensor([[0.4]]))
    gt = torch.rand(H, W, 3, device="cuda")
    calls, real = [], ops.se3_apply
    ops.se3_apply = lambda *a: calls.append(1) or real(*a)

    def step(knob):
        if knob:
            os.environ[KNOB] = "1"
        else:
            os.environ.pop(KNOB, None)
        model.zero_grad(set_to_none=True)
        model.get_loss_dict(model.get_outputs(cam), {"image": gt})["main_loss"].backward()

    res = {"n": n, "width": W, "height": H, "settings": {}}
    os.environ["FG_FUSED_MLP_TRAIN"], os.environ["FG_FUSED_MLP_WGRAD"] = "1", "1"
    for precision in ("fp32", "bf16x3"):
        os.environ["FG_FUSED_MLP_PRECISION"] = os.environ["FG_FUSED_MLP_WGRAD_PRECISION"] = precision
        del calls[:]
        res["settings"][precision] = alternate({"unset": lambda: step(False), "1": lambda: step(True)}, warm=5, timed=30)
        assert len(calls) == 35, len(calls)
    os.environ.pop(KNOB, None)
    ops.se3_apply = real
    return res


def measure(out):
    os.makedirs(out, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "op": [_op(n) for n in SIZES], "model": _model_step()}
    json.dump(res, open(os.path.join(out, "se3_apply.json"), "w"), indent=1)
    print(json.dumps(res), flush=True)


def render(out):
    r = json.load(open(os.path.join(out, "se3_apply.json")))
    print("# Fused SE(3) transform of the means (`FG_FUSED_SE3=1`): what it costs and saves\n")
    print(f"Measured on one {r['device']} by `scripts/se3_apply_bench.py`; nothing about this op had been measured before this run "
          "(the 130 B per row and \"most of the glue\" that motivated it were estimates).  Protocol: the two sides alternate call by call in one "
          f"process, {WARM} warm-up and {TIMED} timed calls between device events, median (p10 .. p90) in ms; the baseline is the "
          "torch ops of the same build (`deform._se3` + `utils.exp_se3` + `utils.transform_points`).  A gain = medians apart with "
          "p10 .. p90 not overlapping; default-on would need <= 0.8 x at every size.  The knob stays opt-in either way.\n")
    print("## (a) The op alone, forward + backward to all three gradients\n")
    print("| rows | fused ms | torch ops ms | outcome |\n|---|---|---|---|")
    for o in r["op"]:
        f, t = o["fwd_bwd_ms"]["fused"], o["fwd_bwd_ms"]["torch"]
        print(f"| {o['n']:,} | {cell(f)} | {cell(t)} | {verdict(f, t)} |")
    print("\n## (b) One model training step at 240 000 Gaussians, 960 x 540, behind `warm_up`\n")
    print("`FG_FUSED_MLP_TRAIN=1` and `FG_FUSED_MLP_WGRAD=1` as in `profiles/mlp_wgrad_split.md` (c); the column is "
          "`FG_FUSED_MLP_PRECISION` = `FG_FUSED_MLP_WGRAD_PRECISION`.\n")
    print("| MLP precision | knob unset ms | `FG_FUSED_SE3=1` ms | outcome |\n|---|---|---|---|")
    for k, v in r["model"]["settings"].items():
        print(f"| {k} | {cell(v['unset'])} | {cell(v['1'])} | {verdict(v['1'], v['unset'])} |")
    print("\n## (c) Peak allocated memory of one forward + backward of (a), above the inputs\n")
    print("| rows | fused MB | torch ops MB | bytes per row, fused | bytes per row, torch ops |\n|---|---|---|---|---|")
    for o in r["op"]:
        p = o["peak_bytes_above_inputs"]
        print(f"| {o['n']:,} | {p['fused'] / 1e6:.1f} | {p['torch'] / 1e6:.1f} | {p['fused'] / o['n']:.0f} | {p['torch'] / o['n']:.0f} |")
    print("\n## (d) Each kernel alone, through the C ABI, from its algorithmic bytes\n")
    print(f"Forward {FWD_BYTES} B per row (w, v, pts read; out written), backward {BWD_BYTES} B per row (w, v, pts, g_out read; three "
          "gradients written).\n")
    print("| rows | forward ms | forward GB/s | backward ms | backward GB/s |\n|---|---|---|---|---|")
    for o in r["op"]:
        k, g = o["kernel_ms"], o["kernel_GBps"]
        print(f"| {o['n']:,} | {cell(k['fwd'])} | {g['fwd']:.0f} | {cell(k['bwd'])} | {g['bwd']:.0f} |")
    print("\n## (e) Resource usage (`-Rpass-analysis=kernel-resource-usage`, gfx950)\n")
    print("`se3_bwd_kernel<w, v, pts>`: one kernel per set of gradients asked for.\n")
    print("| kernel | SGPRs | VGPRs | scratch bytes / lane | occupancy, waves / SIMD | LDS bytes / workgroup |\n|---|---|---|---|---|---|")
    for k in kernel_resources(csrc("se3_apply.hip")):
        print(f"| `{k['kernel']}` | {k['TotalSGPRs']} | {k['VGPRs']} | {k['ScratchSize']} | {k['Occupancy']} | {k['LDS']} |")


if __name__ == "__main__":
    {"measure": measure, "render": render}[sys.argv[1]](sys.argv[2])
