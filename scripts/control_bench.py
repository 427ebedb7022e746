"""Measure the fused stage-2 control stage (``FG_FUSED_CONTROL=1``: ``ops.control_*``, csrc/control.hip) against the torch ops of
the same build and write profiles/control_fused.md.

    python scripts/control_bench.py measure OUT_DIR      on an MI355X: OUT_DIR/control_fused.json
    python scripts/control_bench.py render OUT_DIR > profiles/control_fused.md      anywhere with hipcc (the resource table)
``render`` prints sections (a) .. (c) and the verdict of the default-on rule; the reading of the numbers in the committed file
was written by hand.

Protocol: the two sides alternate call by call in one process, 10 warm-up and 50 timed calls between device events, median
(p10 .. p90).  A gain = medians apart with p10 .. p90 not overlapping; default-on would need <= 0.8 x at every size.  The host
wall time per step is taken over 50 steps of one side with no synchronisation inside (the clock stops before the final
synchronise), three times per side, the sides taking turns.  Both cameras' times live on the device on both sides: a time on
the host is uploaded by a blocking copy on either path."""
import json
import os
import sys

import torch

from fused_bench_common import TIMED, WARM, alternate, cell, csrc, host_ms_per_step, kernel_resources, verdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STAGE_SIZES = ((240_000, 0.05), (240_000, 0.25), (1_000_000, 0.05))
KNOB = "FG_FUSED_CONTROL"
M = 3


def _mask(n, fraction, seed=0):
    """[n,3] bool: ``fraction`` of the rows selected, in three overlapping runs of rows as a segmented object gives them."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randperm(n, generator=g)[: int(n * fraction)]
    mask = torch.zeros(n, M, dtype=torch.bool)
    third = rows.numel() // 3
    mask[rows[: third + third // 4], 0] = True
    mask[rows[third : 2 * third + third // 4], 1] = True
    mask[rows[2 * third :], 2] = True
    return mask


def _model(n, fraction, W, H):
    from freegaussian_amd.model import Camera, FreeGaussianControlModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1
    f = 750.0 * W / 960
    init = Camera(c2w[None, :3], f, f, W / 2, H / 2, W, H, times=torch.tensor([[0.0]]))
    cm = FreeGaussianControlModel(_mask(n, fraction), init, config=FreeGaussianModelConfig(background_color="black", num_downscales=0),
                                  seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-4.5)  # fmt: skip
    with torch.no_grad():
        for q in cm.deform.parameters():
            q.mul_(0.3)
    cm = cm.cuda().train()
    cm.init_camera.times = cm.init_camera.times.cuda()
    cam = Camera(c2w[None, :3], f, f, W / 2, H / 2, W, H, times=torch.tensor([[0.4]]).cuda(), metadata={"cameras0": cm.init_camera})
    return cm, cam


def _set(knob):
    if knob:
        os.environ[KNOB] = "1"
    else:
        os.environ.pop(KNOB, None)


def _stage(n, fraction):
    """(a) the control stage alone, forward + backward, on a model of n Gaussians."""
    cm, cam = _model(n, fraction, 64, 64)
    ups = [torch.randn(n, w, device="cuda") for w in (3, 4, 3)]

    def run(knob):
        _set(knob)
        cm.zero_grad(set_to_none=True)
        torch.autograd.backward(cm._control_stage(cam), ups)

    sides = {"fused": lambda: run(True), "torch": lambda: run(False)}
    outs = {}
    for k, knob in (("fused", True), ("torch", False)):
        _set(knob)
        with torch.no_grad():
            outs[k] = cm._control_stage(cam)
    worst = max(float((a - b).abs().max()) for a, b in zip(outs["fused"], outs["torch"]))
    res = {"N": n, "fraction": fraction, "n": int(cm.gaussian_mask.any(-1).sum()), "max_abs_difference": worst,
           "fwd_bwd_ms": alternate(sides), "host_ms_per_call": host_ms_per_step(sides)}  # fmt: skip
    _set(False)
    return res


def _train_step():
    """(b) a stage-2 ``harness.train_step`` at 240 000 Gaussians, 960 x 540, 5 % of the rows masked."""
    from freegaussian_amd import harness

    n, W, H = 240_000, 960, 540
    cm, cam = _model(n, 0.05, W, H)
    opts = harness.build_optimizers(cm)
    gt = torch.rand(H, W, 3, device="cuda")
    state = {"step": 30_000}

    def step(knob):
        _set(knob)
        state["step"] += 1
        harness.train_step(cm, opts, cam, gt, state["step"], metrics_every=10**9)

    sides = {"unset": lambda: step(False), "1": lambda: step(True)}
    res = {"N": n, "n": int(cm.gaussian_mask.any(-1).sum()), "width": W, "height": H, "optimizers": sorted(opts),
           "gpu_ms": alternate(sides), "host_ms_per_step": host_ms_per_step(sides)}  # fmt: skip
    _set(False)
    return res


def measure(out):
    os.makedirs(out, exist_ok=True)
    os.environ["FG_FUSED_MLP_TRAIN"], os.environ["FG_FUSED_MLP_WGRAD"] = "1", "1"
    res = {"device": torch.cuda.get_device_name(0), "stage": [], "mlp_knobs": "FG_FUSED_MLP_TRAIN=1 FG_FUSED_MLP_WGRAD=1"}
    for n, fraction in STAGE_SIZES:
        res["stage"].append(_stage(n, fraction))
        json.dump(res, open(os.path.join(out, "control_fused.json"), "w"), indent=1)
        print(json.dumps(res["stage"][-1]), flush=True)
    res["train_step"] = _train_step()
    json.dump(res, open(os.path.join(out, "control_fused.json"), "w"), indent=1)
    print(json.dumps(res["train_step"]), flush=True)


def render(out):
    r = json.load(open(os.path.join(out, "control_fused.json")))
    print("# Fused stage-2 control stage (`FG_FUSED_CONTROL=1`): what it costs and saves\n")
    print(f"Measured on one {r['device']} by `scripts/control_bench.py`; nothing about this stage had been measured before this run.  "
          f"Protocol: the two sides alternate call by call in one process, {WARM} warm-up and {TIMED} timed calls between device "
          "events, median (p10 .. p90) in ms; the baseline is the torch ops of the same build (the knob unset).  A gain = medians "
          "apart with p10 .. p90 not overlapping; default-on would need <= 0.8 x at every size.  Host wall time: per call, over "
          f"{TIMED} calls of one side in a row with no synchronisation inside, three rounds per side.  Both sides run under "
          f"`{r['mlp_knobs']}`, with M = {M} attributes and both cameras' times on the device.\n")
    print("## (a) The control stage alone, forward + backward (`_control_stage`: mask rows to the three full-N arrays)\n")
    print("| N | masked rows n | fused ms | torch ops ms | outcome | host ms per call, fused | host ms per call, torch ops | max abs difference of the outputs |")
    print("|---|---|---|---|---|---|---|---|")
    ratios = []
    for s in r["stage"]:
        f, t = s["fwd_bwd_ms"]["fused"], s["fwd_bwd_ms"]["torch"]
        ratios.append(f["median"] / t["median"])
        hf, ht = (", ".join(f"{v:.3f}" for v in s["host_ms_per_call"][k]) for k in ("fused", "torch"))
        print(f"| {s['N']:,} | {s['n']:,} ({100 * s['fraction']:.0f} %) | {cell(f)} | {cell(t)} | {verdict(f, t)} | {hf} | {ht} | {s['max_abs_difference']:.2e} |")
    t = r["train_step"]
    print(f"\n## (b) One stage-2 `harness.train_step` at {t['N']:,} Gaussians, {t['width']} x {t['height']}, {t['n']:,} masked rows\n")
    print("| | knob unset | `FG_FUSED_CONTROL=1` | outcome |\n|---|---|---|---|")
    print(f"| GPU ms per step, between events | {cell(t['gpu_ms']['unset'])} | {cell(t['gpu_ms']['1'])} | {verdict(t['gpu_ms']['1'], t['gpu_ms']['unset'])} |")
    hu, h1 = (", ".join(f"{v:.3f}" for v in t["host_ms_per_step"][k]) for k in ("unset", "1"))
    print(f"| host wall ms per step, no synchronisation inside (three rounds) | {hu} | {h1} | |")
    print("\n## (c) Resource usage (`-Rpass-analysis=kernel-resource-usage`, gfx950)\n")
    print("| kernel | SGPRs | VGPRs | scratch bytes / lane | occupancy, waves / SIMD | LDS bytes / workgroup |\n|---|---|---|---|---|---|")
    for k in kernel_resources(csrc("control.hip")):
        print(f"| `{k['kernel']}` | {k['TotalSGPRs']} | {k['VGPRs']} | {k['ScratchSize']} | {k['Occupancy']} | {k['LDS']} |")
    met = all(x <= 0.8 for x in ratios)
    print(f"\n## The default-on rule\n\nFused over torch ops, medians of (a): {', '.join(f'{x:.2f}' for x in ratios)}.  The rule (<= 0.8 x at every "
          f"size) is {'met' if met else 'NOT met'}.  The knob stays opt-in.")


if __name__ == "__main__":
    {"measure": measure, "render": render}[sys.argv[1]](sys.argv[2])
