#!/usr/bin/env python3
"""Deformation-MLP forward without gradients: the fused kernel (``ops.mlp_forward`` through the module's dispatch)
against the torch forward of the same module (``FG_FUSED_MLP=0``), both under ``no_grad`` and both with the transformed
points included.  Writes profiles/mlp_forward.md.

    python scripts/mlp_forward_bench.py [--out DIR] [--md profiles/mlp_forward.md]

runs the steps below as child processes, each under its own ``timeout -k 10``, stopping at the first that fails (a
fault or a time limit in one step starts nothing more on the GPU):

    --step time    N = 33 000, 240 000, 1 000 000: the two paths ALTERNATE call by call in one process, 10 warm-up and
                   50 timed calls each between device events; median, p10, p90; FLOPs per row from the layer shapes
    --step error   both paths at N = 33 000 against a float64 run of the same module on the CPU (default init, one time
                   per row): the fused kernel's margin beside the torch fp32 path's own
    --step frame   ``get_outputs_for_camera`` per frame, knob on and off alternating, behind ``warm_up``: the Gaussians and
                   first camera of ``data/trained_scene_r06.npz`` when that file is there (as ``bench.py --layout
                   trained:auto``), else 240 000 random Gaussians at 1920 x 1080 -- the table says which
    --step trace   three fused calls at N = 240 000 for ``rocprofv3 --kernel-trace --stats`` (with --trace; a run of its own)
    --step report  profiles/mlp_forward.md from these

    python scripts/mlp_forward_bench.py --precision [--trace] [--out results/mlp_split]

compares the opt-in split-bf16 mode (``precision="bf16x3"`` / ``FG_FUSED_MLP_PRECISION``) with the fp32 path OF THE SAME BUILD,
same protocol (the two sides alternate call by call); ``scripts/mlp_train_bench.py --precision`` adds the training side and
writes profiles/mlp_split_bf16.md from both:

    --step ptime   ``ops.mlp_forward`` (``fg_mlp_fwd`` alone: points, rotations, scalings) at the three sizes
    --step pframe  ``get_outputs_for_camera`` per frame, ``FG_FUSED_MLP_PRECISION`` set and unset alternating
    --step ptrace  three calls of either precision at N = 240 000 for ``rocprofv3 --kernel-trace --stats`` (with --trace)
"""
import argparse
import copy
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SIZES = (33_000, 240_000, 1_000_000)
WARM, TIMED = 10, 50
PEAK_TF = 157.0  # fp32 matrix peak of an MI355X
DEFAULT_ON_RATIO = 0.8  # the fused path stays default-on above an N only if its median is at most this x the torch path's


def flops_per_row(m):
    """2 x in x out over every linear the forward runs per row (the time net of the blender variant runs on one row)."""
    layers = list(m.linear) + [m.branch_w, m.branch_v, m.gaussian_rotation, m.gaussian_scaling]
    return sum(2 * l.in_features * l.out_features for l in layers)


def _quantiles(ms):
    s = sorted(ms)
    q = lambda p: s[min(len(s) - 1, int(round(p * (len(s) - 1))))]  # noqa: E731
    return {"median": q(0.5), "p10": q(0.1), "p90": q(0.9)}


def _timed_pair(run_fused, run_torch, warm=WARM, timed=TIMED):
    """Alternate the two callables; -> (fused ms list, torch ms list) from device events."""
    out = {"fused": [], "torch": []}
    for i in range(warm + timed):
        for name, fn in (("fused", run_fused), ("torch", run_torch)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warm:
                out[name].append(a.elapsed_time(b))
    return out["fused"], out["torch"]


def _module():
    from freegaussian_amd.deform import FreeGaussianDeformableModel

    torch.manual_seed(0)
    return FreeGaussianDeformableModel()


def _knob(value):
    os.environ["FG_FUSED_MLP"] = value


def step_time(out):
    from freegaussian_amd import ops
    from freegaussian_amd.deform import fused_applies
    from freegaussian_amd.utils import transform_points

    m = _module().cuda()
    fl = flops_per_row(m)
    res = {"flops_per_row": fl, "row_tile": ops.MLP_ROW_TILE, "sizes": {}}
    calls = []
    real = ops.mlp_forward
    ops.mlp_forward = lambda *a, **k: calls.append(1) or real(*a, **k)
    for n in SIZES:
        x = (torch.rand(n, 3, generator=torch.Generator().manual_seed(n)) * 2 - 1).cuda()
        t = torch.full((1, 1), 0.4, device="cuda").expand(n, -1)

        def run_fused():
            _knob("1")
            with torch.no_grad():
                assert fused_applies(m, x, t)
                return m.deformed_points(x, t)

        def run_torch():
            _knob("0")
            with torch.no_grad():
                T, rot, scale = m(x, t)
                return transform_points(T, x), rot, scale

        before = len(calls)
        f, p = _timed_pair(run_fused, run_torch)
        assert len(calls) - before == WARM + TIMED  # the fused path ran the kernel, the torch path never did
        qf, qp = _quantiles(f), _quantiles(p)
        res["sizes"][str(n)] = {"fused_ms": qf, "torch_ms": qp, "ratio": qf["median"] / qp["median"],
                                "fused_tflops": fl * n / qf["median"] / 1e9, "torch_tflops": fl * n / qp["median"] / 1e9}  # fmt: skip
        print(n, res["sizes"][str(n)], flush=True)
    json.dump(res, open(os.path.join(out, "time.json"), "w"), indent=1)


def step_error(out):
    from freegaussian_amd.utils import transform_points

    n = 33_000
    m = _module()
    g = torch.Generator().manual_seed(1)
    x, t = torch.rand(n, 3, generator=g) * 2 - 1, torch.rand(n, 1, generator=g)
    with torch.no_grad():
        m64 = copy.deepcopy(m).double()
        want = m64(x.double(), t.double())
        want = (*want, transform_points(want[0], x.double()))
        md, xd, td = m.cuda(), x.cuda(), t.cuda()
        _knob("1")
        T, rot, scale = md(xd, td)
        fused = (T, rot, scale, md.deformed_points(xd, td)[0])
        _knob("0")
        T, rot, scale = md(xd, td)
        plain = (T, rot, scale, transform_points(T, xd))

    def rel(a, b):
        return float((a.double().cpu() - b).abs().max() / b.abs().max())

    names = ("d_xyz", "d_rot", "d_scale", "pts")
    res = {k: {"fused": rel(f, w), "torch_fp32": rel(p, w)} for k, f, p, w in zip(names, fused, plain, want)}
    print(res, flush=True)
    json.dump(res, open(os.path.join(out, "error.json"), "w"), indent=1)


def _precision_knob(value):
    if value == "fp32":
        os.environ.pop("FG_FUSED_MLP_PRECISION", None)
    else:
        os.environ["FG_FUSED_MLP_PRECISION"] = value


def _forward_pair(m, n):
    """(run(precision), flops per row) of ``ops.mlp_forward`` over n rows into buffers made once: one time for all rows."""
    from freegaussian_amd import ops
    from freegaussian_amd.utils import positional_encoding

    x = (torch.rand(n, 3, generator=torch.Generator().manual_seed(n)) * 2 - 1).cuda()
    aux = positional_encoding(torch.full((1, 1), 0.4, device="cuda"), m.t_multires)
    heads = (m.branch_w, m.branch_v, m.gaussian_rotation, m.gaussian_scaling)
    outs = [False] + [torch.empty(n, c, device="cuda") for c in (4, 3, 3)]

    def run(precision):
        def go():
            return ops.mlp_forward(x, aux, m.linear, heads, mode="se3", outs=outs, precision=precision)
        return go

    return run


def pstep_time(out):
    m = _module().cuda().requires_grad_(False)
    fl = flops_per_row(m)
    res = {"flops_per_row": fl, "sizes": {}}
    for n in SIZES:
        run = _forward_pair(m, n)
        s, f = _timed_pair(run("bf16x3"), run("fp32"))
        qs, qf = _quantiles(s), _quantiles(f)
        res["sizes"][str(n)] = {"split_ms": qs, "fp32_ms": qf, "ratio": qs["median"] / qf["median"],
                                "split_tflops": fl * n / qs["median"] / 1e9, "fp32_tflops": fl * n / qf["median"] / 1e9}  # fmt: skip
        print(n, res["sizes"][str(n)], flush=True)
    json.dump(res, open(os.path.join(out, "ptime.json"), "w"), indent=1)


def pstep_trace(out):
    m = _module().cuda().requires_grad_(False)
    run = _forward_pair(m, 240_000)
    for precision in ("bf16x3", "fp32"):
        for _ in range(3):
            run(precision)()
    torch.cuda.synchronize()


TRAINED = os.path.join(ROOT, "data", "trained_scene_r06.npz")  # (what bench.py --layout trained:auto takes; not in the history)


def step_frame(out, precision=False):
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import load_trained_scene, look_at_viewmat

    torch.manual_seed(0)
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    if os.path.exists(TRAINED):
        # the trained scene's Gaussians and its first camera; its file holds the rasterizer's inputs (deformation applied),
        # not the net, so the net in front of them is a default-init one scaled down
        sc = load_trained_scene(TRAINED)
        n, W, H, source = sc.means.shape[0], sc.width, sc.height, "data/trained_scene_r06.npz"
        model = FreeGaussianModel(cfg, seed_points=sc.means, init_scales=0.0)
        with torch.no_grad():
            g = model.gauss_params
            g["scales"].copy_(sc.scales.clamp_min(1e-12).log())
            g["quats"].copy_(sc.quats)
            g["opacities"].copy_(torch.logit(sc.opacities.reshape(-1, 1).clamp(1e-6, 1 - 1e-6)))
            k = min(g["features_rest"].shape[1], sc.colors.shape[1] - 1)
            g["features_dc"].copy_(sc.colors[:, 0])
            g["features_rest"][:, :k].copy_(sc.colors[:, 1 : 1 + k])
        c2w = torch.linalg.inv(sc.viewmats[0])
        fx, fy, cx, cy = (float(sc.Ks[0][i, j]) for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
    else:
        n, W, H, source = 240_000, 1920, 1080, "240 000 random Gaussians (the trained scene's file is not here)"
        model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-4.5)
        c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
        fx, fy, cx, cy = 1500.0, 1500.0, W / 2, H / 2
    with torch.no_grad():
        for q in model.deform.parameters():
            q.mul_(0.3)
    model.step = 4000
    model = model.cuda().eval()
    c2w[:3, 1:3] *= -1  # OpenCV -> OpenGL camera axes (utils.get_viewmat flips them back)
    cam = Camera(c2w[None, :3], fx, fy, cx, cy, W, H, times=torch.tensor([[0.4]]))

    def frame(knob):
        def run():
            _knob(knob)
            return model.get_outputs_for_camera(cam)["rgb"]
        return run

    if precision:  # the fused forward on both sides, FG_FUSED_MLP_PRECISION set and unset
        _knob("1")

        def frame_at(value):
            def run():
                _precision_knob(value)
                return model.get_outputs_for_camera(cam)["rgb"]
            return run

        s, f = _timed_pair(frame_at("bf16x3"), frame_at("fp32"), warm=5, timed=30)
        res = {"n": n, "width": W, "height": H, "source": source, "split_ms": _quantiles(s), "fp32_ms": _quantiles(f)}
        print(res, flush=True)
        return json.dump(res, open(os.path.join(out, "pframe.json"), "w"), indent=1)
    f, p = _timed_pair(frame("1"), frame("0"), warm=5, timed=30)
    res = {"n": n, "width": W, "height": H, "source": source, "fused_ms": _quantiles(f), "torch_ms": _quantiles(p)}
    print(res, flush=True)
    json.dump(res, open(os.path.join(out, "frame.json"), "w"), indent=1)


def step_trace(out):
    m = _module().cuda()
    n = 240_000
    x = (torch.rand(n, 3) * 2 - 1).cuda()
    t = torch.full((1, 1), 0.4, device="cuda").expand(n, -1)
    _knob("1")
    with torch.no_grad():
        for _ in range(3):
            m.deformed_points(x, t)
    torch.cuda.synchronize()


def step_report(out, md):
    from freegaussian_amd.deform import FUSED_MIN_ROWS

    tm = json.load(open(os.path.join(out, "time.json")))
    L = ["# Fused fp32 MLP forward (`ops.mlp_forward`) against the torch forward", "",
         "Written by `scripts/mlp_forward_bench.py` on an MI355X.  Deformation net (D = 8, W = 256, multires 10, 21-wide time",
         f"encoding), `no_grad`, transformed points included; {tm['flops_per_row']} FLOP per row from the layer shapes; row tile",
         f"{tm['row_tile']}.  The two paths alternate call by call in one process, {WARM} warm-up and {TIMED} timed calls each between",
         f"device events.  Share of peak: of the {PEAK_TF:.0f} TFLOP/s fp32 matrix rate.", "",
         "| N | fused ms median (p10 .. p90) | torch ms median (p10 .. p90) | fused / torch | fused TFLOP/s | share of peak | torch TFLOP/s |",
         "|---|---|---|---|---|---|---|"]  # fmt: skip
    for n, r in tm["sizes"].items():
        f, p = r["fused_ms"], r["torch_ms"]
        L.append(f"| {int(n):,} | {f['median']:.3f} ({f['p10']:.3f} .. {f['p90']:.3f}) | {p['median']:.3f} ({p['p10']:.3f} .. {p['p90']:.3f}) | "
                 f"{r['ratio']:.2f} | {r['fused_tflops']:.1f} | {100 * r['fused_tflops'] / PEAK_TF:.0f} % | {r['torch_tflops']:.1f} |")  # fmt: skip
    ok = [int(n) for n, r in tm["sizes"].items() if r["ratio"] <= DEFAULT_ON_RATIO]
    L += ["", f"Default-on rule: fused median <= {DEFAULT_ON_RATIO} x torch median.  Sizes that meet it: "
          f"{', '.join(f'{n:,}' for n in ok) if ok else 'none'}.  Threshold in `deform.FUSED_MIN_ROWS`: {FUSED_MIN_ROWS:,} rows."]  # fmt: skip
    if os.path.exists(os.path.join(out, "error.json")):
        er = json.load(open(os.path.join(out, "error.json")))
        L += ["", "## Error against float64 (N = 33 000, default init, a time per row; max |a - b| / max |b|; the bar is 1e-4)", "",
              "| output | fused kernel | torch fp32 on the GPU |", "|---|---|---|"]  # fmt: skip
        L += [f"| {k} | {v['fused']:.2e} | {v['torch_fp32']:.2e} |" for k, v in er.items()]
    if os.path.exists(os.path.join(out, "frame.json")):
        fr = json.load(open(os.path.join(out, "frame.json")))
        f, p = fr["fused_ms"], fr["torch_ms"]
        L += ["", f"## `get_outputs_for_camera` per frame ({fr['source']}: {fr['n']:,} Gaussians behind `warm_up`, {fr['width']} x {fr['height']}, eval)", "",
              "| knob | ms per frame median (p10 .. p90) |", "|---|---|",
              f"| `FG_FUSED_MLP=0` (before) | {p['median']:.2f} ({p['p10']:.2f} .. {p['p90']:.2f}) |",
              f"| default (after) | {f['median']:.2f} ({f['p10']:.2f} .. {f['p90']:.2f}) |"]  # fmt: skip
    stats = sorted(glob.glob(os.path.join(out, "trace", "**", "*kernel_stats.csv"), recursive=True))
    if stats:
        L += ["", "## Kernels of three fused calls at N = 240 000 (`rocprofv3 --kernel-trace --stats`, a run of its own)", "",
              "| kernel | calls | average us | share % |", "|---|---|---|---|"]  # fmt: skip
        for r in list(csv.DictReader(open(stats[0])))[:8]:
            L.append(f"| `{r['Name'][:80]}` | {r['Calls']} | {float(r['AverageNs']) / 1e3:.1f} | {float(r['Percentage']):.1f} |")
    # (hand-written sections of the file -- everything from the first "## Notes" heading on -- are kept)
    if os.path.exists(md) and "\n## Notes" in open(md).read():
        L += ["", "## Notes" + open(md).read().split("\n## Notes", 1)[1].rstrip()]
    open(md, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["time", "error", "frame", "trace", "report", "ptime", "pframe", "ptrace"])
    ap.add_argument("--precision", action="store_true", help="the split-bf16 mode against fp32, the forward's share of profiles/mlp_split_bf16.md")
    ap.add_argument("--trace", action="store_true", help="also one rocprofv3 --kernel-trace --stats run of the fused calls")
    ap.add_argument("--out", default=None, help="default: results/mlp_forward, results/mlp_split with --precision")
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "mlp_forward.md"))
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "results", "mlp_split" if a.precision or (a.step or "").startswith("p") else "mlp_forward")
    os.makedirs(a.out, exist_ok=True)
    if a.step:
        if a.step == "report":
            return step_report(a.out, a.md)
        if a.step.startswith("p"):
            return {"ptime": pstep_time, "pframe": lambda out: step_frame(out, precision=True), "ptrace": pstep_trace}[a.step](a.out)
        return {"time": step_time, "error": step_error, "frame": step_frame, "trace": step_trace}[a.step](a.out)
    me = [sys.executable, os.path.abspath(__file__), "--out", a.out, "--md", a.md, "--step"]
    steps = [(240, me + ["time"]), (180, me + ["error"]), (240, me + ["frame"])]
    if a.trace:
        steps.append((180, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(a.out, "trace"),
                            "-o", "mlp", "--"] + me + ["trace"]))  # fmt: skip
    steps.append((60, me + ["report"]))
    if a.precision:
        steps = [(240, me + ["ptime"]), (240, me + ["pframe"])]
        if a.trace:
            steps.append((180, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(a.out, "ptrace_fwd"),
                                "-o", "mlp", "--"] + me + ["ptrace"]))  # fmt: skip
    for limit, cmd in steps:  # chained like &&: the first failure ends the job
        rc = subprocess.call(["timeout", "-k", "10", str(limit)] + cmd)
        if rc != 0:
            sys.exit(f"step failed ({rc}): {' '.join(cmd[-2:])}")


if __name__ == "__main__":
    main()
