"""Times bilagrid.color_correct with FG_FUSED_COLOR_CORRECT=1 against the torch ops of the same build (knob unset), and one
harness.average_image_metrics with color_corrected_metrics on both ways; writes profiles/color_correct_fused.md.

    python scripts/color_correct_bench.py --measure out.json     on the GPU: the timed series, the differences, the eval loop
    python scripts/color_correct_bench.py --trace W H            on the GPU, under `rocprofv3 --kernel-trace --stats`: three fused
                                                                 calls at that size, nothing else
    python scripts/color_correct_bench.py --report out.json [--stats WxH:kernel_stats.csv ...]
                                                                 anywhere: the markdown file from the recorded figures

480 x 270, 960 x 540 and 1920 x 1080 (the reference's three resolution phases) on a rendered-like pair: a smooth random
field, and the same field through an affine-plus-quadratic colour change with 1 % noise.  The two paths alternate call by
call in one process; host clock around a call that ends in a device synchronise (the torch path's time is mostly host
work: fifteen float64 copies and factorizations a call); warm-up first.  The torch path gets fewer calls (--torch-calls,
per size): a call takes seconds at 1920 x 1080."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((480, 270), (960, 540), (1920, 1080))
KNOB = "FG_FUSED_COLOR_CORRECT"


def _pair(W, H, dev):
    import torch
    import torch.nn.functional as F

    g = torch.Generator(device="cpu").manual_seed(W)
    low = torch.rand(1, 3, max(H // 16, 2), max(W // 16, 2), generator=g) * 0.9 + 0.05
    ref = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True)[0].permute(1, 2, 0).contiguous()
    M = torch.tensor([[0.9, 0.05, 0.0], [0.02, 0.85, 0.03], [0.0, 0.04, 0.8]])
    img = ref @ M.T + torch.tensor([0.03, 0.01, 0.05]) + 0.08 * ref * ref + 0.01 * torch.randn(H, W, 3, generator=g)
    return img.clamp(0, 1).to(dev), ref.to(dev)


def _pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def _summary(ms):
    return {"calls": len(ms), "median_ms": _pct(ms, 0.5), "p10_ms": _pct(ms, 0.1), "p90_ms": _pct(ms, 0.9)}


def _timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _eval_loop(dev, views=3, W=480, H=270, n=4000):
    """One harness.average_image_metrics over `views` views of a small random scene, color_corrected_metrics on, each way."""
    import torch

    from freegaussian_amd import harness
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, color_corrected_metrics=True)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-3.2)
    with torch.no_grad():
        model.gauss_params["scales"].fill_(-3.2)
    model.step = 4000
    model = model.to(dev)
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1
    f = W / 160.0
    pairs = []
    for v in range(views):
        cam = Camera(c2w[None, :3], 140.0 * f, 150.0 * f, W / 2, H / 2, W, H, times=torch.tensor([[0.2 + 0.2 * v]]))
        model.eval()
        rgb = model.get_outputs_for_camera(cam)["rgb"]
        gt = (0.9 * rgb + 0.03 + 0.05 * rgb * rgb + 0.01 * torch.randn_like(rgb)).clamp(0, 1)
        pairs.append((cam, {"image": gt}))
    res = {"views": views, "size": f"{W}x{H}", "gaussians": n}
    for knob, name in (("1", "fused"), ("0", "torch")):
        os.environ[KNOB] = knob
        harness.average_image_metrics(model, pairs)  # warm-up
        ms, metrics = _timed(lambda: harness.average_image_metrics(model, pairs))
        res[name] = {"wall_ms": ms, "fps": metrics["fps"], "cc_psnr": metrics["cc_psnr"], "cc_ssim": metrics["cc_ssim"], "psnr": metrics["psnr"]}
    return res


def measure(path, calls, torch_calls, warmup):
    import torch

    from freegaussian_amd import bilagrid

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "warmup": warmup, "sizes": {}}

    def call(img, ref, knob):
        os.environ[KNOB] = knob
        return bilagrid.color_correct(img, ref)

    for (W, H), n_torch in zip(SIZES, torch_calls):
        img, ref = _pair(W, H, dev)
        for _ in range(warmup):
            call(img, ref, "1")
        call(img, ref, "0")
        ms = {"1": [], "0": []}
        out = {}
        for r in range(max(calls, n_torch)):
            for knob, n in (("1", calls), ("0", n_torch)):
                if r < n:
                    t, out[knob] = _timed(lambda: call(img, ref, knob))
                    ms[knob].append(t)
        row = {"fused": _summary(ms["1"]), "torch": _summary(ms["0"]), "max_abs_diff": float((out["1"] - out["0"]).abs().max())}
        res["sizes"][f"{W}x{H}"] = row
        print(f"{W}x{H}", json.dumps(row), flush=True)
    res["eval_loop"] = _eval_loop(dev)
    print("eval_loop", json.dumps(res["eval_loop"]), flush=True)
    os.environ.pop(KNOB, None)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def trace(W, H):
    import torch

    from freegaussian_amd import bilagrid

    assert torch.cuda.is_available(), "the trace needs a GPU"
    img, ref = _pair(W, H, torch.device("cuda", 0))
    os.environ[KNOB] = "1"
    for _ in range(3):
        bilagrid.color_correct(img, ref)
    torch.cuda.synchronize()


def report(path, stats=()):
    import csv

    res = json.load(open(path))
    L = ["# Fused colour correction against the torch ops (scripts/color_correct_bench.py)", ""]
    L += [f"Device: {res['device']}.  `bilagrid.color_correct(img, ref)` (5 iterations) on a rendered-like pair; `FG_FUSED_COLOR_CORRECT=1` and the",
          f"torch ops of the same build (knob unset) alternate call by call in one process; {res['warmup']} warm-up calls, host clock around a call",
          "that ends in a device synchronise.  Calls per path and size are in the table: the torch path gets fewer.", ""]  # fmt: skip
    L += ["| size | fused median (p10 .. p90) ms, calls | torch median (p10 .. p90) ms, calls | fused / torch | verdict | default-on rule (<= 0.8) | largest difference |",
          "|---|---|---|---|---|---|---|"]  # fmt: skip
    all_on = True
    for size, r in res["sizes"].items():
        f, t = r["fused"], r["torch"]
        ratio = f["median_ms"] / t["median_ms"]
        apart = f["p90_ms"] < t["p10_ms"] or t["p90_ms"] < f["p10_ms"]
        verdict = ("gain" if ratio < 1 else "loss") if apart else "no difference shown (ranges overlap)"
        all_on &= ratio <= 0.8
        L.append(f"| {size} | {f['median_ms']:.3f} ({f['p10_ms']:.3f} .. {f['p90_ms']:.3f}), {f['calls']} | {t['median_ms']:.1f} ({t['p10_ms']:.1f} .. {t['p90_ms']:.1f}), {t['calls']} "
                 f"| {ratio:.5f} | {verdict} | {'met' if ratio <= 0.8 else 'not met'} | {r['max_abs_diff']:.1e} |")  # fmt: skip
    L += ["", f"Default-on rule (fused median <= 0.8 x torch at every size): {'met' if all_on else 'NOT met'}.  The knob stays opt-in whatever the numbers",
          "are: where an image channel is 0 everywhere the two paths differ (the torch path's default `lstsq` driver does not return a",
          "least-squares fit there; bilagrid.color_correct's docstring), and a default must change no result.", ""]  # fmt: skip
    e = res.get("eval_loop")
    if e:
        f, t = e["fused"], e["torch"]
        L += [f"`harness.average_image_metrics` over {e['views']} views at {e['size']}, {e['gaussians']} Gaussians, `color_corrected_metrics` on, one timed call each way",
              f"after a warm-up call (host clock, synchronised; ONE call: no spread was taken): fused {f['wall_ms']:.1f} ms (fps {f['fps']:.1f}), torch {t['wall_ms']:.1f} ms",
              f"(fps {t['fps']:.1f}).  cc_psnr {f['cc_psnr']:.4f} / {t['cc_psnr']:.4f}, cc_ssim {f['cc_ssim']:.5f} / {t['cc_ssim']:.5f} (fused / torch)."]  # fmt: skip
    else:
        L += ["A `harness.average_image_metrics` series: not done."]
    if not stats:
        L += ["", "Kernel table under `rocprofv3 --kernel-trace --stats`: not taken."]
    for item in stats:
        size, _, csv_path = item.partition(":")
        L += ["", f"## Kernels of three fused calls at {size} under `rocprofv3 --kernel-trace --stats` (a run of its own)", "",
              "| kernel | calls | total us | average us | share |", "|---|---|---|---|---|"]  # fmt: skip
        for r in list(csv.DictReader(open(csv_path)))[:8]:
            name = r.get("Name", "")[:110].replace("|", "/")
            L.append(f"| `{name}` | {r.get('Calls')} | {float(r.get('TotalDurationNs', 0)) / 1e3:.1f} | {float(r.get('AverageNs', 0)) / 1e3:.1f} | {r.get('Percentage')} |")
    out = os.path.join(ROOT, "profiles", "color_correct_fused.md")
    if os.path.exists(out):  # the hand-written section at the end is kept
        old = open(out).read()
        if "\n## Notes" in old:
            L += ["", old[old.index("\n## Notes") + 1 :].rstrip("\n")]
    with open(out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure")
    ap.add_argument("--report")
    ap.add_argument("--trace", type=int, nargs=2, metavar=("W", "H"))
    ap.add_argument("--stats", action="append", default=[], help="WxH:path of a kernel_stats.csv, for --report")
    ap.add_argument("--calls", type=int, default=50, help="fused calls per size")
    ap.add_argument("--torch-calls", type=int, nargs=3, default=(10, 6, 3), help="torch calls at the three sizes")
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.measure:
        measure(a.measure, a.calls, tuple(a.torch_calls), a.warmup)
    if a.trace:
        trace(*a.trace)
    if a.report:
        report(a.report, a.stats)
