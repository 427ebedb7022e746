"""Times "target + loss + PSNR" -- ``get_metrics_dict`` then ``get_loss_dict`` on one outputs dict, then the backward to the
render -- with FG_FUSED_TARGET=1 against the torch ops of the same build, and writes profiles/target_loss_fused.md.

    python scripts/target_loss_time.py --measure out.json      on the GPU: the timed series, memory, differences
    python scripts/target_loss_time.py --train-step out.json   on the GPU: adds a harness.train_step series at 960 x 540 from a
                                                               1080p RGBA uint8 source to that file
    python scripts/target_loss_time.py --trace fused|torch     on the GPU, under `rocprofv3 --kernel-trace --stats`: three calls
                                                               of that path at 960 x 540 from 1080p RGBA uint8 with a mask
    python scripts/target_loss_time.py --report out.json [--stats FUSED TORCH]    (the two traces' kernel_stats.csv or results .db)
                                                               anywhere: the markdown file from the recorded figures

Sources 1920 x 1080 at d = 4, 2, 1 and 800 x 800 at d = 1 (the blender / D-NeRF size); RGBA uint8 and RGB float32; with and
without a bool mask.  The two paths alternate call by call in one process; device events per call; warm-up first."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (source W0, H0, d, the source layouts measured)
ROWS = ((1920, 1080, 4, ("rgba_u8", "rgb_f32")), (1920, 1080, 2, ("rgba_u8", "rgb_f32")), (1920, 1080, 1, ("rgba_u8", "rgb_f32")),
        (800, 800, 1, ("rgba_u8",)))  # fmt: skip


def _model(d, dev):
    import torch

    from freegaussian_amd.model import FreeGaussianModel, FreeGaussianModelConfig

    torch.manual_seed(0)
    cfg = FreeGaussianModelConfig(num_downscales={1: 0, 2: 1, 4: 2, 8: 3}[d], resolution_schedule=10**9, background_color="random")
    m = FreeGaussianModel(cfg, num_points=64).to(dev).train()
    m.step = 0
    assert m._get_downscale_factor() == d
    return m


def _setup(W0, H0, d, layout, masked, dev):
    import torch

    g = torch.Generator(device="cpu").manual_seed(W0 + d)
    if layout == "rgba_u8":
        image = (torch.rand(H0, W0, 4, generator=g) * 256).clamp_max(255).to(torch.uint8)
    else:
        image = torch.rand(H0, W0, 3, generator=g)
    batch = {"image": image.to(dev)}
    if masked:
        batch["mask"] = (torch.rand(H0, W0, 1, generator=g) > 0.3).to(dev)
    pred = torch.rand(H0 // d, W0 // d, 3, generator=g).to(dev).requires_grad_(True)
    return _model(d, dev), pred, torch.rand(3, generator=g).to(dev), batch


def _call(m, pred, bg, batch, knob):
    os.environ["FG_FUSED_TARGET"] = knob
    pred.grad = None
    outputs = {"rgb": pred, "background": bg}
    metrics = m.get_metrics_dict(outputs, batch)
    loss = m.get_loss_dict(outputs, batch)
    loss["main_loss"].backward()
    return loss["main_loss"].detach(), metrics["psnr"].detach()


def _pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def measure(path, calls, warmup):
    import torch

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "calls": calls, "warmup": warmup, "rows": []}
    for W0, H0, d, layouts in ROWS:
        for layout in layouts:
            for masked in (False, True):
                m, pred, bg, batch = _setup(W0, H0, d, layout, masked, dev)
                for _ in range(warmup):
                    for knob in ("1", "0"):
                        _call(m, pred, bg, batch, knob)
                torch.cuda.synchronize()
                events = {"1": [], "0": []}
                for _ in range(calls):
                    for knob in ("1", "0"):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        _call(m, pred, bg, batch, knob)
                        b.record()
                        events[knob].append((a, b))
                torch.cuda.synchronize()
                row = {"source": f"{W0}x{H0}", "d": d, "output": f"{W0 // d}x{H0 // d}", "layout": layout, "mask": masked}
                got = {}
                for knob, name in (("1", "fused"), ("0", "torch")):
                    ms = [a.elapsed_time(b) for a, b in events[knob]]
                    row[name] = {"median_ms": _pct(ms, 0.5), "p10_ms": _pct(ms, 0.1), "p90_ms": _pct(ms, 0.9)}
                    # peak memory of one call over what is resident before it (model, render, batch)
                    pred.grad = None
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    loss, psnr = _call(m, pred, bg, batch, knob)
                    torch.cuda.synchronize()
                    row[name]["peak_bytes_over_inputs"] = torch.cuda.max_memory_allocated() - base
                    got[name] = (loss.clone(), psnr.clone(), pred.grad.clone())
                row["max_rel_diff"] = {k: float((a - b).abs().max() / b.abs().max()) for k, a, b in zip(("loss", "psnr", "v_pred"), got["fused"], got["torch"])}
                # (a render within rounding of its target takes either sign of the L1 term: such elements are counted, the rest compared)
                gf, gt_ = got["fused"][2], got["torch"][2]
                off = (gf - gt_).abs() > 1e-4 * gt_.abs().max()
                row["v_pred_sign_ties"] = int(off.sum())
                row["max_rel_diff"]["v_pred"] = float((gf - gt_).abs()[~off].max() / gt_.abs().max())
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def train_steps(path, calls=60, warmup=20):
    """One `harness.train_step` series on a small scene rendered at 960 x 540 against a 1920 x 1080 RGBA uint8 batch image
    (d = 2): the knob set and unset alternate step by step on one model; host clock around a step that ends in a synchronise."""
    import time

    import torch

    from freegaussian_amd.harness import build_optimizers, train_step
    from freegaussian_amd.model import FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import room_scene
    from scripts.train_e2e import camera_from_viewmat, render_ground_truth

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    dev = torch.device("cuda", 0)
    W, H = 1920, 1080
    scene, _ = room_scene(6000, W, H, n_views=40, seed=2)
    scene.viewmats, scene.Ks = scene.viewmats[:1], scene.Ks[:1]
    rgba = render_ground_truth(scene, dev)[0].contiguous()  # uint8 [1080,1920,4], resident on the device
    torch.manual_seed(0)
    cfg = FreeGaussianModelConfig(background_color="random", num_downscales=1, resolution_schedule=10**9, warm_up=10**9,
                                  refine_every=10**9, num_random=4000, random_scale=3.0)  # fmt: skip
    m = FreeGaussianModel(cfg, num_train_data=2).to(dev).train()
    opts = build_optimizers(m)
    ms = {"1": [], "0": []}
    for step in range(1, warmup + calls + 1):
        for knob in ("1", "0"):
            os.environ["FG_FUSED_TARGET"] = knob
            cam = camera_from_viewmat(scene.viewmats[0].clone(), scene.Ks[0], W, H, 0.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train_step(m, opts, cam, rgba, step)
            torch.cuda.synchronize()
            if step > warmup:
                ms[knob].append((time.perf_counter() - t0) * 1e3)
    res = json.load(open(path)) if os.path.exists(path) else {}
    res["train_step"] = {"size": "960x540 from 1920x1080 RGBA uint8", "calls": calls, "gaussians": int(m.num_points),
                         **{name: {"median_ms": _pct(ms[k], 0.5), "p10_ms": _pct(ms[k], 0.1), "p90_ms": _pct(ms[k], 0.9)} for k, name in (("1", "fused"), ("0", "torch"))}}  # fmt: skip
    print("train_step", json.dumps(res["train_step"]), flush=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def trace(path_name):
    """Three calls of ONE path ("fused" or "torch") and nothing else on the device: the launches of a call are the trace's
    kernel calls over three."""
    import torch

    assert torch.cuda.is_available(), "the trace needs a GPU"
    m, pred, bg, batch = _setup(1920, 1080, 2, "rgba_u8", True, torch.device("cuda", 0))
    for _ in range(3):
        _call(m, pred, bg, batch, {"fused": "1", "torch": "0"}[path_name])
    torch.cuda.synchronize()


def _kernel_calls(path):
    """[(kernel name, calls)] of a rocprofv3 run: its kernel_stats.csv, or its results database."""
    if path.endswith(".db"):
        import sqlite3

        return list(sqlite3.connect(path).execute("select name, count(*) from kernels group by name"))
    return [(r.get("Name", ""), int(r.get("Calls", 0) or 0)) for r in csv.DictReader(open(path))]


def _apart(f, t):
    return f["p90_ms"] < t["p10_ms"] or t["p90_ms"] < f["p10_ms"]


def report(path, stats):
    res = json.load(open(path))
    L = ["# Fused training target against the torch ops (scripts/target_loss_time.py)", ""]
    L += [f"Device: {res['device']}.  `get_metrics_dict` + `get_loss_dict` on one outputs dict + the backward to the render ('target +",
          "loss + PSNR'); `FG_FUSED_TARGET=1` and the torch ops of the same build (the knob-unset path) alternate call by call in one",
          f"process; {res['warmup']} warm-up and {res['calls']} timed calls per row and path, device events around each call (host launch",
          "gaps included).  Batch image, mask and render are resident on the device.", ""]  # fmt: skip
    L += ["| source | d | output | layout | mask | fused median (p10 .. p90) ms | torch median (p10 .. p90) ms | fused / torch | verdict | <= 0.8 |",
          "|---|---|---|---|---|---|---|---|---|---|"]  # fmt: skip
    all_on = True
    for r in res["rows"]:
        f, t = r["fused"], r["torch"]
        ratio = f["median_ms"] / t["median_ms"]
        verdict = ("gain" if ratio < 1 else "loss") if _apart(f, t) else "no difference shown (ranges overlap)"
        all_on &= ratio <= 0.8 and _apart(f, t)
        L.append(f"| {r['source']} | {r['d']} | {r['output']} | {r['layout']} | {'bool' if r['mask'] else '-'} | {f['median_ms']:.3f} ({f['p10_ms']:.3f} .. "
                 f"{f['p90_ms']:.3f}) | {t['median_ms']:.3f} ({t['p10_ms']:.3f} .. {t['p90_ms']:.3f}) | {ratio:.2f} | {verdict} | "
                 f"{'yes' if ratio <= 0.8 else 'no'} |")  # fmt: skip
    L += ["", "Peak memory of one call over what is resident before it, and the two paths' results against each other (v_pred: elements",
          "whose render lies within rounding of the target take either sign of the L1 term; they are counted, not compared):", "",
          "| source | d | layout | mask | fused peak over inputs MB | torch peak over inputs MB | max rel diff loss / psnr / v_pred | sign ties |", "|---|---|---|---|---|---|---|---|"]  # fmt: skip
    for r in res["rows"]:
        dd = r["max_rel_diff"]
        L.append(f"| {r['source']} | {r['d']} | {r['layout']} | {'bool' if r['mask'] else '-'} | {r['fused']['peak_bytes_over_inputs'] / 1e6:.1f} | "
                 f"{r['torch']['peak_bytes_over_inputs'] / 1e6:.1f} | {dd['loss']:.1e} / {dd['psnr']:.1e} / {dd['v_pred']:.1e} | {r.get('v_pred_sign_ties', 0)} |")  # fmt: skip
    if "train_step" in res:
        ts = res["train_step"]
        f, t = ts["fused"], ts["torch"]
        verdict = ("gain" if f["median_ms"] < t["median_ms"] else "loss") if _apart(f, t) else "no difference shown (ranges overlap)"
        L += ["", f"`harness.train_step`, {ts['size']}, {ts['gaussians']} Gaussians, {ts['calls']} steps per path alternating (host clock, step ends in a",
              f"synchronise): fused {f['median_ms']:.2f} ({f['p10_ms']:.2f} .. {f['p90_ms']:.2f}) ms, torch {t['median_ms']:.2f} ({t['p10_ms']:.2f} .. "
              f"{t['p90_ms']:.2f}) ms: {verdict}."]  # fmt: skip
    if stats:
        L += ["", "Kernel trace (`rocprofv3 --kernel-trace --stats`, a run of its own per path: three calls at 960 x 540 from 1080p RGBA",
              "uint8 with a mask, nothing else on the device; launches per call = kernel calls / 3):", "",
              "| path | kernels launched per call | distinct kernels | of them the new unit's | buffer copies in the whole run |", "|---|---|---|---|---|"]  # fmt: skip
        for name, path_ in zip(("fused", "torch"), stats):
            rows = _kernel_calls(path_)
            copies = sum(n for k, n in rows if "copyBuffer" in k)  # (the uploads of the set-up, and one per host scalar)
            rows = [(k, n) for k, n in rows if "copyBuffer" not in k]
            own = sum(n for k, n in rows if "target_loss" in k)
            L.append(f"| {name} | {sum(n for _, n in rows) / 3:.1f} | {len(rows)} | {own / 3:.1f} | {copies} |")
    L += ["", "Verdict by the project's rule (a gain only where the medians are apart and p10 .. p90 do not overlap; default-on only at",
          f"<= 0.8 x at every size): {'meets' if all_on else 'does NOT meet'} the default-on rule.  The knob stays opt-in either way."]  # fmt: skip
    print("\n".join(L))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure")
    ap.add_argument("--train-step")
    ap.add_argument("--trace", choices=("fused", "torch"))
    ap.add_argument("--report")
    ap.add_argument("--stats", nargs=2)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    a = ap.parse_args()
    if a.measure:
        measure(a.measure, a.calls, a.warmup)
    if a.train_step:
        train_steps(a.train_step)
    if a.trace:
        trace(a.trace)
    if a.report:
        report(a.report, a.stats)
