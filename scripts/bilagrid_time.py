"""Times bilagrid.apply_to_render forward + backward (to both gradients) with FG_FUSED_BILAGRID=1 against the torch ops of the
same build, and writes profiles/bilagrid_fused.md.

    python scripts/bilagrid_time.py --measure out.json      on the GPU: the timed series, memory, differences, kernel-only times
    python scripts/bilagrid_time.py --train-step out.json   on the GPU: adds a harness.train_step series at 960 x 540 to that file
    python scripts/bilagrid_time.py --trace                 on the GPU, under `rocprofv3 --kernel-trace --stats`: three calls of
                                                            each path at 1920 x 1080, nothing else
    python scripts/bilagrid_time.py --report out.json [--stats kernel_stats.csv] [--resources remarks.txt]
                                                            anywhere: the markdown file from the recorded figures

Grid (16, 16, 8), 100 cameras; 480 x 270, 960 x 540 and 1920 x 1080 (the reference's three resolution phases).  The two paths
alternate call by call in one process; device events per call; warm-up first."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((480, 270), (960, 540), (1920, 1080))
GRID = (16, 16, 8)
NUM, CAM = 100, 37
HBM_PEAK = 8.0e12  # bytes / s (spec)


def _setup(W, H, dev):
    import torch

    from freegaussian_amd.bilagrid import BilateralGrid

    g = torch.Generator(device="cpu").manual_seed(W)
    m = BilateralGrid(num=NUM, grid_X=GRID[0], grid_Y=GRID[1], grid_W=GRID[2]).to(dev)
    with torch.no_grad():
        m.grids.add_(0.3 * torch.randn(m.grids.shape, generator=g).to(dev))
    rgb = torch.rand(1, H, W, 3, generator=g).to(dev).requires_grad_(True)
    v_out = torch.randn(1, H, W, 3, generator=g).to(dev)
    return m, rgb, v_out


def _call(m, rgb, v_out, knob):
    from freegaussian_amd import bilagrid

    os.environ["FG_FUSED_BILAGRID"] = knob
    m.grids.grad = rgb.grad = None
    out = bilagrid.apply_to_render(m, rgb, CAM, rgb.shape[1], rgb.shape[2])
    out.backward(v_out)
    return out


def _pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def measure(path, calls, warmup):
    import torch

    from freegaussian_amd import _lib, ops

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    res = {"device": torch.cuda.get_device_name(0), "calls": calls, "warmup": warmup, "sizes": {}}
    for W, H in SIZES:
        m, rgb, v_out = _setup(W, H, dev)
        for _ in range(warmup):
            for knob in ("1", "0"):
                _call(m, rgb, v_out, knob)
        torch.cuda.synchronize()
        events = {"1": [], "0": []}
        for _ in range(calls):
            for knob in ("1", "0"):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                _call(m, rgb, v_out, knob)
                b.record()
                events[knob].append((a, b))
        torch.cuda.synchronize()
        row = {}
        for knob, name in (("1", "fused"), ("0", "torch")):
            ms = [a.elapsed_time(b) for a, b in events[knob]]
            row[name] = {"median_ms": _pct(ms, 0.5), "p10_ms": _pct(ms, 0.1), "p90_ms": _pct(ms, 0.9)}
        # peak memory of one forward + backward, and the two paths' results
        got = {}
        for knob, name in (("1", "fused"), ("0", "torch")):
            m.grids.grad = rgb.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = _call(m, rgb, v_out, knob)
            torch.cuda.synchronize()
            row[name]["peak_bytes_over_inputs"] = torch.cuda.max_memory_allocated() - base
            got[name] = (out.detach().clone(), rgb.grad.clone(), m.grids.grad.clone())
        row["max_rel_diff"] = {k: float((a - b).abs().max() / b.abs().max()) for k, a, b in zip(("out", "v_rgb", "v_grids"), got["fused"], got["torch"])}
        # kernel-only: the C calls back to back between two events (the launches of one call: 1 forward, 3 backward)
        block, img = m.grids.detach()[CAM], rgb.detach()[0].contiguous()
        out_buf, v_rgb, v_grid = torch.empty_like(img), torch.empty_like(img), torch.empty_like(block)
        n_ws = int(lib.fg_bilagrid_bwd_workspace_bytes(H, W, *GRID))
        ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
        v = v_out[0].contiguous()
        s = ops._stream()
        reps = 50

        def timed(fn):
            for _ in range(5):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / reps

        P = lambda t: t.data_ptr()  # noqa: E731
        t_fwd = timed(lambda: _lib.check(lib.fg_bilagrid_slice_fwd(H, W, *GRID, P(block), P(img), P(out_buf), s), "fwd"))
        t_bwd = timed(lambda: _lib.check(lib.fg_bilagrid_slice_bwd(H, W, *GRID, P(block), P(img), P(v), P(v_rgb), P(v_grid), P(ws), n_ws, s), "bwd"))
        t_bwd_rgb = timed(lambda: _lib.check(lib.fg_bilagrid_slice_bwd(H, W, *GRID, P(block), P(img), P(v), P(v_rgb), None, None, 0, s), "bwd rgb"))
        px = H * W
        # bytes from shapes: forward reads rgb, writes out; backward reads rgb and v_out twice (v_rgb launch, gather), writes
        # v_rgb, writes and reads the partial blocks, writes v_grid
        fwd_bytes = 24 * px
        bwd_bytes = (24 + 12 + 24) * px + 2 * n_ws + block.numel() * 4
        row["kernels"] = {"fwd_ms": t_fwd, "bwd_ms": t_bwd, "bwd_v_rgb_only_ms": t_bwd_rgb, "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
                          "workspace_bytes": n_ws, "fwd_share_of_hbm": fwd_bytes / (t_fwd * 1e-3) / HBM_PEAK,
                          "bwd_share_of_hbm": bwd_bytes / (t_bwd * 1e-3) / HBM_PEAK}  # fmt: skip
        res["sizes"][f"{W}x{H}"] = row
        print(f"{W}x{H}", json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def train_steps(path, calls=60, warmup=20):
    """One `harness.train_step` series on the scene of tests/test_bilagrid_fused_gpu.py's model-level test at 960 x 540: the
    knob set and unset alternate step by step on one model; host clock around a step that ends in a synchronise."""
    import time

    import torch

    from freegaussian_amd.harness import build_optimizers, train_step
    from freegaussian_amd.model import FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import room_scene
    from scripts.train_e2e import camera_from_viewmat, render_ground_truth

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    dev = torch.device("cuda", 0)
    W, H = 960, 540
    scene, _ = room_scene(6000, W, H, n_views=40, seed=2)
    scene.viewmats, scene.Ks = scene.viewmats[:1], scene.Ks[:1]
    rgba = render_ground_truth(scene, dev)[0].float() / 255.0
    gt = rgba[..., :3] * rgba[..., 3:]
    torch.manual_seed(0)
    cfg = FreeGaussianModelConfig(use_bilateral_grid=True, grid_shape=GRID, background_color="black", num_downscales=0,
                                  warm_up=10**9, refine_every=10**9, num_random=4000, random_scale=3.0)  # fmt: skip
    m = FreeGaussianModel(cfg, num_train_data=2).to(dev).train()
    opts = build_optimizers(m)
    ms = {"1": [], "0": []}
    for step in range(1, warmup + calls + 1):
        for knob in ("1", "0"):
            os.environ["FG_FUSED_BILAGRID"] = knob
            cam = camera_from_viewmat(scene.viewmats[0].clone(), scene.Ks[0], W, H, 0.0)
            cam.metadata["cam_idx"] = step % 2
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train_step(m, opts, cam, gt, step)
            torch.cuda.synchronize()
            if step > warmup:
                ms[knob].append((time.perf_counter() - t0) * 1e3)
    res = json.load(open(path))
    res["train_step"] = {"size": f"{W}x{H}", "calls": calls, "gaussians": int(m.num_points),
                         **{name: {"median_ms": _pct(ms[k], 0.5), "p10_ms": _pct(ms[k], 0.1), "p90_ms": _pct(ms[k], 0.9)} for k, name in (("1", "fused"), ("0", "torch"))}}  # fmt: skip
    print("train_step", json.dumps(res["train_step"]), flush=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def trace():
    import torch

    assert torch.cuda.is_available(), "the trace needs a GPU"
    W, H = SIZES[-1]
    m, rgb, v_out = _setup(W, H, torch.device("cuda", 0))
    for knob in ("1", "0"):
        for _ in range(3):
            _call(m, rgb, v_out, knob)
    torch.cuda.synchronize()


def report(path, stats, resources):
    res = json.load(open(path))
    L = ["# Fused bilateral-grid slice against the torch ops (scripts/bilagrid_time.py)", ""]
    L += [f"Device: {res['device']}.  `bilagrid.apply_to_render` forward + backward to both gradients, grid (16, 16, 8), {NUM} cameras;",
          f"`FG_FUSED_BILAGRID=1` and the torch ops of the same build alternate call by call in one process; {res['warmup']} warm-up and",
          f"{res['calls']} timed calls per size and path, device events around each call (host launch gaps included).", ""]  # fmt: skip
    L += ["| size | fused median (p10 .. p90) ms | torch median (p10 .. p90) ms | fused / torch | verdict | default-on rule (<= 0.8) |", "|---|---|---|---|---|---|"]
    all_on = True
    for size, r in res["sizes"].items():
        f, t = r["fused"], r["torch"]
        ratio = f["median_ms"] / t["median_ms"]
        apart = f["p90_ms"] < t["p10_ms"] or t["p90_ms"] < f["p10_ms"]
        verdict = ("gain" if ratio < 1 else "loss") if apart else "no difference shown (ranges overlap)"
        all_on &= ratio <= 0.8
        L.append(f"| {size} | {f['median_ms']:.3f} ({f['p10_ms']:.3f} .. {f['p90_ms']:.3f}) | {t['median_ms']:.3f} ({t['p10_ms']:.3f} .. {t['p90_ms']:.3f}) "
                 f"| {ratio:.3f} | {verdict} | {'met' if ratio <= 0.8 else 'not met'} |")  # fmt: skip
    L += ["", f"Default-on rule (fused median <= 0.8 x torch at every size): {'met' if all_on else 'NOT met'}.  The knob stays opt-in either way.", ""]
    L += ["| size | peak memory over the inputs, fused | torch | largest difference fused - torch, relative to the torch array's largest magnitude |", "|---|---|---|---|"]
    for size, r in res["sizes"].items():
        d = r["max_rel_diff"]
        L.append(f"| {size} | {r['fused']['peak_bytes_over_inputs'] / 1e6:.1f} MB | {r['torch']['peak_bytes_over_inputs'] / 1e6:.1f} MB "
                 f"| out {d['out']:.1e}, v_rgb {d['v_rgb']:.1e}, v_grids {d['v_grids']:.1e} |")  # fmt: skip
    L += ["", "Kernels alone (the C calls back to back, 50 per figure, between two device events), bytes from shapes over time as a share of",
          "the 8.0 TB/s HBM peak.  Forward: 24 B per pixel.  Backward: rgb and v_out read by the v_rgb launch and again by the gather,",
          "v_rgb written, the partial blocks written and read, v_grid written.", "",
          "| size | forward ms | share | backward (3 launches) ms | share | backward, v_rgb alone ms | workspace |", "|---|---|---|---|---|---|---|"]  # fmt: skip
    for size, r in res["sizes"].items():
        k = r["kernels"]
        L.append(f"| {size} | {k['fwd_ms']:.4f} | {100 * k['fwd_share_of_hbm']:.1f} % | {k['bwd_ms']:.4f} | {100 * k['bwd_share_of_hbm']:.1f} % "
                 f"| {k['bwd_v_rgb_only_ms']:.4f} | {k['workspace_bytes'] / 1e6:.2f} MB |")  # fmt: skip
    if stats:
        rows = list(csv.DictReader(open(stats)))
        L += ["", "## Kernel table at 1920 x 1080: three calls of each path under `rocprofv3 --kernel-trace --stats` (a run of its own)", "",
              "| kernel | calls | total us | average us | share |", "|---|---|---|---|---|"]  # fmt: skip
        for r in rows[:24]:
            name = r.get("Name", "")[:110].replace("|", "/")
            L.append(f"| `{name}` | {r.get('Calls')} | {float(r.get('TotalDurationNs', 0)) / 1e3:.1f} | {float(r.get('AverageNs', 0)) / 1e3:.1f} | {r.get('Percentage')} |")
    else:
        L += ["", "Kernel table under `rocprofv3 --kernel-trace --stats`: not taken."]
    if resources:
        L += ["", "## The kernels' resources (`hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage`)", "",
              "| kernel | VGPRs | AGPRs | SGPRs | scratch B/lane | LDS B/block (static) | occupancy waves/SIMD |", "|---|---|---|---|---|---|---|"]  # fmt: skip
        import re

        text = open(resources).read()
        for blk in re.split(r"Function Name: ", text)[1:]:
            get = lambda key: (re.search(key + r": (\d+)", blk) or [None, "?"])[1]  # noqa: E731
            scratch, lds, occ = get(r"ScratchSize \[bytes/lane\]"), get(r"LDS Size \[bytes/block\]"), get(r"Occupancy \[waves/SIMD\]")
            L.append(f"| `{blk.split()[0]}` | {get('VGPRs')} | {get('AGPRs')} | {get('TotalSGPRs')} | {scratch} | {lds} | {occ} |")
        L += ["", "(`slice_kernel` adds dynamic LDS: 48 B per level and x node its 256-pixel row segment touches -- 1.5 KB at 1920 x 1080 with",
              "the default grid, at most 48 KB.)"]
    ts = res.get("train_step")
    if ts:
        f, t = ts["fused"], ts["torch"]
        apart = f["p90_ms"] < t["p10_ms"] or t["p90_ms"] < f["p10_ms"]
        L += ["", f"`harness.train_step` (host clock, synchronised) on the model-level test's scene at {ts['size']}, {ts['gaussians']} Gaussians, grid (16, 16, 8),",
              f"the knob set and unset alternating step by step on one model, {ts['calls']} timed steps each: fused {f['median_ms']:.2f} ms ({f['p10_ms']:.2f} .. {f['p90_ms']:.2f}),",
              f"torch {t['median_ms']:.2f} ms ({t['p10_ms']:.2f} .. {t['p90_ms']:.2f}), ratio {f['median_ms'] / t['median_ms']:.3f}: "
              + (("a gain" if f["median_ms"] < t["median_ms"] else "a loss") if apart else "no difference shown (ranges overlap)") + "."]  # fmt: skip
    else:
        L += ["", "A `harness.train_step` series on a whole scene: not done."]
    out = os.path.join(ROOT, "profiles", "bilagrid_fused.md")
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
    ap.add_argument("--train-step", help="add a harness.train_step series to the JSON file --measure wrote")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--report")
    ap.add_argument("--stats")
    ap.add_argument("--resources")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if a.measure:
        measure(a.measure, a.calls, a.warmup)
    if a.train_step:
        train_steps(a.train_step)
    if a.trace:
        trace()
    if a.report:
        report(a.report, a.stats, a.resources)
