#!/usr/bin/env python3
"""Initial-scale neighbour search: ``ops.knn`` on the GPU against the route a CUDA tensor took before it existed
(device -> host copy + ``utils.knn_mean_distance`` on 16 CPU threads), on three 1M-point layouts and the 200k outlier set.  Writes
profiles/knn_init.md.

    python scripts/knn_init_bench.py [--out DIR] [--md profiles/knn_init.md]

runs the steps below as child processes, each under its own ``timeout -k 10``, stopping at the first that fails (a
fault or a time limit in one step starts nothing more on the GPU):

    --step gpu     ops.knn(x, 3): warm-up call, then the median of 20 calls between device events; the grid the library
                   builds (restated here on the host from the same sample) and the candidates per query it implies
    --step parent  the former route, timed once per layout (scikit-learn's tree query when it imports; otherwise the
                   former brute-force chunks, TWO of them timed and the rest extrapolated -- it says which)
    --step trace   two calls on the uniform layout, for ``rocprofv3 --kernel-trace --stats`` (a run of its own)
    --step sweep   (with --sweep) the same calls through every libfgraster_knn_occ*.so, builds with other FG_KNN_OCC
                   (`make -C freegaussian_amd/csrc knn-occ`), one child process each
    --step report  profiles/knn_init.md from these
"""
import argparse
import csv
import glob
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

N = 1_000_000
SAMPLE = 4096  # rows fg_knn samples to size its grid


def layouts():
    from freegaussian_amd.scenes import room_scene

    def uniform(n, seed):
        return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * 10

    def clustered():
        x = uniform(N, 2)
        x[: (4 * N) // 5] *= 0.2
        return x

    def outliers():
        n = 200_000  # (the set of tests/test_knn_gpu.py)
        x = uniform(n, 3)
        out = torch.randperm(n, generator=torch.Generator().manual_seed(4))[: n // 100]
        x[out] = (x[out] - 5.0) * 1000.0
        return x

    return {"uniform": lambda: uniform(N, 1), "clustered 0.8 / 0.2": clustered,
            "room_scene": lambda: room_scene(N, 320, 180)[0].means.detach().float().contiguous(),
            "1 % outliers at 1000 x": outliers}  # fmt: skip


def plan_grid(x):
    """The grid fg_knn plans for x (the library's own planner through its test hook, fed the rows fg_knn samples):
    (lo, h, inv, g, slack, occ) with occ = the FG_KNN_OCC the loaded library was built with."""
    import ctypes

    from freegaussian_amd import _lib

    n = x.shape[0]
    count = min(n, SAMPLE)
    s = x[(torch.arange(count, dtype=torch.int64) * n) // count].cpu().float().contiguous()
    f, i = (ctypes.c_float * 10)(), (ctypes.c_int32 * 4)()
    _lib.check(_lib.load().fg_debug_knn_grid(n, s.data_ptr(), count, f, i), "fg_debug_knn_grid")
    f = list(f)
    return f[0:3], f[3:6], f[6:9], list(i)[:3], f[9], i[3]


def candidates_per_query(x, dk, grid):
    """Mean number of points in the block of cells the search of each query ends on, the query itself not counted: from
    the cell histogram and the returned k-th distances (the search stops at the first ring whose nearest inner face is
    farther than the k-th neighbour -- then the block holds all k, so the final distance decides).  x, dk on one device."""
    lo, h, inv, g, slack, occ = grid
    dev = x.device
    c = [((x[:, a] - lo[a]) * inv[a]).floor().clamp(0, g[a] - 1).long() for a in range(3)]
    hist = torch.bincount((c[2] * g[1] + c[1]) * g[0] + c[0], minlength=g[0] * g[1] * g[2]).view(g[2], g[1], g[0])
    sat = torch.zeros(g[2] + 1, g[1] + 1, g[0] + 1, dtype=torch.int64, device=dev)
    sat[1:, 1:, 1:] = hist.cumsum(0).cumsum(1).cumsum(2)
    n = x.shape[0]
    R = torch.ones(n, dtype=torch.int64, device=dev)
    live = torch.ones(n, dtype=torch.bool, device=dev)
    for _ in range(max(g) + 1):
        bound = torch.full((n,), float("inf"), device=dev)
        for a in range(3):
            lo_face = x[:, a] - (lo[a] + (c[a] - R).float() * h[a])
            hi_face = (lo[a] + (c[a] + R + 1).float() * h[a]) - x[:, a]
            bound = torch.where(c[a] - R > 0, torch.minimum(bound, lo_face), bound)
            bound = torch.where(c[a] + R < g[a] - 1, torch.minimum(bound, hi_face), bound)
        b = (bound - slack).clamp_min(0)
        live &= ~(torch.isinf(bound) | (dk * dk < b * b))
        if not bool(live.any()):
            break
        R += live.long()
    a0 = [(c[a] - R).clamp(0, g[a]) for a in range(3)]
    a1 = [(c[a] + R + 1).clamp(0, g[a]) for a in range(3)]
    box = 0
    for sz, z in ((1, a1[2]), (-1, a0[2])):
        for sy, y in ((1, a1[1]), (-1, a0[1])):
            for sx, xx in ((1, a1[0]), (-1, a0[0])):
                box = box + sz * sy * sx * sat[z, y, xx]
    return {"occ": occ, "grid": g, "cells": g[0] * g[1] * g[2], "candidates_per_query": float((box - 1).double().mean()),
            "block_3x3x3_share": float((R == 1).double().mean()), "max_rings": int(R.max()),
            "max_cell": int(hist.max())}  # fmt: skip


def step_gpu(out):
    from freegaussian_amd import ops

    res = {}
    for name, make in layouts().items():
        x = make().cuda()
        d, _ = ops.knn(x, 3)  # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            d, _ = ops.knn(x, 3)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        ms.sort()
        res[name] = {"n": x.shape[0], "gpu_ms_median": ms[len(ms) // 2], "gpu_ms_min": ms[0], "gpu_ms_max": ms[-1],
                     **candidates_per_query(x, d[:, -1].contiguous(), plan_grid(x.cpu()))}  # fmt: skip
        print(name, json.dumps(res[name]), flush=True)
    json.dump(res, open(os.path.join(out, "gpu.json"), "w"), indent=1)


def step_parent(out):
    from freegaussian_amd import utils

    torch.set_num_threads(16)
    try:
        import sklearn  # noqa: F401

        have = True
    except ImportError:
        have = False
    res = {"sklearn": have}
    for name, make in layouts().items():
        x = make().cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xc = x.detach().cpu().float()
        copy_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        if have:
            utils.knn_mean_distance(xc, 3)
            note = "tree query"
            scale = 1.0
        else:  # the former fallback: cdist(2048 x N) per chunk; two chunks timed, only they are scaled up
            for i in (0, 2048):
                torch.cdist(xc[i : i + 2048], xc).topk(4, dim=1, largest=False)
            scale = xc.shape[0] / 4096.0
            note = "brute force, extrapolated from 2 of %d chunks" % math.ceil(xc.shape[0] / 2048)
        res[name] = {"parent_s": copy_s + (time.perf_counter() - t0) * scale, "copy_s": copy_s, "how": note}
        print(name, json.dumps(res[name]), flush=True)
    json.dump(res, open(os.path.join(out, "parent.json"), "w"), indent=1)


def _median_ms(x, k, reps=10):
    from freegaussian_amd import ops

    ops.knn(x, k)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.knn(x, k)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[reps // 2]


def step_sweep_one(out):
    """The library this process loaded (FG_RASTER_LIB): median of 10 calls per layout at k = 3 and k = 8."""
    res = {}
    for name, make in layouts().items():
        x = make().cuda()
        occ = plan_grid(x)[5]
        res[name] = {"k3_ms": _median_ms(x, 3), "k8_ms": _median_ms(x, 8)}
    print(json.dumps({"occ": occ, "ms": res}), flush=True)
    json.dump(res, open(os.path.join(out, f"sweep_occ{occ}.json"), "w"), indent=1)


def step_sweep(out):
    """One child per build of the library: the product build and every freegaussian_amd/libfgraster_knn_occ*.so
    (`make -C freegaussian_amd/csrc knn-occ`)."""
    libs = [None] + sorted(glob.glob(os.path.join(ROOT, "freegaussian_amd", "libfgraster_knn_occ*.so")))
    for lib in libs:
        env = dict(os.environ)
        if lib:
            env["FG_RASTER_LIB"] = lib
        rc = subprocess.call(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--out", out,
                              "--step", "sweep-one"], env=env)  # fmt: skip
        if rc != 0:
            sys.exit(f"sweep: {lib or 'product build'} failed ({rc})")


def step_trace(out):
    from freegaussian_amd import ops

    x = layouts()["uniform"]().cuda()
    for _ in range(2):
        ops.knn(x, 3)
    torch.cuda.synchronize()


def step_report(out, md):
    gpu = json.load(open(os.path.join(out, "gpu.json")))
    par = json.load(open(os.path.join(out, "parent.json")))
    L = ["# Initial scales: `ops.knn` against the host route", "",
         "Written by `scripts/knn_init_bench.py` on an MI355X box.  k = 3; per-query columns divide by the layout's n.  GPU: median of 20 calls",
         "between device events after a warm-up call (the call's own read-back of the grid sample included).  Host: the",
         "route a CUDA tensor took before `ops.knn` -- device -> host copy + `utils.knn_mean_distance` on 16 threads --",
         f"timed once; scikit-learn importable on that box: **{'yes' if par['sklearn'] else 'no'}**.", "",
         f"Occupancy constant `FG_KNN_OCC` = {gpu['uniform']['occ']} points per cell (mean).  Candidates per query: points in the block of",
         "cells each query's search ends on, counted on the host from the cell histogram and the returned distances.", "",
         "| layout | n | grid | GPU ms (min .. max) | host s | host / GPU | candidates / query | vs uniform | time per query vs uniform | 3x3x3 enough | most rings | fullest cell |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|"]  # fmt: skip
    u = gpu["uniform"]
    for name, r in gpu.items():
        p = par[name]
        L.append(f"| {name} | {r['n']} | {'x'.join(map(str, r['grid']))} | {r['gpu_ms_median']:.2f} ({r['gpu_ms_min']:.2f} .. {r['gpu_ms_max']:.2f}) | "
                 f"{p['parent_s']:.2f} ({p['how']}) | {p['parent_s'] * 1e3 / r['gpu_ms_median']:.0f} x | {r['candidates_per_query']:.0f} | "
                 f"{r['candidates_per_query'] / u['candidates_per_query']:.1f} x | {r['gpu_ms_median'] / r['n'] / (u['gpu_ms_median'] / u['n']):.1f} x | "
                 f"{100 * r['block_3x3x3_share']:.1f} % | {r['max_rings']} | {r['max_cell']} |")  # fmt: skip
    stats = sorted(glob.glob(os.path.join(out, "trace", "**", "*kernel_stats.csv"), recursive=True))
    L += ["", "## Kernels of two calls on the uniform layout (`rocprofv3 --kernel-trace --stats`, a run of its own)", ""]
    if stats:
        rows = list(csv.DictReader(open(stats[0])))
        L += ["| kernel | calls | total us | average us | share % |", "|---|---|---|---|---|"]
        for r in rows[:16]:
            L.append(f"| `{r['Name'][:90]}` | {r['Calls']} | {float(r['TotalDurationNs']) / 1e3:.1f} | "
                     f"{float(r['AverageNs']) / 1e3:.1f} | {float(r['Percentage']):.1f} |")  # fmt: skip
    else:
        L.append("(no kernel table: the trace step left no *kernel_stats.csv)")
    sweep = {}
    for f in glob.glob(os.path.join(out, "sweep_occ*.json")):
        sweep[int(os.path.basename(f)[len("sweep_occ"):-len(".json")])] = json.load(open(f))
    if sweep:
        names = list(gpu)
        L += ["", "## `FG_KNN_OCC` sweep (`--sweep`: one build of the library per value, median of 10 calls, ms at k = 3 / k = 8)", "",
              "| points per cell | " + " | ".join(names) + " |", "|---|" + "---|" * len(names)]  # fmt: skip
        for occ in sorted(sweep):
            L.append(f"| {occ} | " + " | ".join(f"{sweep[occ][n]['k3_ms']:.2f} / {sweep[occ][n]['k8_ms']:.2f}" for n in names) + " |")
    extra = os.path.join(os.path.dirname(md), "knn_init_notes.md")
    if os.path.exists(extra):
        L += ["", open(extra).read().rstrip()]
    open(md, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["gpu", "parent", "trace", "sweep", "sweep-one", "report"])
    ap.add_argument("--sweep", action="store_true", help="also time every libfgraster_knn_occ*.so build (make knn-occ)")
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "knn_init"))
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "knn_init.md"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.step:
        if a.step == "report":
            return step_report(a.out, a.md)
        return {"gpu": step_gpu, "parent": step_parent, "trace": step_trace, "sweep": step_sweep,
                "sweep-one": step_sweep_one}[a.step](a.out)  # fmt: skip
    me = [sys.executable, os.path.abspath(__file__), "--out", a.out, "--md", a.md, "--step"]
    steps = [(300, me + ["gpu"]), (900, me + ["parent"]),
             (300, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(a.out, "trace"), "-o",
                    "knn", "--"] + me + ["trace"]),
             ] + ([(1300, me + ["sweep"])] if a.sweep else []) + [(60, me + ["report"])]  # fmt: skip
    for limit, cmd in steps:  # chained like &&: the first failure ends the job
        rc = subprocess.call(["timeout", "-k", "10", str(limit)] + cmd)
        if rc != 0:
            sys.exit(f"step failed ({rc}): {' '.join(cmd[-2:])}")


if __name__ == "__main__":
    main()
