#!/usr/bin/env python3
"""The clustering of the dynamic Gaussians: what ``ops.dbscan`` / ``fg_dbscan`` costs, stage by stage, whether staging
the core and union passes through LDS beats direct loads, and scikit-learn on the same host.  Writes profiles/dbscan.md.

    make -C freegaussian_amd/csrc dbscan-staged        # the second side: libfgraster_dbscan_staged.so
    python scripts/dbscan_bench.py [--out DIR] [--md profiles/dbscan.md]

runs the steps below as child processes, each under its own ``timeout -k 10``, stopping at the first that fails (a fault
or a time limit in one step starts nothing more on the GPU):

    --step gpu      per case: both builds once (their labels must be equal), then the two alternating call by call in one
                    process (scripts/fused_bench_common.py: 10 warm-up and 50 timed calls between device events, median
                    (p10 .. p90)), then the per-stage times of each build from the device events of its measurement hook
    --step sklearn  ``sklearn.cluster.DBSCAN`` on the same points on the host, timed once per case (where it imports)
    --step report   profiles/dbscan.md from these and from the kernels' resource table (needs hipcc only, no GPU)

Cases: uniform points and the ``room_scene`` means at 33 000 / 240 000 / 1 000 000 rows, eps = the median distance to the
third neighbour (``ops.knn``) so that at min_samples 4 about half the rows are core and core, border and noise rows mix;
and 20 000 rows inside one eps-ball."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import fused_bench_common as C  # noqa: E402

SIZES = (33_000, 240_000, 1_000_000)
MIN_SAMPLES = 4
STAGES = ("grid", "core", "mark", "union", "roots + numbering", "labels")
STAGED_LIB = os.path.join(ROOT, "freegaussian_amd", "libfgraster_dbscan_staged.so")


def cases():
    from freegaussian_amd.scenes import room_scene

    out = []
    for n in SIZES:
        out.append(("uniform", n, lambda n=n: torch.rand(n, 3, generator=torch.Generator().manual_seed(n)) * 10, None))
        out.append(("room_scene", n, lambda n=n: room_scene(n, 320, 180)[0].means.detach().float().contiguous(), None))
    out.append(("one eps-ball", 20_000, lambda: torch.rand(20_000, 3, generator=torch.Generator().manual_seed(5)) * 0.25, 0.5))
    return out


def eps_of(x, eps):
    """The case's eps: given, or the median distance to the third neighbour (rounded to 3 digits, so that the host step
    uses the same number)."""
    from freegaussian_amd import ops

    if eps is not None:
        return eps
    return float(f"{float(ops.knn(x, 3)[0][:, 2].median()):.3g}")


class Side:
    """One build of the library on one point set: its own outputs and workspace."""

    def __init__(self, lib, x, eps):
        from freegaussian_amd import _lib

        self.lib, self.x, self.eps, self.n = lib, x, eps, x.shape[0]
        for name in ("fg_dbscan", "fg_debug_dbscan_stages", "fg_dbscan_workspace_bytes"):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = {**_lib.SIGNATURES, **_lib._EXTRA}[name]
        dev = x.device
        self.labels = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.core = torch.empty(self.n, dtype=torch.uint8, device=dev)
        self.counts = torch.empty(2, dtype=torch.int32, device=dev)
        self.ws = torch.empty(int(lib.fg_dbscan_workspace_bytes(self.n)), dtype=torch.uint8, device=dev)
        self.ms, self.staged = (ctypes.c_float * len(STAGES))(), ctypes.c_int32(-1)

    def _args(self):
        return (self.n, self.x.data_ptr(), self.eps, MIN_SAMPLES, self.labels.data_ptr(), self.core.data_ptr(),
                self.counts.data_ptr(), self.ws.data_ptr(), self.ws.numel(), torch.cuda.current_stream().cuda_stream)  # fmt: skip

    def call(self):
        rc = self.lib.fg_dbscan(*self._args())
        assert rc == 0, rc

    def stages(self):
        rc = self.lib.fg_debug_dbscan_stages(*self._args(), self.ms, ctypes.byref(self.staged))
        assert rc == 0, rc
        return list(self.ms)


def step_gpu(out):
    from freegaussian_amd import _lib

    libs = {"direct": _lib.load()}
    if os.path.exists(STAGED_LIB):
        libs["staged"] = ctypes.CDLL(STAGED_LIB)
    res = {"staged_build": "staged" in libs, "cases": []}
    for layout, n, make, eps in cases():
        x = make().cuda()
        eps = eps_of(x, eps)
        sides = {k: Side(lib, x, eps) for k, lib in libs.items()}
        for k, s in sides.items():
            s.stages()
            assert s.staged.value == (1 if k == "staged" else 0), (k, s.staged.value)
            s.call()
        torch.cuda.synchronize()
        d = sides["direct"]
        k_found, status = d.counts.tolist()
        assert status == 0
        for s in sides.values():  # the builds must agree before their times mean anything
            assert torch.equal(s.labels, d.labels) and torch.equal(s.core, d.core) and s.counts.tolist() == [k_found, 0]
        core = d.core.bool()
        r = {"layout": layout, "n": n, "eps": eps, "K": k_found, "core": int(core.sum()), "border": int(((d.labels >= 0) & ~core).sum()),
             "noise": int((d.labels < 0).sum()), "workspace_MiB": d.ws.numel() / 2**20,
             "call_ms": C.alternate({k: s.call for k, s in sides.items()})}  # fmt: skip
        per = {k: [] for k in sides}
        for i in range(3 + 21):
            for k, s in sides.items():
                ms = s.stages()
                if i >= 3:
                    per[k].append(ms)
        r["stage_ms"] = {k: [C.quantiles([row[j] for row in rows]) for j in range(len(STAGES))] for k, rows in per.items()}
        r["core_union_ms"] = {k: C.quantiles([row[1] + row[3] for row in rows]) for k, rows in per.items()}
        res["cases"].append(r)
        print(json.dumps(r), flush=True)
        del sides, x
    json.dump(res, open(os.path.join(out, "gpu.json"), "w"), indent=1)


def step_sklearn(out):
    gpu = json.load(open(os.path.join(out, "gpu.json")))
    try:
        from sklearn.cluster import DBSCAN
        import sklearn
    except ImportError:
        json.dump({"sklearn": None}, open(os.path.join(out, "sklearn.json"), "w"))
        return
    res = {"sklearn": sklearn.__version__, "threads": 16, "cases": []}
    made = {(layout, n): make for layout, n, make, _ in cases()}
    for r in gpu["cases"]:
        x = made[(r["layout"], r["n"])]().numpy()
        t0 = time.perf_counter()
        labels = DBSCAN(eps=r["eps"], min_samples=MIN_SAMPLES, n_jobs=16).fit(x).labels_
        s = time.perf_counter() - t0
        res["cases"].append({"layout": r["layout"], "n": r["n"], "seconds": s, "K": int(labels.max()) + 1})
        print(json.dumps(res["cases"][-1]), flush=True)
        json.dump(res, open(os.path.join(out, "sklearn.json"), "w"), indent=1)  # (after every case: a later one may run out of time)


def step_report(out, md):
    gpu = json.load(open(os.path.join(out, "gpu.json")))
    sk_path = os.path.join(out, "sklearn.json")
    sk = json.load(open(sk_path)) if os.path.exists(sk_path) else {"sklearn": None}
    sk_s = {(c["layout"], c["n"]): c for c in sk.get("cases", [])}
    both = gpu["staged_build"]
    L = ["# `ops.dbscan`: what the clustering of the dynamic Gaussians costs", "",
         "Written by `scripts/dbscan_bench.py` from runs on an MI355X.  A capability: its cost is stated, no ratio is promised.",
         f"min_samples {MIN_SAMPLES}; eps of the uniform and `room_scene` cases = the median distance to the third neighbour, so that core,",
         "border and noise rows mix.  Whole call: the library call between device events, its read-back of the grid sample",
         "included, 10 warm-up and 50 timed calls, the two builds alternating call by call in one process, median (p10 .. p90) in ms.",
         "", "## Whole call", "",
         "| layout | rows | eps | K | core | border | noise | workspace MiB | direct loads (the product build) | core and union staged through LDS | staged against direct | scikit-learn, same host |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|"]  # fmt: skip
    for r in gpu["cases"]:
        c = r["call_ms"]
        s = sk_s.get((r["layout"], r["n"]))
        if sk["sklearn"] is None:
            base = "not available"
        elif s is None:
            base = "not run at this size"
        else:
            base = f"{s['seconds']:.2f} s (K {s['K']}), {s['seconds'] * 1e3 / c['direct']['median']:.0f} x"
        L.append(f"| {r['layout']} | {r['n']} | {r['eps']:g} | {r['K']} | {r['core']} | {r['border']} | {r['noise']} | {r['workspace_MiB']:.0f} | "
                 f"{C.cell(c['direct'])} | {C.cell(c['staged']) if both else 'not built'} | "
                 f"{C.verdict(c['staged'], c['direct']) if both else '-'} | {base} |")  # fmt: skip
    if sk["sklearn"]:
        L += ["", f"scikit-learn {sk['sklearn']}: `DBSCAN(eps, min_samples={MIN_SAMPLES}, n_jobs=16).fit(x)` on float32 input, timed once, "
              "its own choice of neighbour search; K may differ by pairs at the rounding edge of eps."]  # fmt: skip
    else:
        L += ["", "scikit-learn did not import on that host: no baseline was measured."]
    for k in (["direct", "staged"] if both else ["direct"]):
        L += ["", f"## Stages, {'direct loads' if k == 'direct' else 'core and union staged through LDS'}", "",
              "Between device events inside one call (the measurement hook), 3 warm-up and 21 timed calls, median (p10 .. p90) in ms.", "",
              "| layout | rows | " + " | ".join(STAGES) + " |", "|---|---|" + "---|" * len(STAGES)]  # fmt: skip
        for r in gpu["cases"]:
            L.append(f"| {r['layout']} | {r['n']} | " + " | ".join(C.cell(q) for q in r["stage_ms"][k]) + " |")
    L += ["", "## The staging decision", ""]
    if both:
        L += ["Core + union time per call, staged against direct, by the rule (medians apart, p10 .. p90 not overlapping):", "",
              "| layout | rows | direct | staged | verdict |", "|---|---|---|---|---|"]
        verdicts = []
        for r in gpu["cases"]:
            cu = r["core_union_ms"]
            verdicts.append(C.verdict(cu["staged"], cu["direct"]))
            L.append(f"| {r['layout']} | {r['n']} | {C.cell(cu['direct'])} | {C.cell(cu['staged'])} | {verdicts[-1]} |")
        gains = sum(v.startswith("gain") for v in verdicts)
        losses = sum(v.startswith("loss") for v in verdicts)
        L += ["", f"Staged is a gain in {gains}, a loss in {losses} and no difference in {len(verdicts) - gains - losses} of {len(verdicts)} cases.",
              "Rule: the simpler variant (direct loads) stays unless the staged one is a gain.  "
              + ("It is a gain in every case: the staged build should become the product build."
                 if gains == len(verdicts) else "It is not a gain across the cases: the product build keeps direct loads; "
                 "`FG_DBSCAN_STAGED=1` remains a measurement build (`make dbscan-staged`).")]  # fmt: skip
    else:
        L += ["The staged build was not there: not measured.  The product build keeps direct loads, the simpler variant."]
    for k, extra in (("direct loads", ()), ("core and union staged through LDS", ("-DFG_DBSCAN_STAGED=1",))):
        rows = [r for r in C.kernel_resources(C.csrc("dbscan.hip"), ("-ffp-contract=off",) + extra) if r["kernel"].startswith("db_")]
        L += ["", f"## Kernel resources, {k} (`-Rpass-analysis=kernel-resource-usage`, gfx950)", "",
              "| kernel | VGPRs | SGPRs | scratch bytes / lane | LDS bytes / block | waves / SIMD |", "|---|---|---|---|---|---|"]
        for r in rows:
            L.append(f"| `{r['kernel']}` | {r.get('VGPRs')} | {r.get('TotalSGPRs')} | {r.get('ScratchSize')} | {r.get('LDS')} | {r.get('Occupancy')} |")
    notes = os.path.join(os.path.dirname(md), "dbscan_notes.md")
    if os.path.exists(notes):
        L += ["", open(notes).read().rstrip()]
    open(md, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["gpu", "sklearn", "report"])
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "dbscan"))
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "dbscan.md"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.step:
        return {"gpu": lambda: step_gpu(a.out), "sklearn": lambda: step_sklearn(a.out), "report": lambda: step_report(a.out, a.md)}[a.step]()
    me = [sys.executable, os.path.abspath(__file__), "--out", a.out, "--md", a.md, "--step"]
    for limit, cmd in ((420, me + ["gpu"]), (600, me + ["sklearn"]), (120, me + ["report"])):  # chained like &&
        rc = subprocess.call(["timeout", "-k", "10", str(limit)] + cmd)
        if rc != 0:
            sys.exit(f"step failed ({rc}): {' '.join(cmd[-2:])}")


if __name__ == "__main__":
    main()
