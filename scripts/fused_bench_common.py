"""What the benchmarks of the opt-in fused ops share (scripts/se3_apply_bench.py, scripts/control_bench.py): the project's
measuring rule, stated once.

Protocol: the two sides alternate call by call in one process, ``WARM`` warm-up and ``TIMED`` timed calls between device
events, median (p10 .. p90).  A gain = medians apart with p10 .. p90 not overlapping.  ``kernel_resources`` needs hipcc only."""
import os
import re
import subprocess
import time

import torch

WARM, TIMED = 10, 50


def quantiles(ms):
    s = sorted(ms)
    return {"median": s[len(s) // 2], "p10": s[len(s) // 10], "p90": s[(9 * len(s)) // 10]}


def alternate(sides, warm=WARM, timed=TIMED):
    """``sides``: {name: callable}; the callables alternate call by call -> {name: quantiles of ms between device events}."""
    ms = {k: [] for k in sides}
    for i in range(warm + timed):
        for k, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warm:
                ms[k].append(a.elapsed_time(b))
    return {k: quantiles(v) for k, v in ms.items()}


def host_ms_per_step(sides, steps=TIMED, rounds=3):
    """Host wall time per call of ``steps`` calls in a row with nothing that waits for the GPU in between."""
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            out[k].append((time.perf_counter() - t0) * 1e3 / steps)
            torch.cuda.synchronize()
    return out


def cell(q):
    return f"{q['median']:.3f} ({q['p10']:.3f} .. {q['p90']:.3f})"


def verdict(a, b):
    """a against b by the project's rule."""
    if a["p90"] < b["p10"]:
        return f"gain, {a['median'] / b['median']:.2f} x"
    if b["p90"] < a["p10"]:
        return f"loss, {a['median'] / b['median']:.2f} x"
    return "no difference"


def kernel_resources(src_path, extra=()):
    """The kernels of one .hip unit with what ``-Rpass-analysis=kernel-resource-usage`` says of each, for gfx950
    (``extra``: further compiler flags, such as the -D of a measurement build)."""
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only",
           *extra, "-Rpass-analysis=kernel-resource-usage", "-c", src_path, "-o", os.devnull]  # fmt: skip
    text = subprocess.run(cmd, capture_output=True, text=True).stderr
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            cur = {"kernel": re.sub(r"\(anonymous namespace\)::|\(.*$|^void ", "", name)}
            rows.append(cur)
        else:
            cur[m.group(1).split(" ")[0]] = m.group(2)
    return rows


def csrc(unit):
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "freegaussian_amd", "csrc", unit)
