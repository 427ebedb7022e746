#!/usr/bin/env python3
"""What ``ops.optical_flow`` / ``fg_optflow`` costs: the whole two-direction call with the defaults at 480 x 270, 960 x 540 and
1920 x 1080, the product build (B staged through LDS per iteration) against the build that samples B by direct loads, and --
for information only -- a torch-ops statement of the same algorithm (``unfold`` + ``grid_sample``) on the same GPU.

    make -C freegaussian_amd/csrc optflow-direct        # the second side: libfgraster_optflow_direct.so
    python scripts/optical_flow_bench.py [--out DIR] [--sizes 270x480,540x960,1080x1920] [--no-torch]
    python scripts/optical_flow_bench.py --resources    # registers, LDS and occupancy of both builds' kernels (no GPU)

Protocol (scripts/fused_bench_common.py): the two builds alternate call by call in one process, 10 warm-up and 50 timed calls
between device events, median (p10 .. p90); before timing, both builds run once and their outputs must be equal bit for bit
(the same taps in the same order: staging changes where a tap is read from, not what is added).  The torch statement is timed
alone (3 warm-up, 10 timed calls).  Writes DIR/optical_flow_bench.json and prints the tables of profiles/optical_flow.md.
Inputs: a seeded sum of sinusoids and the same texture moved by a smooth flow of up to 6 px (scaled with the image)."""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fused_bench_common as C  # noqa: E402

DIRECT_LIB = os.path.join(ROOT, "freegaussian_amd", "libfgraster_optflow_direct.so")
ITERS, RADIUS, MIN_EIG, CONSISTENCY = 4, 3, 1e-5, 1.0


def frames(H, W, dev):
    """Two grey frames: 48 sinusoids (0.02 .. 0.18 cycles per pixel at 480 x 270, scaled with the width), the second one
    sampled at x + a smooth displacement of up to 6 px x W / 480."""
    g = torch.Generator().manual_seed(H * 10000 + W)
    s = 480.0 / W
    f = (torch.rand(48, generator=g) * 0.16 + 0.02) * s
    th, ph = torch.rand(48, generator=g) * 2 * math.pi, torch.rand(48, generator=g) * 2 * math.pi
    kx, ky, amp = (2 * math.pi * f * th.cos()).to(dev), (2 * math.pi * f * th.sin()).to(dev), (1 / f / (6 * ((1 / f) ** 2).sum().div(2).sqrt())).to(dev)
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")

    def tex(x, y):
        out = torch.full_like(x, 0.5)
        for k in range(48):
            out += amp[k] * torch.sin(kx[k] * x + ky[k] * y + ph[k].to(dev))
        return out

    mag = 6.0 / s
    dx, dy = mag * torch.sin(2 * math.pi * y / H), mag * 0.5 * torch.cos(2 * math.pi * x / W)
    return tex(x, y).contiguous(), tex(x + dx, y + dy).contiguous()


def raw_call(lib, a, b, levels, flow, valid, ws):
    H, W = a.shape
    rc = lib.fg_optflow(H, W, 1, 1, a.data_ptr(), b.data_ptr(), levels, ITERS, RADIUS, MIN_EIG, 1, CONSISTENCY, None, flow.data_ptr(),
                        valid.data_ptr(), ws.data_ptr(), ws.numel(), torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))  # fmt: skip
    if rc != 0:
        raise RuntimeError(f"fg_optflow: {rc}")


# ---- the torch-ops statement (information only; not in the product)


def _sample(img, px, py):
    """img [h,w] bilinearly at the real (px, py) [h,w], clamped to the image."""
    h, w = img.shape
    gx = px.clamp(0, w - 1) * (2.0 / max(w - 1, 1)) - 1.0
    gy = py.clamp(0, h - 1) * (2.0 / max(h - 1, 1)) - 1.0
    return F.grid_sample(img[None, None], torch.stack([gx, gy], -1)[None], mode="bilinear", padding_mode="border", align_corners=True)[0, 0]


def _windows(img, r):
    """[h,w] -> [(2r+1)^2, h, w]: the window of every pixel, coordinates clamped (replicate padding)."""
    h, w = img.shape
    return F.unfold(F.pad(img[None, None], (r, r, r, r), mode="replicate"), 2 * r + 1).view(-1, h, w)


def torch_direction(pa, pb, iters, r):
    u = None
    for A, B in zip(reversed(pa), reversed(pb)):
        h, w = A.shape
        y, x = torch.meshgrid(torch.arange(h, device=A.device, dtype=torch.float32), torch.arange(w, device=A.device, dtype=torch.float32), indexing="ij")
        if u is None:
            u = torch.zeros(2, h, w, device=A.device)
        else:
            u = 2.0 * torch.stack([_sample(u[c], x / 2, y / 2) for c in (0, 1)])
        P = F.pad(A[None, None], (1, 1, 1, 1), mode="replicate")[0, 0]
        ix, iy = (P[1:-1, 2:] - P[1:-1, :-2]) * 0.5, (P[2:, 1:-1] - P[:-2, 1:-1]) * 0.5
        wa, wx, wy = _windows(A, r), _windows(ix, r), _windows(iy, r)
        cx, cy = _windows(x, r), _windows(y, r)  # the clamped window coordinates
        gxx, gxy, gyy = (wx * wx).sum(0) + 1e-6, (wx * wy).sum(0), (wy * wy).sum(0) + 1e-6
        det = gxx * gyy - gxy * gxy
        for _ in range(iters):
            it = torch.stack([_sample(B, cx[q] + u[0], cy[q] + u[1]) for q in range(cx.shape[0])]) - wa
            bx, by = (it * wx).sum(0), (it * wy).sum(0)
            u = torch.stack([u[0] - (gyy * bx - gxy * by) / det, u[1] - (gxx * by - gxy * bx) / det])
    return u, (gxx, gxy, gyy)


def torch_statement(a, b, levels, iters=ITERS, r=RADIUS):
    k = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], device=a.device) / 16
    k2 = (k[:, None] * k[None, :])[None, None]

    def pyramid(img):
        out = [img]
        for _ in range(levels - 1):
            out.append(F.conv2d(F.pad(out[-1][None, None], (2, 2, 2, 2), mode="replicate"), k2, stride=2)[0, 0])
        return out

    pa, pb = pyramid(a), pyramid(b)
    u, (gxx, gxy, gyy) = torch_direction(pa, pb, iters, r)
    v, _ = torch_direction(pb, pa, iters, r)
    H, W = a.shape
    y, x = torch.meshgrid(torch.arange(H, device=a.device, dtype=torch.float32), torch.arange(W, device=a.device, dtype=torch.float32), indexing="ij")
    px, py = x + u[0], y + u[1]
    eig = ((gxx + gyy) - ((gxx - gyy) ** 2 + 4 * gxy * gxy).sqrt()) * (0.5 / (2 * r + 1) ** 2)
    res = torch.stack([u[c] + _sample(v[c], px, py) for c in (0, 1)])
    valid = (eig >= MIN_EIG) & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1) & (res.norm(dim=0) <= CONSISTENCY)
    return u.permute(1, 2, 0), valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "optical_flow"))
    ap.add_argument("--sizes", default="270x480,540x960,1080x1920")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--resources", action="store_true", help="only the kernels' resource table (needs hipcc, no GPU)")
    args = ap.parse_args()
    if args.resources:
        return resources()
    from freegaussian_amd import _lib, ops

    dev = torch.device("cuda")
    staged = _lib.load()
    direct = ctypes.CDLL(DIRECT_LIB)
    direct.fg_optflow.restype, direct.fg_optflow.argtypes = _lib.SIGNATURES["fg_optflow"]
    os.makedirs(args.out, exist_ok=True)
    results = []
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        a, b = frames(H, W, dev)
        levels = ops.optical_flow_default_levels(H, W)
        ws_bytes = int(staged.fg_optflow_workspace_bytes(H, W, levels, 1))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = {k: (torch.empty(H, W, 2, device=dev), torch.empty(H, W, dtype=torch.uint8, device=dev)) for k in ("direct", "staged")}
        raw_call(direct, a, b, levels, *out["direct"], ws)
        raw_call(staged, a, b, levels, *out["staged"], ws)
        torch.cuda.synchronize()
        equal = bool(torch.equal(out["direct"][0], out["staged"][0]) and torch.equal(out["direct"][1], out["staged"][1]))
        q = C.alternate({"direct": lambda: raw_call(direct, a, b, levels, *out["direct"], ws),
                         "staged": lambda: raw_call(staged, a, b, levels, *out["staged"], ws)})  # fmt: skip
        q["op"] = C.alternate({"op": lambda: ops.optical_flow(a, b)})["op"]  # with the allocations of the Python layer
        row = {"H": H, "W": W, "levels": levels, "launches": 2 * levels + 2 * levels + 1, "workspace_bytes": ws_bytes, "equal": equal,
               "valid_share": float(out["staged"][1].float().mean()), **q, "verdict": C.verdict(q["staged"], q["direct"])}  # fmt: skip
        if not args.no_torch:
            tu, tv = torch_statement(a, b, levels)
            both = tv & out["staged"][1].bool()
            row["torch_max_diff_px"] = float((tu - out["staged"][0])[both].abs().max())
            row["torch"] = C.alternate({"torch": lambda: torch_statement(a, b, levels)}, warm=3, timed=10)["torch"]
        results.append(row)
        print(json.dumps(row), flush=True)
        del ws, out
    json.dump(results, open(os.path.join(args.out, "optical_flow_bench.json"), "w"), indent=1)
    print("\n| size | levels | launches | workspace MiB | direct ms | staged ms | staged against direct | same bits | ops.optical_flow ms | torch ops ms |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        print(f"| {r['W']} x {r['H']} | {r['levels']} | {r['launches']} | {r['workspace_bytes'] / 2**20:.1f} | {C.cell(r['direct'])} | "
              f"{C.cell(r['staged'])} | {r['verdict']} | {r['equal']} | {C.cell(r['op'])} | {C.cell(r['torch']) if 'torch' in r else '-'} |")


def resources():
    print("\n| kernel | build | VGPRs | SGPRs | scratch | occupancy (waves/SIMD) | LDS bytes |\n|---|---|---|---|---|---|---|")
    for build, extra in (("staged", ()), ("direct", ("-DFG_OPTFLOW_STAGED=0",))):
        for k in C.kernel_resources(C.csrc("optflow.hip"), extra):
            print(f"| {k['kernel']} | {build} | {k.get('VGPRs')} | {k.get('TotalSGPRs')} | {k.get('ScratchSize')} | {k.get('Occupancy')} | {k.get('LDS')} |")


if __name__ == "__main__":
    main()
