"""The flow kernels (csrc/flow.hip) in isolation, row by row and pixel by pixel against ``oracle.raster_oracle`` on double
inputs (``gaussian_flow`` and autograd through it, ``camera_flow``, ``camera_flow_reprojection``); no restatement of its own.

``ops.gaussian_flow`` -- fg_flow_fwd, fg_flow_bwd -- with and without ``radii`` (positive, 0 and negative), N = 1000 rows
labelled by regime: ``means2d`` at the principal point / far off-screen / generic, depth 1e-3 / 1 / 1e3, velocity zero / not:
    every output (u_gs, u_cam) and every gradient (means2d, depths, vel), per row:
        |x_hip - x64|_2 / |A64|_2  <=  F * E32(regime, tensor)
    A = the absolute accumulation of the row's terms (``_accumulations``: the same sums with every term by magnitude),
    E32 from the same oracle in fp32 (CPU) over the regime's rows (tests/parity_common.py has the protocol);
    wherever ``radii <= 0``: u_gs, u_cam and all three gradients are exactly 0 -- rows whose inputs hold NaN included.
``ops.camera_flow`` and ``ops.reprojection_flow`` per pixel on a 37 x 19 map (703 pixels: not a multiple of 256), the same
rule; pixels of infinite depth give exactly 0.  ``ops.reprojection_flow`` takes the 3 x 4 motion M rounded to fp32, the float64
reference composes it in double from the fp32 poses: M's rounding is counted against the kernel (it is within the bound).

The recorded table is in profiles/loss_adam_flow_parity.md.

``PYTHONPATH=. python tests/test_flow_rows_gpu.py REPORT.jsonl`` turns the records of a run under FG_PARITY_REPORT into the table of
profiles/loss_adam_flow_parity.md.
"""
import functools
import math
import sys

import pytest
import torch

import parity_common as P
from freegaussian_amd import ops
from freegaussian_amd import flow as FL
from oracle import raster_oracle as O
from parity_common import need_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLOOR = 16 * 2.0**-24  # floor of the fp32 yardstick E32
# The bound is F * E32(regime, tensor).  Set from the MI355X run recorded in profiles/loss_adam_flow_parity.md: 4 x the
# worst recorded ratio (HIP distance) / E32 = 4 x 0.27, rounded up to a power of two.  None: record only.
F = 2.0

N = 1000
K = torch.tensor([[80.0, 0, 47.5], [0, 90.0, 31.0], [0, 0, 1]])
VELOC, OMEGA = torch.tensor([0.02, -0.01, 0.03]), torch.tensor([0.004, 0.01, -0.006])
POSITIONS, DEPTHS, MOTIONS = ("principal", "offscreen", "generic"), (1e-3, 1.0, 1e3), ("still", "moving")
REGIMES = tuple(f"{a}/Z={z:g}/{m}" for a in POSITIONS for z in DEPTHS for m in MOTIONS)
TENSORS = ("u_gs", "u_cam", "v_means2d", "v_depths", "v_vel")


@functools.lru_cache(maxsize=None)
def _inputs():
    """means2d [N,2], depths [N], vel [N,3], cotangents of u_gs and u_cam [N,2] (fp32), regime [N] (row i: i mod 18),
    radii [N] int32 (positive, 0 and negative)."""
    g = torch.Generator().manual_seed(21)
    regime = torch.arange(N) % len(REGIMES)
    pos, dep, mot = regime // 6, (regime // 2) % 3, regime % 2
    generic = torch.rand(N, 2, generator=g) * torch.tensor([96.0, 64.0])
    off = torch.where(torch.rand(N, 2, generator=g) < 0.5, -1.0, 1.0) * 10.0 ** (4.0 + torch.rand(N, 2, generator=g))
    m2 = torch.where((pos == 0)[:, None], torch.tensor([47.5, 31.0]).expand(N, 2), torch.where((pos == 1)[:, None], off, generic))
    depths = torch.tensor(DEPTHS)[dep] * (0.9 + 0.2 * torch.rand(N, generator=g))
    vel = torch.randn(N, 3, generator=g) * (mot == 1)[:, None]
    v_gs, v_cam = torch.randn(N, 2, generator=g), torch.randn(N, 2, generator=g)
    radii = torch.randint(-3, 7, (N,), generator=g, dtype=torch.int32)  # 40 % culled: -3 .. 0
    return m2.contiguous(), depths.contiguous(), vel.contiguous(), v_gs, v_cam, regime, radii


def _oracle(dtype):
    """-> name -> [N,k] of the oracle in ``dtype`` on the fp32 inputs: both outputs and, by autograd, the three gradients."""
    m2, depths, vel, v_gs, v_cam, _, _ = _inputs()
    x = [t.to(dtype).clone().requires_grad_(True) for t in (m2, depths, vel)]
    k = K.to(dtype)
    u_gs, u_cam = O.gaussian_flow(*x, k[0, 0], k[1, 1], k[0, 2], k[1, 2], VELOC.to(dtype), OMEGA.to(dtype))
    ((u_gs * v_gs.to(dtype)).sum() + (u_cam * v_cam.to(dtype)).sum()).backward()
    return dict(u_gs=u_gs.detach(), u_cam=u_cam.detach(), v_means2d=x[0].grad, v_depths=x[1].grad[:, None], v_vel=x[2].grad)


def _accumulations():
    """float64, name -> [N,k]: every output and gradient of a row with each of its terms by magnitude (the terms are those
    of u = A(mu) v / Z + B(mu) w and of its derivatives; B's entries are sums of one sign)."""
    m2, depths, vel, v_gs, v_cam, _, _ = (t.double() if t.is_floating_point() else t for t in _inputs())
    k, v, w = K.double(), VELOC.double().abs(), OMEGA.double().abs()
    fx, fy, cx, cy = k[0, 0], k[1, 1], k[0, 2], k[1, 2]
    A, B = O.camera_flow_AB(m2[:, 0], m2[:, 1], fx, fy, cx, cy)
    A, B, iz = A.abs(), B.abs(), 1.0 / depths.abs()
    xc, yc = (m2[:, 0] - cx).abs(), (m2[:, 1] - cy).abs()
    vg, vc, av = v_gs.abs(), v_cam.abs(), vel.abs()
    n = torch.einsum("nij,nj->ni", A, av)  # |fx vx| + |a02 vz|, |fy vy| + |a12 vz|
    mt = torch.einsum("nij,j->ni", A, v)
    acc = dict(u_gs=n * iz[:, None], u_cam=mt * iz[:, None] + torch.einsum("nij,j->ni", B, w))
    acc["v_vel"] = torch.stack([vg[:, 0] * fx * iz, vg[:, 1] * fy * iz, (vg[:, 0] * A[:, 0, 2] + vg[:, 1] * A[:, 1, 2]) * iz], -1)
    acc["v_depths"] = ((vg * n).sum(-1) + (vc * mt).sum(-1))[:, None] * (iz * iz)[:, None]
    gx = (vg[:, 0] * av[:, 2] + vc[:, 0] * v[2]) * iz + vc[:, 0] * (yc / fy * w[0] + 2 * xc / fx * w[1]) + vc[:, 1] * (yc / fx * w[1] + fy / fx * w[2])
    gy = (vg[:, 1] * av[:, 2] + vc[:, 1] * v[2]) * iz + vc[:, 0] * (xc / fy * w[0] + fx / fy * w[2]) + vc[:, 1] * (2 * yc / fy * w[0] + xc / fx * w[1])
    acc["v_means2d"] = torch.stack([gx, gy], -1)
    return acc


@functools.lru_cache(maxsize=None)
def _reference():
    """(float64 oracle, accumulations, E32[tensor][regime]); computed once."""
    r64, r32, acc = _oracle(torch.float64), _oracle(torch.float32), _accumulations()
    masks = P.masks_of_index(_inputs()[5], REGIMES)
    e32 = {t: P.yardstick(masks, P.distance(r32[t], r64[t], acc[t], rows=True), FLOOR) for t in TENSORS}
    return r64, acc, e32


@pytest.mark.parametrize("masked", [False, True], ids=["all-rows", "radii"])
def test_every_row_of_gaussian_flow(masked):
    m2, depths, vel, v_gs, v_cam, regime, radii = _inputs()
    r64, acc, e32 = _reference()
    live = radii > 0 if masked else torch.ones(N, dtype=torch.bool)
    if masked:
        assert int((radii < 0).sum()) > 100 and int((radii == 0).sum()) > 50 and int(live.sum()) > 400
        # every second culled row holds NaN in each of its inputs: nothing of it may leak
        poison = ~live & (torch.arange(N) % 2 == 0)
        m2, depths, vel = m2.clone(), depths.clone(), vel.clone()
        m2[poison], depths[poison], vel[poison] = float("nan"), float("nan"), float("nan")
    x = [t.detach().to(DEV).requires_grad_(True) for t in (m2, depths, vel)]
    u_gs, u_cam = ops.gaussian_flow(*x, K.to(DEV), VELOC.to(DEV), OMEGA.to(DEV), radii=radii.to(DEV) if masked else None)
    ((u_gs * v_gs.to(DEV)).sum() + (u_cam * v_cam.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    hip = dict(u_gs=u_gs.detach().cpu(), u_cam=u_cam.detach().cpu(), v_means2d=x[0].grad.cpu(), v_depths=x[1].grad.cpu()[:, None],
               v_vel=x[2].grad.cpu())  # fmt: skip
    failures = []
    for t in TENSORS:
        assert hip[t].shape == r64[t].shape, t
        culled = hip[t][~live]
        if not bool((culled == 0).all()):  # (NaN != 0)
            failures.append(f"{t}: {int((culled != 0).any(dim=1).sum())} culled rows are not exactly zero")
        masks = P.restrict(P.masks_of_index(regime, REGIMES), live)
        tag = "radii" if masked else "all-rows"
        P.check(f"{tag}|{t}|{{regime}}", masks, P.distance(hip[t], r64[t], acc[t], rows=True), e32[t], F, failures)
    # a still Gaussian has no flow of its own, whatever the rounding
    still = live & (regime % 2 == 0)
    assert bool((hip["u_gs"][still] == 0).all())
    assert not failures, "\n".join(failures)


W_MAP, H_MAP = 37, 19


@functools.lru_cache(maxsize=None)
def _maps():
    g = torch.Generator().manual_seed(22)
    Z = torch.rand(H_MAP, W_MAP, generator=g) * 4 + 0.3
    Z1 = Z * (0.9 + 0.2 * torch.rand(H_MAP, W_MAP, generator=g))
    Z[3, 5] = Z[0, 0] = Z[H_MAP - 1, W_MAP - 1] = float("inf")
    Z[7, 10:20] = float("inf")
    return Z, Z1


def _check_pixels(tag, f, f64, a64, f32, inf, failures):
    assert f.shape == (H_MAP, W_MAP, 2)
    assert bool((f[inf] == 0).all()), f"{tag}: a pixel of infinite depth is not exactly zero"
    flat = lambda t: t.reshape(-1, 2)  # noqa: E731
    finite = {"finite": ~inf.reshape(-1)}  # (the one regime of a map: its pixels of finite depth, row-major)
    e32 = P.yardstick(finite, P.distance(flat(f32), flat(f64), flat(a64), rows=True), FLOOR)
    P.check(f"{tag}|flow|{{regime}}", finite, P.distance(flat(f), flat(f64), flat(a64), rows=True), e32, F, failures)


def test_every_pixel_of_camera_flow():
    Z, _ = _maps()
    inf = torch.isinf(Z)
    ref = lambda dt: O.camera_flow(Z.to(dt), *(K.to(dt)[i, j] for i, j in ((0, 0), (1, 1), (0, 2), (1, 2))), VELOC.to(dt), OMEGA.to(dt))  # noqa: E731
    k = K.double()
    yy, xx = torch.meshgrid(torch.arange(H_MAP, dtype=torch.float64), torch.arange(W_MAP, dtype=torch.float64), indexing="ij")
    A, B = O.camera_flow_AB(xx, yy, k[0, 0], k[1, 1], k[0, 2], k[1, 2])
    acc = (A.abs() @ VELOC.double().abs()) / Z.double()[..., None] + B.abs() @ OMEGA.double().abs()
    f = ops.camera_flow(Z.to(DEV), K.to(DEV), VELOC.to(DEV), OMEGA.to(DEV)).cpu()
    failures = []
    _check_pixels("camera_flow", f, ref(torch.float64), acc, ref(torch.float32), inf, failures)
    assert not failures, "\n".join(failures)


def test_every_pixel_of_reprojection_flow():
    Z, Z1 = _maps()
    inf = torch.isinf(Z)
    c, s = math.cos(0.03), math.sin(0.03)
    c2w0 = torch.tensor([[1.0, 0, 0, 0.1], [0, 1.0, 0, -0.2], [0, 0, 1.0, 0.3]])
    c2w1 = torch.tensor([[c, 0, s, 0.15], [0, 1.0, 0, -0.18], [-s, 0, c, 0.32]])
    ref = lambda dt: O.camera_flow_reprojection(Z.to(dt)[..., None], Z1.to(dt)[..., None], c2w0, c2w1, K.to(dt))["sceneflow"]  # noqa: E731
    M = FL.reprojection_motion(c2w0, c2w1)  # [3,4] float64
    k = K.double()
    yy, xx = torch.meshgrid(torch.arange(H_MAP, dtype=torch.float64), torch.arange(W_MAP, dtype=torch.float64), indexing="ij")
    Zd = torch.where(inf, torch.ones_like(Z), Z).double()
    P = torch.stack([((xx - k[0, 2]) / k[0, 0] * Zd).abs(), ((yy - k[1, 2]) / k[1, 1] * Zd).abs(), Zd, torch.ones_like(Zd)], -1)
    q = P @ M.abs().t()  # [H,W,3]: |M X| with every term by magnitude
    acc = torch.stack([(k[0, 0] * q[..., 0] + k[0, 2] * q[..., 2]) / Z1.double() + xx,
                       (k[1, 1] * q[..., 1] + k[1, 2] * q[..., 2]) / Z1.double() + yy], -1)  # fmt: skip
    f = ops.reprojection_flow(Z.to(DEV), Z1.to(DEV), K.to(DEV), M.float().to(DEV), sign=-1.0).cpu()
    failures = []
    _check_pixels("reprojection_flow", f, ref(torch.float64), acc, ref(torch.float32), inf, failures)
    assert not failures, "\n".join(failures)


def _report(path):
    """Markdown of a run's records (FG_PARITY_REPORT): per call and tensor x regime, the HIP ratio and (E32)."""
    ratio, e32 = P.read_records(path, "test_flow_rows_gpu")
    worst = max(ratio, key=ratio.get)
    print(f"Flow: worst ratio {ratio[worst]:.2f} at {' | '.join(worst)}; {len(ratio)} cells.\n")
    print("| regime | " + " | ".join(f"{tag} {t}" for tag in ("all-rows", "radii") for t in TENSORS) + " |\n|---|" + "---|" * (2 * len(TENSORS)))
    for name in REGIMES:
        cells = [f"{ratio[(tag, t, name)]:.2f} ({e32[(tag, t, name)]:.1e})" if (tag, t, name) in ratio else ""
                 for tag in ("all-rows", "radii") for t in TENSORS]  # fmt: skip
        print(f"| {name} | " + " | ".join(cells) + " |")
    print("\n| map | ratio (E32) |\n|---|---|")
    for tag in ("camera_flow", "reprojection_flow"):
        print(f"| {tag} | {ratio[(tag, 'flow', 'finite')]:.2f} ({e32[(tag, 'flow', 'finite')]:.1e}) |")


if __name__ == "__main__":
    _report(sys.argv[1])
