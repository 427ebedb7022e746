"""Float64 numpy restatement of the bilateral-grid slice of a whole image (freegaussian_amd/bilagrid.py apply_to_render:
grid_sample with mode="bilinear", align_corners=True, padding_mode="border", then the 3 x 4 multiply), its two gradients,
and the inputs the fused-slice tests share.  A helper, not a test file.

The three luma weights are the fp32 values taken as doubles: a white pixel then clamps in float64 as it does in fp32
(the sum is 1.0000000075).  Vectorised over pixels; a loop version of the same formulas agrees with torch's float64
autograd of apply_to_render to 3e-7 (the weights' own rounding).

    case(...), forward, backward, clear_of_knife_edges     what tests/test_bilagrid_fused_*.py use: the array-wide bar

PER ELEMENT (tests/test_bilagrid_elements_*.py), by the protocol of tests/parity_common.py:

    restate(grid, rgb, v_out, dtype)   out, v_rgb, v_grid in float64 or float32 (plain numpy, CPU) -- beside each its
                           ABSOLUTE ACCUMULATION A, every term by magnitude:
                               out[p, j]          sum_k (sum_corners |w| |g_k|) |(r, g, b, 1)_k|
                               v_rgb[p, c]        sum_j (sum_corners |w| |g|) |v_j|  +  (GL-1) |luma_c| sum_k (sum_corners |w_y w_x| |g_k|) |u_k|
                               v_grid[k, z, y, x] sum over pixels |w| |u_k|        (u_k = v_out[k / 4] (r, g, b, 1)[k % 4])
                           The cell of a pixel is the integer map of csrc/bilagrid.hip (cell_of below), the fraction
                           t = p (n-1) / (S-1) - cell from ONE division: t is exactly 0 on a node and exactly 1 on the last
                           pixel, in either dtype, so which nodes a pixel reaches does not depend on rounding.  The
                           float64 variant takes the fp32 inputs exactly.
    regime_case(...)       inputs, both restatements, the regime masks of pixels and grid nodes, E32 per (array, regime);
                           a node no pixel reaches has A = 0 and must be exactly 0.0
    MUTANTS                wrong restatements (float64, CPU only: they prove that the bound has teeth)
"""
import functools
from typing import Optional

import numpy as np

import parity_common as P

LUMA = np.array([np.float32(0.299), np.float32(0.587), np.float32(0.114)], dtype=np.float64)


def _axis(f, n):
    """Clamped coordinate -> (i0, i1, t) of the border-clamped linear interpolation over n nodes."""
    f = np.clip(f, 0.0, n - 1.0)
    i0 = np.minimum(np.floor(f).astype(np.int64), n - 1)
    return i0, np.minimum(i0 + 1, n - 1), f - i0


def guidance(rgb, GL):
    """The unclamped level coordinate fz [H,W] in float64."""
    return (np.asarray(rgb, dtype=np.float64) @ LUMA) * (GL - 1)


def _corners(grid, rgb):
    _, GL, GY, GX = grid.shape
    H, W, _ = rgb.shape
    x0, x1, tx = _axis(np.arange(W, dtype=np.float64) / (W - 1) * (GX - 1), GX)
    y0, y1, ty = _axis(np.arange(H, dtype=np.float64) / (H - 1) * (GY - 1), GY)
    fz = guidance(rgb, GL)
    z0, z1, tz = _axis(fz, GL)
    inside = (fz > 0) & (fz < GL - 1)
    xs = [(np.broadcast_to(x0[None, :], (H, W)), np.broadcast_to(1 - tx[None, :], (H, W))), (np.broadcast_to(x1[None, :], (H, W)), np.broadcast_to(tx[None, :], (H, W)))]
    ys = [(np.broadcast_to(y0[:, None], (H, W)), np.broadcast_to(1 - ty[:, None], (H, W))), (np.broadcast_to(y1[:, None], (H, W)), np.broadcast_to(ty[:, None], (H, W)))]
    zs = [(z0, 1 - tz, -1.0), (z1, tz, 1.0)]
    return xs, ys, zs, inside


def forward(grid, rgb):
    """grid [12,GL,GY,GX], rgb [H,W,3] -> out [H,W,3], all float64."""
    grid, rgb = np.asarray(grid, dtype=np.float64), np.asarray(rgb, dtype=np.float64)
    xs, ys, zs, _ = _corners(grid, rgb)
    A = np.zeros((12,) + rgb.shape[:2])
    for zi, wz, _ in zs:
        for yi, wy in ys:
            for xi, wx in xs:
                A += (wz * wy * wx)[None] * grid[:, zi, yi, xi]
    A = A.reshape(3, 4, *rgb.shape[:2])
    return np.einsum("jchw,hwc->hwj", A[:, :3], rgb) + A[:, 3].transpose(1, 2, 0)


def backward(grid, rgb, v_out):
    """-> (v_rgb [H,W,3], v_grid [12,GL,GY,GX]) of sum(out * v_out), float64."""
    grid, rgb, v_out = (np.asarray(a, dtype=np.float64) for a in (grid, rgb, v_out))
    GL = grid.shape[1]
    H, W, _ = rgb.shape
    xs, ys, zs, inside = _corners(grid, rgb)
    rgb1 = np.concatenate([rgb, np.ones((H, W, 1))], axis=-1)
    u = (v_out[:, :, :, None] * rgb1[:, :, None, :]).reshape(H, W, 12).transpose(2, 0, 1)  # u[k] = v_out[k / 4] (r,g,b,1)[k % 4]
    A = np.zeros((12, H, W))
    dA = np.zeros((12, H, W))
    v_grid = np.zeros_like(grid)
    for zi, wz, sign in zs:
        for yi, wy in ys:
            for xi, wx in xs:
                g = grid[:, zi, yi, xi]
                A += (wz * wy * wx)[None] * g
                dA += (sign * wy * wx)[None] * g
                for k in range(12):
                    np.add.at(v_grid[k], (zi, yi, xi), wz * wy * wx * u[k])
    A = A.reshape(3, 4, H, W)
    v_rgb = np.einsum("jchw,hwj->hwc", A[:, :3], v_out)
    slope = np.where(inside, (dA * u).sum(axis=0), 0.0) * (GL - 1)
    return v_rgb + slope[:, :, None] * LUMA[None, None, :], v_grid


def node_distance(rgb, GL):
    """Distance of every pixel's float64 fz to the nearest level node 0 .. GL-1."""
    fz = guidance(rgb, GL)
    return np.abs(fz - np.clip(np.round(fz), 0, GL - 1))


def is_black(rgb):
    return (np.asarray(rgb) == 0).all(axis=-1)


def is_white(rgb):
    return (np.asarray(rgb) == 1).all(axis=-1)


def clear_of_knife_edges(rgb, GL, margin=1e-3):
    """Every pixel is exactly black, exactly white, or at least `margin` away (in fz) from every level node: on a node the
    slice takes either neighbouring cell's slope depending on the last bit of the luma, at 0 / GL-1 either the border
    rule or the slope."""
    return bool((is_black(rgb) | is_white(rgb) | (node_distance(rgb, GL) >= margin)).all())


@functools.lru_cache(maxsize=None)
def case(H, W, GX, GY, GL, num=1, cam=0, seed=0):
    """Seeded inputs, repaired before any path sees them, and their float64 results (computed once per shape, shared,
    never modified: the arrays are read-only).  Grids: identity + 0.3 x normal noise, for every camera; rgb: uniform in
    [0.02, 0.98], any pixel within 1e-3 (in fz) of a level node scaled by 0.97 until it is not; then, on purpose, exactly
    black pixels, exactly white ones, and out-of-range ones (luma <= -0.05 and >= 1.05); cotangents: normal."""
    rng = np.random.default_rng(1000 * seed + 7 * H + W)
    eye = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]).reshape(1, 12, 1, 1, 1)
    grids = (eye + 0.3 * rng.standard_normal((num, 12, GL, GY, GX))).astype(np.float32)
    rgb = rng.uniform(0.02, 0.98, (H, W, 3)).astype(np.float32)
    flat = rgb.reshape(-1, 3)
    n = flat.shape[0]
    placed = rng.permutation(n)[: max(8, n // 16) // 4 * 4].reshape(4, -1)
    flat[placed[0]] = 0.0
    flat[placed[1]] = 1.0
    flat[placed[2]] = rng.uniform(-0.4, -0.05, (placed.shape[1], 1)).astype(np.float32)  # grey, luma = the value (weights sum to 1)
    flat[placed[3]] = rng.uniform(1.05, 1.4, (placed.shape[1], 1)).astype(np.float32)
    for _ in range(200):
        bad = ~(is_black(flat) | is_white(flat)) & (node_distance(flat, GL) < 1e-3)
        if not bad.any():
            break
        flat[bad] = (flat[bad] * np.float32(0.97)).astype(np.float32)
    assert clear_of_knife_edges(rgb, GL)
    luma = guidance(rgb, 2)
    assert is_black(rgb).sum() >= 2 and is_white(rgb).sum() >= 2 and (luma <= -0.05).sum() >= 2 and (luma >= 1.05).sum() >= 2
    v_out = rng.standard_normal((H, W, 3)).astype(np.float32)
    out = forward(grids[cam], rgb)
    v_rgb, v_grid = backward(grids[cam], rgb, v_out)
    res = {"grids": grids, "rgb": rgb, "v_out": v_out, "out": out, "v_rgb": v_rgb, "v_grid": v_grid, "cam": cam}
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# per element: the integer maps, the restatement in either dtype with its absolute accumulations, the mutants

FLOOR = 16 * 2.0**-24  # floor of the fp32 yardstick E32 (loss_restatement.FLOOR)
SEG, CHUNK = 256, 1024  # pixels of a row per workgroup of the slice; pixels of a cell per workgroup of the gather

# The GPU bound is F * E32(regime, array).  Set from the MI355X run recorded in profiles/bilagrid_parity.md: 4 x the worst
# recorded ratio (HIP distance) / E32, rounded up to a power of two = 4 x 1.02 -> 8; capped by the host test's mutant
# assertion (F <= 9.7: the gather with the next row's ty on the 700 x 3 image).  None: record only (how the run F was set
# from was made).
F: Optional[float] = 8.0

PIXEL_REGIMES = ("interior", "black", "white", "below_range", "above_range", "near_node", "on_x_node", "on_y_node", "last_col",
                 "last_row", "segment_start", "coherent")  # fmt: skip
NODE_REGIMES = ("corner", "edge", "interior", "sparse", "multi_chunk", "unreached")
ARRAYS = ("out", "v_rgb", "v_grid")
MUTANTS = ("align_corners_false", "luma_weights_permuted", "slope_not_zeroed_outside_range", "slope_without_GL_minus_1",
           "last_column_dropped_from_the_gather", "last_chunk_pixel_dropped", "second_chunk_dropped", "neighbour_row_ty",
           "x_node_shifted_in_later_segments", "skipped_level_keeps_previous_sums")  # fmt: skip
# (H, W, GX, GY, GL, cameras, camera, input): tests/test_bilagrid_elements_gpu.py says what each one reaches
SHAPES = ((3, 523, 7, 2, 3, 1, 0, "noise"), (5, 257, 9, 3, 3, 1, 0, "noise"), (4, 769, 3, 2, 2, 1, 0, "noise"),
          (700, 3, 2, 2, 2, 1, 0, "noise"), (7, 130, 64, 64, 16, 1, 0, "noise"), (5, 300, 64, 4, 16, 1, 0, "noise"),
          (2, 2, 2, 2, 2, 1, 0, "noise"), (9, 49, 5, 3, 2, 1, 0, "noise"), (24, 600, 16, 3, 8, 1, 0, "coherent"),
          (37, 53, 5, 4, 3, 3, 1, "existing"))  # fmt: skip


def first_px(c, S, n):
    """The first pixel of cell c along an axis of S pixels and n nodes: ceil(c (S-1) / (n-1))."""
    return (c * (S - 1) + n - 2) // (n - 1)


def cell_of(p, S, n):
    """min(floor(p (n-1) / (S-1)), n-2), in integers: the last pixel sits on node n-1, in cell n-2 with t = 1."""
    return np.minimum(p * (n - 1) // (S - 1), n - 2)


def end_px(c, S, n):
    """One past the last pixel of cell c."""
    return np.where(c == n - 2, S, first_px(c + 1, S, n))


def segments(W, GX):
    """The slice's row segments: [(x0, x1, cx_lo, x nodes in LDS)]."""
    out = []
    for x0 in range(0, W, SEG):
        x1 = min(x0 + SEG, W)
        lo = int(cell_of(x0, W, GX))
        out.append((x0, x1, lo, int(cell_of(x1 - 1, W, GX)) - lo + 2))
    return out


def gather_layout(H, W, GX, GY):
    """Where the gather holds every pixel: its cell [H,W] (cy (GX-1) + cx), its row-major index inside the cell's rectangle,
    the chunk (index / 1024) and the wave (lane = index % 256, wave = lane >> 6); npx [GY-1,GX-1] pixels per cell."""
    px, py = np.arange(W), np.arange(H)
    cx, cy = cell_of(px, W, GX), cell_of(py, H, GY)
    xc, yc = np.arange(GX - 1), np.arange(GY - 1)
    xa, ya = first_px(xc, W, GX), first_px(yc, H, GY)
    nx, ny = end_px(xc, W, GX) - xa, end_px(yc, H, GY) - ya
    index = (py - ya[cy])[:, None] * nx[cx][None, :] + (px - xa[cx])[None, :]
    return dict(cell=cy[:, None] * (GX - 1) + cx[None, :], index=index, chunk=index // CHUNK, wave=(index % 256) >> 6,
                npx=ny[:, None] * nx[None, :], nx=nx, ny=ny)  # fmt: skip


def _cell_frac(S, n, T, align_corners=True, shift=0):
    """Along one axis: the cell [S] and the fraction t [S] in dtype T of pixel p + shift measured from pixel p's cell."""
    p = np.arange(S)
    if not align_corners:  # (a mutant) pixel centres over the whole extent, border-clamped
        f = np.clip((p + 0.5) * n / S - 0.5, 0.0, n - 1.0)
        c = np.minimum(np.floor(f).astype(np.int64), n - 2)
        return c, (f - c).astype(T)
    c = cell_of(p, S, n)
    return c, ((p + shift) * (n - 1)).astype(T) / T(S - 1) - c.astype(T)


def restate(grid, rgb, v_out, dtype=np.float64, mutant=None):
    """grid [12,GL,GY,GX], rgb, v_out [H,W,3] -> dict: out, v_rgb [H,W,3], v_grid [12,GL,GY,GX] and out_acc, v_rgb_acc,
    v_grid_acc, every operation in ``dtype``; in float64 also reach, reach_big [GL,GY,GX]: the pixels (of cells of more
    than 1024 pixels) that reach a node with a weight above zero.  ``mutant``: one of MUTANTS, float64 only (the skipped-level
    mutant also returns got_stale [12,GL,GY,GX]: the sums that received a stale sum other than zero)."""
    T = np.dtype(dtype).type
    assert mutant is None or (mutant in MUTANTS and T is np.float64)
    grid, rgb, v_out = (np.asarray(a).astype(T) for a in (grid, rgb, v_out))
    _, GL, GY, GX = grid.shape
    H, W, _ = rgb.shape
    lw = LUMA.astype(T)
    if mutant == "luma_weights_permuted":
        lw = lw[[1, 2, 0]]
    ac = mutant != "align_corners_false"
    cx, tx = _cell_frac(W, GX, T, ac)
    cy, ty = _cell_frac(H, GY, T, ac)
    ty_gather = _cell_frac(H, GY, T, shift=1)[1] if mutant == "neighbour_row_ty" else ty
    x_read = cx
    if mutant == "x_node_shifted_in_later_segments":
        x_read = cx.copy()
        for x0, x1, lo, _ in segments(W, GX)[1:]:
            x_read[x0:x1] -= lo
    top = T(GL - 1)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    fz = (lw[0] * r + lw[1] * g + lw[2] * b) * top
    inside = (fz > 0) & (fz < top)
    if mutant == "slope_not_zeroed_outside_range":
        inside = np.ones_like(inside)
    fc = np.clip(fz, T(0), top)
    z0 = np.minimum(np.floor(fc).astype(np.int64), GL - 2)
    tz = fc - z0.astype(T)
    rgb1 = [r, g, b, np.ones((H, W), T)]
    u = np.stack([v_out[..., k // 4] * rgb1[k % 4] for k in range(12)])  # [12,H,W]
    lay = gather_layout(H, W, GX, GY)
    keep = np.ones((H, W), bool)  # pixels the gather takes
    if mutant == "last_column_dropped_from_the_gather":
        keep[:, W - 1] = False
    elif mutant == "last_chunk_pixel_dropped":
        keep = lay["index"] != CHUNK - 1
    elif mutant == "second_chunk_dropped":
        keep = lay["chunk"] != 1
    big = (lay["npx"] > CHUNK).ravel()[lay["cell"]]
    one = T(1)
    A, A_abs, dA, dA_abs = (np.zeros((12, H, W), T) for _ in range(4))
    nodes = GL * GY * GX
    vg, vg_abs = np.zeros((nodes, 12), T), np.zeros((nodes, 12), T)
    reach, reach_big = np.zeros(nodes, np.int64), np.zeros(nodes, np.int64)
    skip = mutant == "skipped_level_keeps_previous_sums"
    if skip:  # the gather's own route: sums per (cell, chunk, wave) and level, a skipped level reports what its buffer held
        gid, group = np.unique((lay["cell"] * (lay["chunk"].max() + 1) + lay["chunk"]) * 4 + lay["wave"], return_inverse=True)
        group = group.reshape(H, W)
        part = np.zeros((len(gid), GL, 4, 12))
        touched = np.zeros((len(gid), GL), bool)
        touched[group, z0] = True
        touched[group, z0 + 1] = True
    for dz in (0, 1):
        wz, sign = (tz, one) if dz else (one - tz, -one)
        for dy in (0, 1):
            for dx in (0, 1):
                wyx = ((ty if dy else one - ty)[:, None] * (tx if dx else one - tx)[None, :]).astype(T)
                gk = grid[:, z0 + dz, (cy + dy)[:, None], (x_read + dx)[None, :]]  # [12,H,W]
                w = wz * wyx
                A += w[None] * gk
                A_abs += np.abs(w)[None] * np.abs(gk)
                dA += (sign * wyx)[None] * gk
                dA_abs += np.abs(wyx)[None] * np.abs(gk)
                wg = np.where(keep, wz * ((ty_gather if dy else one - ty_gather)[:, None] * (tx if dx else one - tx)[None, :]), T(0)).astype(T)
                idx = (((z0 + dz) * GY + (cy + dy)[:, None]) * GX + (cx + dx)[None, :]).ravel()
                val = (wg[None] * u).reshape(12, -1).T
                if skip:
                    np.add.at(part, (group.ravel(), (z0 + dz).ravel(), 2 * dy + dx), val)
                else:
                    np.add.at(vg, idx, val)
                np.add.at(vg_abs, idx, np.abs(val))
                np.add.at(reach, idx, (wg > 0).ravel())
                np.add.at(reach_big, idx, ((wg > 0) & big).ravel())
    if skip:
        got_stale = np.zeros((nodes, 12), np.int64)  # how many stale sums other than zero an element received
        cell = gid // 4 // (lay["chunk"].max() + 1)
        gy, gx = cell // (GX - 1), cell % (GX - 1)
        for z in range(GL):
            stale = part[:, z - 2] if z >= 2 else np.zeros_like(part[:, 0])
            part[:, z] = np.where(touched[:, z, None, None], part[:, z], stale)
            for c in range(4):
                at = (z * GY + gy + c // 2) * GX + gx + c % 2
                np.add.at(vg, at, part[:, z, c])
                np.add.at(got_stale, at, ~touched[:, z, None] & (stale[:, c] != 0))
    out = np.stack([A[4 * j] * r + A[4 * j + 1] * g + A[4 * j + 2] * b + A[4 * j + 3] for j in range(3)], axis=-1)
    out_acc = np.stack([A_abs[4 * j] * np.abs(r) + A_abs[4 * j + 1] * np.abs(g) + A_abs[4 * j + 2] * np.abs(b) + A_abs[4 * j + 3]
                        for j in range(3)], axis=-1)  # fmt: skip
    scale = one if mutant == "slope_without_GL_minus_1" else top
    slope = np.where(inside, (dA * u).sum(axis=0, dtype=T), T(0)) * scale
    slope_abs = np.where(inside, (dA_abs * np.abs(u)).sum(axis=0, dtype=T), T(0)) * scale
    v = [v_out[..., j] for j in range(3)]
    v_rgb = np.stack([A[c] * v[0] + A[4 + c] * v[1] + A[8 + c] * v[2] + lw[c] * slope for c in range(3)], axis=-1)
    v_rgb_acc = np.stack([A_abs[c] * np.abs(v[0]) + A_abs[4 + c] * np.abs(v[1]) + A_abs[8 + c] * np.abs(v[2]) + lw[c] * slope_abs
                          for c in range(3)], axis=-1)  # fmt: skip
    res = dict(out=out, out_acc=out_acc, v_rgb=v_rgb, v_rgb_acc=v_rgb_acc, v_grid=vg.T.reshape(12, GL, GY, GX).copy(),
               v_grid_acc=vg_abs.T.reshape(12, GL, GY, GX).copy())  # fmt: skip
    assert all(a.dtype == T for a in res.values())
    if T is np.float64:
        res["reach"], res["reach_big"] = reach.reshape(GL, GY, GX), reach_big.reshape(GL, GY, GX)
    if skip:
        res["got_stale"] = got_stale.T.reshape(12, GL, GY, GX) > 0
    return res


# ---------------------------------------------------------------------------------------------------------------------
# inputs and regimes


def _repair(flat, GL):
    for _ in range(400):
        bad = ~(is_black(flat) | is_white(flat)) & (node_distance(flat, GL) < 1e-3)
        if not bad.any():
            return
        flat[bad] = (flat[bad] * np.float32(0.97)).astype(np.float32)
    raise AssertionError("pixels on a level node remain")


def _inputs(H, W, GX, GY, GL, num, kind, seed):
    """-> grids, rgb, v_out (fp32), placed [H,W] bool: the pixels put 1.5e-3 from a level node on purpose.
    noise: as ``case`` (uniform rgb, then black, white and out-of-range pixels), plus grey pixels 1.5e-3 either side of a
    level node; an image of fewer than 40 pixels is noise alone.  coherent: luma is a ramp across the image (0.1 .. 0.9
    left to right, + 0.04 top to bottom) with 0.3 % noise, the channels at fixed offsets (+0.05, -0.02, -0.03) from it."""
    rng = np.random.default_rng(77 + 1000 * seed + 7 * H + W + 31 * GX)
    eye = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]).reshape(1, 12, 1, 1, 1)
    grids = (eye + 0.3 * rng.standard_normal((num, 12, GL, GY, GX))).astype(np.float32)
    placed = np.zeros(H * W, bool)
    if kind == "coherent":
        ramp = np.linspace(0.1, 0.9, W)[None, :, None] + np.linspace(0.0, 0.04, H)[:, None, None]
        rgb = (ramp + np.array([0.05, -0.02, -0.03]) + 0.003 * rng.standard_normal((H, W, 3))).astype(np.float32)
        _repair(rgb.reshape(-1, 3), GL)
    else:
        rgb = rng.uniform(0.02, 0.98, (H, W, 3)).astype(np.float32)
        flat = rgb.reshape(-1, 3)
        n = flat.shape[0]
        _repair(flat, GL)
        if n >= 40:
            m = max(2, n // 64)
            at = rng.permutation(n)[: 5 * m].reshape(5, m)
            flat[at[0]] = 0.0
            flat[at[1]] = 1.0
            flat[at[2]] = rng.uniform(-0.4, -0.05, (m, 1)).astype(np.float32)  # grey, luma = the value (weights sum to 1)
            flat[at[3]] = rng.uniform(1.05, 1.4, (m, 1)).astype(np.float32)
            node = rng.integers(0, GL, m)
            side = np.where(node == 0, 1.0, np.where(node == GL - 1, -1.0, rng.choice([-1.0, 1.0], m)))
            flat[at[4]] = ((node + 1.5e-3 * side) / (GL - 1))[:, None].astype(np.float32)
            placed[at[4]] = True
    assert clear_of_knife_edges(rgb, GL)
    v_out = rng.standard_normal((H, W, 3)).astype(np.float32)
    return grids, rgb, v_out, placed.reshape(H, W)


def pixel_regimes(rgb, H, W, GX, GY, GL, coherent=False):
    """{regime: [H,W] bool}, the empty ones left out.  A pixel may carry several labels."""
    fz = guidance(rgb, GL)
    black, white = is_black(rgb), is_white(rgb)
    px, py = np.arange(W)[None, :], np.arange(H)[:, None]
    full = np.ones((H, W), bool)
    m = {"black": black, "white": white, "below_range": (fz < 0) & ~black, "above_range": (fz > GL - 1) & ~white}
    dist = node_distance(rgb, GL)
    m["near_node"] = (dist >= 1e-3) & (dist <= 2e-3) & (fz > 0) & (fz < GL - 1)
    m["on_x_node"] = full & ((px * (GX - 1) % (W - 1) == 0) & (px < W - 1))
    m["on_y_node"] = full & ((py * (GY - 1) % (H - 1) == 0) & (py < H - 1))
    m["last_col"], m["last_row"] = full & (px == W - 1), full & (py == H - 1)
    m["segment_start"] = full & ((px % SEG == 0) & (px > 0))
    m["interior"] = ~np.any(list(m.values()), axis=0)
    m["coherent"] = full & coherent
    return {k: m[k] for k in PIXEL_REGIMES if m[k].any()}


def node_regimes(reach, reach_big):
    """{regime: [GL,GY,GX] bool} from the reach counts of the float64 restatement, the empty ones left out."""
    GL, GY, GX = reach.shape
    on_x = ((np.arange(GX) == 0) | (np.arange(GX) == GX - 1))[None, None, :]
    on_y = ((np.arange(GY) == 0) | (np.arange(GY) == GY - 1))[None, :, None]
    full = np.ones(reach.shape, bool)
    m = {"corner": full & on_x & on_y, "edge": full & (on_x ^ on_y), "interior": full & ~on_x & ~on_y,
         "sparse": (reach >= 1) & (reach <= 4), "multi_chunk": reach_big > 0, "unreached": reach == 0}  # fmt: skip
    return {k: m[k] for k in NODE_REGIMES if m[k].any()}


@functools.lru_cache(maxsize=None)
def regime_case(H, W, GX, GY, GL, num=1, cam=0, kind="noise", seed=0):
    """One shape of SHAPES: inputs (``existing``: those of ``case``), the float64 restatement (r64), the regime masks of pixels
    and of grid nodes, and E32 per array and regime from the fp32 restatement.  Computed once, shared, read-only."""
    if kind == "existing":
        c = case(H, W, GX, GY, GL, num, cam, seed)
        grids, rgb, v_out = c["grids"], c["rgb"], c["v_out"]
        placed = np.zeros((H, W), bool)
    else:
        grids, rgb, v_out, placed = _inputs(H, W, GX, GY, GL, num, kind, seed)
    r64 = restate(grids[cam], rgb, v_out, np.float64)
    r32 = restate(grids[cam], rgb, v_out, np.float32)
    pix = pixel_regimes(rgb, H, W, GX, GY, GL, kind == "coherent")
    nod = node_regimes(r64["reach"], r64["reach_big"])
    masks = {"out": pix, "v_rgb": pix, "v_grid": nod}
    e32 = {a: P.yardstick(masks[a], P.distance(r32[a], r64[a], r64[a + "_acc"]), FLOOR) for a in ARRAYS}
    res = {"grids": grids, "rgb": rgb, "v_out": v_out, "placed": placed, "cam": cam, "r64": r64, "r32": r32, "masks": masks, "e32": e32,
           "tag": f"{H}x{W} ({GX},{GY},{GL})" + ("" if kind == "noise" else " " + kind)}  # fmt: skip
    for d in (res, r64, r32, pix, nod):
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return res
