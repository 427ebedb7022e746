"""Float64 numpy restatement of the bilateral-grid slice of a whole image (freegaussian_amd/bilagrid.py apply_to_render:
grid_sample with mode="bilinear", align_corners=True, padding_mode="border", then the 3 x 4 multiply), its two gradients,
and the inputs the fused-slice tests share.  A helper, not a test file.

The three luma weights are the fp32 values taken as doubles: a white pixel then clamps in float64 as it does in fp32
(the sum is 1.0000000075).  Vectorised over pixels; a loop version of the same formulas agrees with torch's float64
autograd of apply_to_render to 3e-7 (the weights' own rounding)."""
import functools

import numpy as np

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
