"""The definition of ``fg_optflow`` (include/fgraster.h, "OF") on the CPU, in numpy: pyramidal, patch-based,
inverse-compositional Lucas-Kanade with a forward-backward check.  One statement for two number formats: ``dt=np.float64`` is
the yardstick, ``dt=np.float32`` what plain fp32 arithmetic does with the kernel's order of operations (E32 of
tests/parity_common.py).  A helper, not a test.  Also here: the synthetic inputs of the tests (a sum of sinusoids that can be
evaluated at real coordinates, so a warped pair has an analytic flow), the MUTANTS -- the definition restated wrongly on
purpose -- and the factors F of the GPU tests.

THE DEFINITION, in the order the kernel works in:
  grey      0.299 R + 0.587 G + 0.114 B, a uint8 value divided by 255 first
  pyramid   level l+1 = level l under the separable [1 4 6 4 1]/16, coordinates clamped, sampled at even coordinates:
            h = ((p0 + p4) + 4 (p1 + p3)) + 6 p2 along x for the five rows, the same form along y, times 1/256
  gradient  Ix = (A[y, min(x+1, W-1)] - A[y, max(x-1, 0)]) / 2, Iy alike
  start     0 (or init[y s, x s] / s, s = 2^(levels-1)) on the coarsest level; below it twice the bilinear sample of the
            coarser u at (x/2, y/2): index x >> 1, fraction (x & 1) / 2
  sample    B at the integer (cx + x0, cy + y0) with fractions (fx, fy), where x0 = floor(ux), fx = ux - x0 of the CENTRE's
            u (clamped to +-32768 first): an index below 0 becomes 0 and one at or beyond W - 1 becomes W - 1, both with
            fraction 0 -- the clamp of cx + ux to [0, W - 1], the fraction kept exact.  t = v00 + fx (v01 - v00),
            b = v10 + fx (v11 - v10), value = t + fy (b - t)
  window    q over (2r+1)^2 offsets, row by row; (cx, cy) = the clamped p + q
  G         sum Ix Ix + lambda, sum Ix Iy, sum Iy Iy + lambda, lambda = 1e-6;  det = Gxx Gyy - Gxy Gxy
  update    It = B(...) - A[cy, cx];  bx = sum It Ix, by = sum It Iy;  ux -= (Gyy bx - Gxy by) / det,
            uy -= (Gxx by - Gxy bx) / det;  ``iters`` times
  validity  (i) ((Gxx + Gyy) - sqrt((Gxx - Gyy)^2 + 4 Gxy^2)) / (2 (2r+1)^2) >= min_eig at level 0;  (ii) 0 <= x + ux <= W - 1
            and 0 <= y + uy <= H - 1;  (iii) |u_ab + u_ba(x + u_ab)|_2 <= consistency, u_ba sampled bilinearly as above
"""
import math

import numpy as np

LAMBDA = 1e-6
U_CLAMP = 32768.0
MUTANTS = ("per_pixel_warp", "gradient_of_b", "no_factor_2", "three_tap", "u_ba_at_x")

# The factors of tests/test_optical_flow_gpu.py: 4 x the worst ratio recorded on an MI355X, rounded up to a power of two
# (profiles/optical_flow_parity.md has the table); None = a recording run (parity_common.bound passes everything).
F_PYRAMID = 1.0  # worst recorded ratio 0.22
F_STEP = 4.0  # 0.63
F_CALL = 16.0  # 3.3
FLOOR = 16 * 2.0**-24  # the families' floor of E32


def default_levels(H: int, W: int) -> int:
    """``levels=None``: the largest L <= 6 whose coarsest level has a shorter side >= 16 (at least 1)."""
    L, s = 1, min(H, W)
    while L < 6 and (s + 1) // 2 >= 16:
        s = (s + 1) // 2
        L += 1
    return L


def level_shapes(H: int, W: int, levels: int):
    out = [(H, W)]
    for _ in range(levels - 1):
        H, W = (H + 1) // 2, (W + 1) // 2
        out.append((H, W))
    return out


def grey(img: np.ndarray, dt) -> np.ndarray:
    if img.ndim == 3 and img.shape[2] != 3:
        raise ValueError(f"optical flow wants [H,W] or [H,W,3] images, got {img.shape}")
    x = img.astype(dt)
    if img.dtype == np.uint8:
        x = x / dt(255)
    if img.ndim == 2:
        return x
    return (dt(0.299) * x[..., 0] + dt(0.587) * x[..., 1]) + dt(0.114) * x[..., 2]


def _five(p0, p1, p2, p3, p4, dt):
    return ((p0 + p4) + dt(4) * (p1 + p3)) + dt(6) * p2


def down(a: np.ndarray, dt, three_tap: bool = False, absolute: bool = False) -> np.ndarray:
    """One pyramid step.  ``absolute``: every tap by magnitude (the denominator of the parity protocol)."""
    H, W = a.shape
    a = np.abs(a) if absolute else a
    xs = np.arange(0, W, 2)
    ys = np.arange(0, H, 2)
    cx = [np.clip(xs + d, 0, W - 1) for d in (-2, -1, 0, 1, 2)]
    cy = [np.clip(ys + d, 0, H - 1) for d in (-2, -1, 0, 1, 2)]
    if three_tap:  # [1 2 1]/4 both ways
        h = (a[:, cx[1]] + a[:, cx[3]]) + dt(2) * a[:, cx[2]]
        return ((h[cy[1]] + h[cy[3]]) + dt(2) * h[cy[2]]) * dt(1.0 / 16)
    h = _five(*(a[:, c] for c in cx), dt)
    return _five(*(h[c] for c in cy), dt) * dt(1.0 / 256)


def pyramid(img: np.ndarray, levels: int, dt, three_tap: bool = False):
    out = [grey(img, dt)]
    for _ in range(levels - 1):
        out.append(down(out[-1], dt, three_tap))
    return out


def pyramid_den(img: np.ndarray, levels: int):
    """float64, per level: the absolute accumulation of the taps that form the level from the one above it."""
    g = grey(img, np.float64)
    ag = grey(np.abs(img.astype(np.float64)) if img.dtype != np.uint8 else img, np.float64)
    out, cur = [ag], g
    for _ in range(levels - 1):
        out.append(down(cur, np.float64, absolute=True))
        cur = down(cur, np.float64)
    return out


def gradients(a: np.ndarray, dt):
    H, W = a.shape
    x, y = np.arange(W), np.arange(H)
    ix = (a[:, np.minimum(x + 1, W - 1)] - a[:, np.maximum(x - 1, 0)]) * dt(0.5)
    iy = (a[np.minimum(y + 1, H - 1)] - a[np.maximum(y - 1, 0)]) * dt(0.5)
    return ix, iy


def bilinear(img: np.ndarray, ix, iy, fx, fy):
    """``img`` [h,w] at integer (ix, iy) + fractions (fx, fy) under the sample rule of the definition."""
    h, w = img.shape
    ex = (ix < 0) | (ix >= w - 1)
    ey = (iy < 0) | (iy >= h - 1)
    ix, iy = np.clip(ix, 0, w - 1), np.clip(iy, 0, h - 1)
    fx, fy = np.where(ex, 0, fx).astype(img.dtype), np.where(ey, 0, fy).astype(img.dtype)
    ix1, iy1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
    v00, v01, v10, v11 = img[iy, ix], img[iy, ix1], img[iy1, ix], img[iy1, ix1]
    t = v00 + fx * (v01 - v00)
    b = v10 + fx * (v11 - v10)
    return t + fy * (b - t)


def split(u: np.ndarray):
    """-> (floor as int64, fraction) of u clamped to +-U_CLAMP (a NaN takes the lower end, as fmaxf gives it)."""
    uc = np.where(np.isnan(u), -U_CLAMP, np.clip(u, -U_CLAMP, U_CLAMP)).astype(u.dtype)
    f = np.floor(uc)
    return f.astype(np.int64), uc - f


def upsample(u: np.ndarray, H: int, W: int, dt, factor=2.0) -> np.ndarray:
    """The start of a level [H,W,2] from the coarser level's u."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fx, fy = (x & 1).astype(dt) * dt(0.5), (y & 1).astype(dt) * dt(0.5)
    return np.stack([dt(factor) * bilinear(u[..., c], x >> 1, y >> 1, fx, fy) for c in (0, 1)], -1)


def structure(A: np.ndarray, radius: int, dt, grad_of=None):
    """-> (cx, cy, Ix, Iy per window offset, Gxx, Gxy, Gyy) of one level; lists in the window's row order."""
    H, W = A.shape
    ix, iy = gradients(A if grad_of is None else grad_of, dt)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    win = []
    gxx, gxy, gyy = (np.zeros((H, W), dt) for _ in range(3))
    for qy in range(-radius, radius + 1):
        for qx in range(-radius, radius + 1):
            cx, cy = np.clip(x + qx, 0, W - 1), np.clip(y + qy, 0, H - 1)
            gx, gy = ix[cy, cx], iy[cy, cx]
            win.append((cx, cy, gx, gy))
            gxx = gxx + gx * gx
            gxy = gxy + gx * gy
            gyy = gyy + gy * gy
    return win, gxx + dt(LAMBDA), gxy, gyy + dt(LAMBDA)


def iterate(A, B, u, radius: int, iters: int, dt, mutant=None, want_den: bool = False):
    """``iters`` updates of u [H,W,2] on one level -> (u, (Gxx, Gxy, Gyy)[, den of the LAST update])."""
    win, gxx, gxy, gyy = structure(A, radius, dt, grad_of=B if mutant == "gradient_of_b" else None)
    det = gxx * gyy - gxy * gxy
    ux, uy = u[..., 0].astype(dt), u[..., 1].astype(dt)
    den = None
    for _ in range(iters):
        x0, fx = split(ux)
        y0, fy = split(uy)
        bx, by = np.zeros_like(ux), np.zeros_like(ux)
        abx, aby = np.zeros_like(ux), np.zeros_like(ux)
        for cx, cy, gx, gy in win:
            if mutant == "per_pixel_warp":
                it = bilinear(B, cx + x0[cy, cx], cy + y0[cy, cx], fx[cy, cx], fy[cy, cx]) - A[cy, cx]
            else:
                it = bilinear(B, cx + x0, cy + y0, fx, fy) - A[cy, cx]
            bx = bx + it * gx
            by = by + it * gy
            if want_den:
                abx += np.abs(it * gx)
                aby += np.abs(it * gy)
        if want_den:
            den = np.stack([np.abs(ux) + (np.abs(gyy) * abx + np.abs(gxy) * aby) / np.abs(det),
                            np.abs(uy) + (np.abs(gxx) * aby + np.abs(gxy) * abx) / np.abs(det)], -1)  # fmt: skip
        ux = ux - (gyy * bx - gxy * by) / det
        uy = uy - (gxx * by - gxy * bx) / det
    out = (np.stack([ux, uy], -1), (gxx, gxy, gyy))
    return out + (den,) if want_den else out


def min_eig(g, radius: int, dt) -> np.ndarray:
    gxx, gxy, gyy = g
    d = gxx - gyy
    return ((gxx + gyy) - np.sqrt(d * d + dt(4) * (gxy * gxy))) * dt(0.5 / (2 * radius + 1) ** 2)


def one_direction(pa, pb, iters: int, radius: int, init, dt, mutant=None):
    """Coarse to fine over two pyramids -> (u at level 0, the level-0 G)."""
    L = len(pa)
    h, w = pa[-1].shape
    if init is None:
        u = np.zeros((h, w, 2), dt)
    else:
        s = 1 << (L - 1)
        u = init.astype(dt)[::s, ::s][:h, :w] * dt(1.0 / s)
    for l in range(L - 1, -1, -1):
        if l != L - 1:
            u = upsample(u, *pa[l].shape, dt, factor=1.0 if mutant == "no_factor_2" else 2.0)
        u, g = iterate(pa[l], pb[l], u, radius, iters, dt, mutant)
    return u, g


def residual(u_ab: np.ndarray, u_ba: np.ndarray, dt, at_x: bool = False) -> np.ndarray:
    """u_ab(x) + u_ba(x + u_ab(x)) [H,W,2] (``at_x``: the mutant that samples u_ba at x)."""
    H, W = u_ab.shape[:2]
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if at_x:
        return u_ab + u_ba
    x0, fx = split(u_ab[..., 0])
    y0, fy = split(u_ab[..., 1])
    return np.stack([u_ab[..., c] + bilinear(np.ascontiguousarray(u_ba[..., c]), x + x0, y + y0, fx, fy) for c in (0, 1)], -1)


def optical_flow(a, b, levels=None, iters=4, radius=3, min_eig_=1e-5, consistency=1.0, init=None, dt=np.float64, mutant=None,
                 details: bool = False):
    """-> (flow [H,W,2], valid bool [H,W]) of the definition; ``details``: also a dict with eig, u_ba and the residual."""
    H, W = a.shape[:2]
    L = default_levels(H, W) if levels is None else levels
    tt = mutant == "three_tap"
    pa, pb = pyramid(a, L, dt, tt), pyramid(b, L, dt, tt)
    u, g = one_direction(pa, pb, iters, radius, init, dt, mutant)
    eig = min_eig(g, radius, dt)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    px, py = x.astype(dt) + u[..., 0], y.astype(dt) + u[..., 1]
    with np.errstate(invalid="ignore"):
        valid = (eig >= dt(min_eig_)) & (px >= 0) & (px <= dt(W - 1)) & (py >= 0) & (py <= dt(H - 1))
    info = {"eig": eig}
    if consistency is not None:
        u_ba, _ = one_direction(pb, pa, iters, radius, None, dt, mutant)
        r = residual(u, u_ba, dt, at_x=mutant == "u_ba_at_x")
        with np.errstate(invalid="ignore"):
            valid &= np.sqrt(r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) <= dt(consistency)
        info.update(u_ba=u_ba, residual=r)
    return (u, valid, info) if details else (u, valid)


# ---- the synthetic inputs ------------------------------------------------------------------------------------------------


class Texture:
    """f(x, y): 48 sinusoids, frequencies uniform in 0.02 .. 0.18 cycles per pixel, random directions and phases, amplitude
    proportional to 1 / frequency, the sum scaled into about [0, 1] (three standard deviations either side of 0.5)."""

    def __init__(self, seed: int, n: int = 48):
        rng = np.random.default_rng(seed)
        f = rng.uniform(0.02, 0.18, n)
        th = rng.uniform(0, 2 * math.pi, n)
        self.kx, self.ky = 2 * math.pi * f * np.cos(th), 2 * math.pi * f * np.sin(th)
        self.ph = rng.uniform(0, 2 * math.pi, n)
        self.amp = (1 / f) / (6 * math.sqrt(((1 / f) ** 2).sum() / 2))

    def __call__(self, x, y):
        x, y = np.asarray(x, np.float64)[..., None], np.asarray(y, np.float64)[..., None]
        return 0.5 + (self.amp * np.sin(self.kx * x + self.ky * y + self.ph)).sum(-1)


AFFINE_CASES = {
    "shift_small": (np.eye(2), (1.3, -0.7)),
    "shift_mid": (np.eye(2), (6.4, 3.2)),
    "shift_large": (np.eye(2), (-11.0, 7.0)),
    "rotate_zoom": (1.02 * np.array([[math.cos(0.03), -math.sin(0.03)], [math.sin(0.03), math.cos(0.03)]]), (-2.0, 1.5)),
}
SHAPES = ((128, 160), (97, 131))
LEVELS = 4


def affine_pair(H: int, W: int, case: str, seed: int = 0):
    """-> (a, b float32 [H,W], truth float64 [H,W,2]): a = f(x), b(y) = f(M^-1 (y - c)), u(x) = (M - I) x + c."""
    M, c = AFFINE_CASES[case]
    f = Texture(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    Mi = np.linalg.inv(M)
    xs, ys = x - c[0], y - c[1]
    a = f(x, y)
    b = f(Mi[0, 0] * xs + Mi[0, 1] * ys, Mi[1, 0] * xs + Mi[1, 1] * ys)
    truth = np.stack([(M[0, 0] - 1) * x + M[0, 1] * y + c[0], M[1, 0] * x + (M[1, 1] - 1) * y + c[1]], -1)
    return a.astype(np.float32), b.astype(np.float32), truth


DISC_SHAPE, DISC_CENTRE, DISC_RADIUS, DISC_SHIFT = (128, 160), (80.0, 64.0), 28.0, (4.0, -3.0)


def disc_pair(seed: int = 0):
    """A disc of radius 28 with a texture of its own moves by (4, -3) over the static first texture -> (a, b float32,
    truth [H,W,2] on a's grid, inside: the disc eroded by 8 px, outside: 8 px or more from both disc positions)."""
    H, W = DISC_SHAPE
    f, g = Texture(seed), Texture(seed + 100)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d0 = np.hypot(x - DISC_CENTRE[0], y - DISC_CENTRE[1])
    d1 = np.hypot(x - DISC_CENTRE[0] - DISC_SHIFT[0], y - DISC_CENTRE[1] - DISC_SHIFT[1])
    a = np.where(d0 <= DISC_RADIUS, g(x, y), f(x, y))
    b = np.where(d1 <= DISC_RADIUS, g(x - DISC_SHIFT[0], y - DISC_SHIFT[1]), f(x, y))
    truth = np.where((d0 <= DISC_RADIUS)[..., None], np.array(DISC_SHIFT), 0.0)
    return a.astype(np.float32), b.astype(np.float32), truth, d0 <= DISC_RADIUS - 8, (d0 >= DISC_RADIUS + 8) & (d1 >= DISC_RADIUS + 8)


def interior(H: int, W: int, radius: int = 3, levels: int = LEVELS) -> np.ndarray:
    m = 2 * radius + (1 << (levels - 1))
    out = np.zeros((H, W), bool)
    out[m : H - m, m : W - m] = True
    return out


def tercile_masks(eig: np.ndarray, within=None) -> dict:
    """Regimes by tercile of the level-0 smaller eigenvalue (over ``within``, default everywhere)."""
    within = np.ones(eig.shape, bool) if within is None else within
    lo, hi = np.quantile(eig[within], [1 / 3, 2 / 3]) if within.any() else (0.0, 0.0)
    return {"eig_low": within & (eig <= lo), "eig_mid": within & (eig > lo) & (eig <= hi), "eig_high": within & (eig > hi)}


def call_distance(u: np.ndarray, u64: np.ndarray) -> np.ndarray:
    """The whole call's distance per pixel: |u - u64|_2 / (1 + |u64|_2)."""
    return np.linalg.norm(u.astype(np.float64) - u64, axis=-1) / (1 + np.linalg.norm(u64, axis=-1))


# ---- what the host and the GPU tests share, computed once and left unchanged ---------------------------------------------

import functools  # noqa: E402

FORMATS = {"f64": np.float64, "f32": np.float32}
CALL_CASES = tuple((case, H, W) for H, W in SHAPES for case in AFFINE_CASES) + (("disc",) + DISC_SHAPE,)


def _frozen(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _frozen(v)
    elif isinstance(x, (tuple, list)):
        for v in x:
            _frozen(v)
    return x


@functools.lru_cache(maxsize=None)
def pair(case: str, H: int, W: int):
    """-> (a, b, truth) of an affine case or of "disc"."""
    return _frozen(disc_pair()[:3] if case == "disc" else affine_pair(H, W, case))


@functools.lru_cache(maxsize=None)
def reference(case: str, H: int, W: int, fmt: str, mutant=None):
    """-> (flow, valid, info) of the whole call with the defaults at LEVELS levels, in one of FORMATS."""
    a, b, _ = pair(case, H, W)
    return _frozen(optical_flow(a, b, levels=LEVELS, dt=FORMATS[fmt], mutant=mutant, details=True))


STEP_SHAPES = ((24, 40), (97, 131))


@functools.lru_cache(maxsize=None)
def step_inputs(H: int, W: int):
    """One update step: a rotate-and-zoom pair and an ``init`` with sub-pixel parts, up to 1.5 px off the truth."""
    a, b, truth = affine_pair(H, W, "rotate_zoom", seed=3)
    rng = np.random.default_rng(H * 1000 + W)
    init = (truth + rng.uniform(-1.5, 1.5, truth.shape)).astype(np.float32)
    return _frozen((a, b, init))


@functools.lru_cache(maxsize=None)
def one_step(H: int, W: int, fmt: str, mutant=None, radius: int = 3):
    """levels = 1, iters = 1 from ``step_inputs`` -> (u1 [H,W,2], den [H,W,2], eig [H,W])."""
    dt = FORMATS[fmt]
    a, b, init = step_inputs(H, W)
    u, g, den = iterate(grey(a, dt), grey(b, dt), init.astype(dt), radius, 1, dt, mutant, want_den=True)
    return _frozen((u, den, min_eig(g, radius, dt)))


def border_masks(H: int, W: int, reach: int) -> dict:
    """Pixels whose window (or taps) of ``reach`` pixels is clamped at the image's edge, and the rest."""
    inner = np.zeros((H, W), bool)
    inner[reach : H - reach, reach : W - reach] = True
    return {"border": ~inner, "interior": inner}


def step_masks(H: int, W: int, eig: np.ndarray, radius: int = 3) -> dict:
    """Regimes of the one-step test: tercile of the smaller eigenvalue x border or interior window."""
    out = {}
    for bname, bm in border_masks(H, W, radius).items():
        for ename, em in tercile_masks(eig).items():
            out[f"{ename}-{bname}"] = em & bm
    return out


PYRAMID_SHAPES = ((97, 131), (64, 80))
PYRAMID_KINDS = ("u8_rgb", "f32_rgb", "f32_grey")
PYRAMID_LEVELS = 3


@functools.lru_cache(maxsize=None)
def pyramid_input(kind: str, H: int, W: int) -> np.ndarray:
    rng = np.random.default_rng(len(kind) * 100000 + H * 1000 + W)
    if kind == "u8_rgb":
        return _frozen(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    shape = (H, W, 3) if kind == "f32_rgb" else (H, W)
    return _frozen(rng.uniform(-0.5, 1.5, shape).astype(np.float32))  # (both signs: the taps can cancel)


def validity(u: np.ndarray, info: dict, consistency, min_eig_: float = 1e-5, at_x: bool = False) -> np.ndarray:
    """The validity map of a whole-call result at ANOTHER ``consistency`` (``at_x``: under the mutant ``u_ba_at_x``)."""
    dt = u.dtype.type
    H, W = u.shape[:2]
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    px, py = x.astype(dt) + u[..., 0], y.astype(dt) + u[..., 1]
    r = residual(u, info["u_ba"], dt, at_x=True) if at_x else info["residual"]
    with np.errstate(invalid="ignore"):
        return ((info["eig"] >= dt(min_eig_)) & (px >= 0) & (px <= dt(W - 1)) & (py >= 0) & (py <= dt(H - 1))
                & (np.sqrt(r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) <= dt(consistency)))  # fmt: skip


# a threshold tight enough that WHERE u_ba is sampled decides: on the rotate-and-zoom pair u_ab(x) + u_ba(x) is the second-order
# term (M + M^-1 - 2 I) x + (I - M^-1) c, up to 0.25 px at the far corner, while the true residual is the estimator's own error
TIGHT_CONSISTENCY = 0.1
TIGHT_CASE = ("rotate_zoom", 97, 131)
