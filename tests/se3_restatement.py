"""The SE(3) transform of the means (csrc/se3_apply.hip, csrc/se3_math.h; ``ops.se3_apply``) restated in plain torch, closed
form, forward and backward, in float64 or float32 -- a helper, not a test.

    theta = |w|,  ws = w / theta + 1e-5,  vs = v / theta + 1e-5,  W = hat(ws)
    R = I + sin(theta) W + (1 - cos theta) W^2,   G = theta I + (1 - cos theta) W + (theta - sin theta) W^2
    out = R x + G vs                                                  (the arithmetic of utils.exp_se3: ``restate`` forward)
    g_w, g_v, g_pts = d(sum g . out) / d(w, v, x)                     (the exact derivative; the offsets are constants)

The backward is written as the kernel's: 1 - cos theta as 2 sin^2(theta / 2), theta - sin theta as its series below 1 rad, and
the two terms of size |v| |g| / theta of the 1 / theta chain cancelled on paper.  In float64 it is torch's float64 autograd of
``deform._se3`` + ``utils.transform_points`` (tests/test_se3_apply_host.py); in float32 it is the yardstick E32 of the GPU test
(tests/parity_common.py has the protocol; rows: the 2-norm of a row's difference over the 2-norm of the float64 row).

``regime_case``: 4096 rows labelled by theta; ``far_point`` (|x| ~ 100) overlays every 16th row.  The two regimes below 1e-2
hold 256 rows each -- 512 of 4096, an eighth -- so that the cap the mutants put on F is decided where fp32 arithmetic is
sound (there the forward itself, in utils.exp_se3's arithmetic, is 2e-4 off: 1 - cos theta times |v| / theta)."""
import functools
import math

import torch

import parity_common as P

FLOOR = 16 * 2.0**-24
# 4 x the worst ratio of a recording run on an MI355X, rounded up to a power of two (profiles/se3_apply_parity.md); None = the
# recording run itself.  Recorded: worst ratio 1.05 (g_v, pi..10) -> 4.2 -> 8
F = 8.0
ARRAYS = ("out", "g_w", "g_v", "g_pts")
REGIMES = (("1e-4..1e-3", 1e-4, 1e-3), ("1e-3..1e-2", 1e-3, 1e-2), ("1e-2..0.1", 1e-2, 0.1), ("0.1..1", 0.1, 1.0),
           ("1..pi", 1.0, math.pi), ("pi..10", math.pi, 10.0))  # fmt: skip
REGIME_NAMES = tuple(r[0] for r in REGIMES)
SMALL = REGIME_NAMES[:2]
ROWS = 4096
ROWS_PER_REGIME = (256, 256, 896, 896, 896, 896)
FAR_EVERY = 16

# deliberate mistakes -> the arrays each concerns
MUTANTS = {
    "dtheta_dw_term_omitted": ("g_w",),  # theta taken as a constant of w: g_w = g_ws / theta
    "R_not_transposed_in_g_pts": ("g_pts",),  # g_pts = R g
    "theta_minus_sin_term_dropped_from_g_v": ("g_v",),  # G^T g without (theta - sin theta) W^2 g
    "v_not_divided_by_theta_in_the_chain": ("g_v",),  # g_v = g_vs
    "cross_term_sign_flipped_in_g_v": ("g_v",),  # G g in place of G^T g
}


def _dot(a, b):
    return (a * b).sum(-1, keepdim=True)


def _cross(a, b):
    return torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                        a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)  # fmt: skip


def _hat(w):
    o = torch.zeros_like(w[:, 0])
    return torch.stack([o, -w[:, 2], w[:, 1], w[:, 2], o, -w[:, 0], -w[:, 1], w[:, 0], o], -1).view(-1, 3, 3)


def theta_minus_sin(theta, s):
    t = theta * theta
    poly = 1 - t / 20 * (1 - t / 42 * (1 - t / 72 * (1 - t / 110 * (1 - t / 156))))
    return torch.where(theta >= 1, theta - s, theta * t / 6 * poly)


def restate(w, v, x, g, dtype, mutant=None):
    """-> {"out", "g_w", "g_v", "g_pts"}: [N,3] tensors of ``dtype``, every operation in ``dtype``."""
    assert mutant is None or mutant in MUTANTS
    w, v, x, g = (a.to(dtype) for a in (w, v, x, g))
    theta = (w[:, 0:1] * w[:, 0:1] + w[:, 1:2] * w[:, 1:2] + w[:, 2:3] * w[:, 2:3]).sqrt()
    n, m = w / theta, v / theta
    ws, vs = n + 1e-5, m + 1e-5
    s, c = torch.sin(theta), torch.cos(theta)
    # forward, as utils.exp_se3 and utils.transform_points form it
    W = _hat(ws)
    W2 = torch.stack([torch.stack([W[:, i, 0] * W[:, 0, j] + W[:, i, 1] * W[:, 1, j] + W[:, i, 2] * W[:, 2, j] for j in range(3)], -1)
                      for i in range(3)], -2)  # fmt: skip
    eye = torch.eye(3, dtype=dtype).expand_as(W)
    th = theta.unsqueeze(-1)
    s3, c3 = s.unsqueeze(-1), c.unsqueeze(-1)
    R = eye + s3 * W + (1.0 - c3) * W2
    G = th * eye + (1.0 - c3) * W + (th - s3) * W2
    p = G[:, :, 0] * vs[:, 0:1] + G[:, :, 1] * vs[:, 1:2] + G[:, :, 2] * vs[:, 2:3]
    out = R[:, :, 0] * x[:, 0:1] + R[:, :, 1] * x[:, 1:2] + R[:, :, 2] * x[:, 2:3] + p
    # backward, in the forms of csrc/se3_math.h
    inv = 1 / theta
    h = torch.sin(0.5 * theta)
    A, B, C = s, 2 * h * h, theta_minus_sin(theta, s)
    q, gw_ = _dot(ws, ws), _dot(g, ws)
    wxg = _cross(ws, g)
    W2g = gw_ * ws - q * g
    g_pts = g - A * wxg + B * W2g
    if mutant == "R_not_transposed_in_g_pts":
        g_pts = g + A * wxg + B * W2g
    g_v = g - (B * inv) * wxg + (C * inv) * W2g
    if mutant == "theta_minus_sin_term_dropped_from_g_v":
        g_v = g - (B * inv) * wxg
    elif mutant == "v_not_divided_by_theta_in_the_chain":
        g_v = theta * g_v
    elif mutant == "cross_term_sign_flipped_in_g_v":
        g_v = g + (B * inv) * wxg + (C * inv) * W2g
    wx, wv, gx, gvs = _dot(ws, x), _dot(ws, vs), _dot(g, x), _dot(g, vs)
    u = A * x + B * vs
    gws = _cross(u, g) + B * (wx * g + gw_ * x - (2 * gx) * ws) + C * (wv * g + gw_ * vs - (2 * gvs) * ws)
    W2x, W2v = wx * ws - q * x, wv * ws - q * vs
    dth = c * _cross(ws, x) + A * (W2x + _cross(ws, vs)) + B * W2v
    bracket = _dot(g, dth) + 1e-5 * g.sum(-1, keepdim=True) + _dot(m, (B * inv) * wxg - (C * inv) * W2g) - _dot(n, gws) * inv
    g_w = inv * gws + bracket * n
    if mutant == "dtheta_dw_term_omitted":
        g_w = inv * gws
    return {"out": out, "g_w": g_w, "g_v": g_v, "g_pts": g_pts}


def labels_of(w) -> list:
    """One regime name per row, from the float64 norm of the float32 w; None outside every regime."""
    theta = w.double().norm(dim=-1)
    out = []
    for t in theta.tolist():
        out.append(next((name for name, lo, hi in REGIMES if lo <= t < hi), None))
    return out


@functools.lru_cache(maxsize=None)
def regime_case(seed: int = 0) -> dict:
    """float32 inputs ``w, v, x, g`` [4096,3] (|v| ~ 0.3, |x| ~ 2, far points |x| ~ 100, g ~ N(0,1)), shuffled over the rows;
    ``labels``; ``masks`` {regime or "far_point": [4096] bool}; ``r64`` / ``r32`` the restatements; ``d32`` / ``e32`` per array
    the fp32 restatement's row distances and the floored yardstick per regime.  Shared: leave it unchanged."""
    gen = torch.Generator().manual_seed(1000 + seed)
    thetas = []
    for (name, lo, hi), count in zip(REGIMES, ROWS_PER_REGIME):
        lo, hi = lo * 1.001, hi * 0.999  # (clear of the regime's ends after rounding to float32)
        thetas.append(torch.exp(torch.rand(count, generator=gen, dtype=torch.float64) * math.log(hi / lo) + math.log(lo)))
    theta = torch.cat(thetas)[torch.randperm(ROWS, generator=gen)]
    axis = torch.randn(ROWS, 3, generator=gen, dtype=torch.float64)
    w = (axis / axis.norm(dim=-1, keepdim=True) * theta[:, None]).float()
    v = (torch.randn(ROWS, 3, generator=gen, dtype=torch.float64) * (0.3 / math.sqrt(3))).float()
    x = torch.randn(ROWS, 3, generator=gen, dtype=torch.float64) * (2 / math.sqrt(3))
    far = torch.arange(ROWS) % FAR_EVERY == FAR_EVERY - 1
    x = torch.where(far[:, None], x * 50, x).float()
    g = torch.randn(ROWS, 3, generator=gen, dtype=torch.float64).float()
    labels = labels_of(w)
    assert None not in labels
    masks = P.masks_of_labels(labels)
    masks = {name: masks[name] for name in REGIME_NAMES}
    masks["far_point"] = far
    r64, r32 = restate(w, v, x, g, torch.float64), restate(w, v, x, g, torch.float32)
    d32 = {a: P.distance(r32[a], r64[a], r64[a], rows=True) for a in ARRAYS}
    e32 = {a: P.yardstick(masks, d32[a], FLOOR) for a in ARRAYS}
    return {"w": w, "v": v, "x": x, "g": g, "labels": labels, "masks": masks, "r64": r64, "r32": r32, "d32": d32, "e32": e32}


def smallest_e32(case: dict, array: str) -> torch.Tensor:
    """Per row: the smallest E32 among the regimes it carries (the GPU test checks it under each)."""
    e = torch.full((ROWS,), math.inf, dtype=torch.float64)
    for name, mask in case["masks"].items():
        e = torch.where(mask, torch.minimum(e, torch.tensor(case["e32"][array][name], dtype=torch.float64)), e)
    return e


def mutant_caps(seed: int = 0) -> dict:
    """{(mutant, array): three_quarter_cap}: over all 4096 rows, the largest F at which three quarters of the rows of the
    mutant's float64 result are still 4 * F * E32 of the row from the true one."""
    c = regime_case(seed)
    caps = {}
    for mutant, arrays in MUTANTS.items():
        rm = restate(c["w"], c["v"], c["x"], c["g"], torch.float64, mutant)
        for a in arrays:
            ratios = P.distance(rm[a], c["r64"][a], c["r64"][a], rows=True) / smallest_e32(c, a)
            caps[mutant, a] = P.three_quarter_cap(ratios)
    return caps
