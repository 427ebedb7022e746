"""Float64 restatement of the fused colour correction's contract (include/fgraster.h, "CC"), and the seeded inputs its tests
share.  A helper, not a test.

Per iteration and channel the masked rows are REMOVED and the fit is ``torch.linalg.lstsq(..., driver="gelsd")`` in float64
(an SVD-based minimum-norm least-squares solve: none of the normal equations, the diagonal scaling or the Jacobi sweeps of
the kernel); an empty mask gives w = 0.  The features are formed in fp32 and the warp is applied in fp32, as the contract
states.  Beside the image it returns what the tests condition on: the margin of every compared value from the two
thresholds, and each solve's numerical rank."""
import functools

import numpy as np
import torch

RCOND = 1e-12  # FG_COLOR_CORRECT_RCOND: on the eigenvalues of the unit-diagonal Gram, i.e. 1e-6 on the singular values below


def thresholds(eps, compare="fp32"):
    """(lo, hi): fp32 comparisons against the rounded scalars -- or, for the threshold test's counter-model, float64 ones."""
    if compare == "fp32":
        return torch.tensor(eps, dtype=torch.float32), torch.tensor(1.0 - eps, dtype=torch.float32)
    return torch.tensor(eps, dtype=torch.float64), torch.tensor(1.0 - eps, dtype=torch.float64)


def features(x):
    """[P,3] fp32 -> [P,10] fp32: x0 x0, x0 x1, x0 x2, x1 x1, x1 x2, x2 x2, x0, x1, x2, 1."""
    x0, x1, x2 = x[:, 0], x[:, 1], x[:, 2]
    return torch.stack([x0 * x0, x0 * x1, x0 * x2, x1 * x1, x1 * x2, x2 * x2, x0, x1, x2, torch.ones_like(x0)], dim=-1)


def numerical_rank(rows):
    """Singular values of the rows with unit-norm columns (zero columns left zero) above sqrt(RCOND) times the largest."""
    if rows.shape[0] == 0:
        return 0
    norms = rows.norm(dim=0)
    scaled = rows / torch.where(norms > 0, norms, torch.ones_like(norms))
    s = torch.linalg.svdvals(scaled)
    return int((s > (RCOND**0.5) * s.max()).sum()) if float(s.max()) > 0 else 0


def restate(img, ref, num_iters=5, eps=0.5 / 255, compare="fp32"):
    """-> {"out" [like img] fp32, "warps" [num_iters,10,3] fp32, "rank" [num_iters,3] int, "margin" float}."""
    img, ref = torch.as_tensor(img, dtype=torch.float32).cpu(), torch.as_tensor(ref, dtype=torch.float32).cpu()
    x, y = img.reshape(-1, 3), ref.reshape(-1, 3)
    lo, hi = thresholds(eps, compare)

    def unclipped(z):
        z = z if compare == "fp32" else z.double()
        return (z >= lo) & (z <= hi)

    def distance(z):
        z = z.double()
        return float(torch.minimum((z - float(lo)).abs(), (z - float(hi)).abs()).min())

    mask0 = unclipped(x)
    margin = distance(y)
    warps = torch.zeros(num_iters, 10, 3, dtype=torch.float32)
    ranks = torch.zeros(num_iters, 3, dtype=torch.int64)
    for k in range(num_iters):
        margin = min(margin, distance(x))
        A = features(x)
        for c in range(3):
            m = mask0[:, c] & unclipped(x[:, c]) & unclipped(y[:, c])
            rows, b = A[m].double(), y[m, c].double()
            ranks[k, c] = numerical_rank(rows)
            if rows.shape[0]:
                warps[k, :, c] = torch.linalg.lstsq(rows, b[:, None], driver="gelsd").solution[:, 0].float()
        x = torch.clamp(A @ warps[k], 0, 1)
    return {"out": x.reshape(img.shape), "warps": warps, "rank": ranks, "margin": margin}


# ---- seeded inputs: (img, ref) float32 [H,W,3] on the CPU ------------------------------------------------------------
def natural(H, W, seed):
    """Correlated channels (a luminance plus a small chroma), an affine-plus-quadratic colour change and 1 % noise; the
    few values that leave [0, 1] are clipped to exactly 0 and 1."""
    rng = np.random.default_rng(seed)
    P = H * W
    ref = np.clip(rng.uniform(0.03, 0.97, (P, 1)) + rng.normal(0.0, 0.06, (P, 3)), 0.0, 1.0)
    M = np.array([[0.9, 0.05, 0.0], [0.02, 0.85, 0.03], [0.0, 0.04, 0.8]])
    img = ref @ M.T + np.array([0.03, 0.01, 0.05]) + 0.08 * ref * ref + rng.normal(0.0, 0.01, (P, 3))
    to = lambda a: torch.from_numpy(np.clip(a, 0.0, 1.0).astype(np.float32).reshape(H, W, 3))  # noqa: E731
    return to(img), to(ref)


def half_clipped(H, W, seed):
    """``natural`` with the first half of img's pixels at exactly 0 or 1."""
    img, ref = natural(H, W, seed)
    rng = np.random.default_rng(seed + 1000)
    flat = img.reshape(-1, 3).clone()
    n = flat.shape[0] // 2
    flat[:n] = torch.from_numpy(rng.integers(0, 2, (n, 3)).astype(np.float32))
    return flat.reshape(H, W, 3), ref


def zero_img_channel(H, W, seed):
    img, ref = natural(H, W, seed)
    img = img.clone()
    img[..., 0] = 0.0
    return img, ref


def saturated_ref_channel(H, W, seed):
    img, ref = natural(H, W, seed)
    ref = ref.clone()
    ref[..., 1] = 1.0
    return img, ref


def constant(H, W, seed):
    img, ref = natural(H, W, seed)
    return torch.tensor([0.3, 0.5, 0.7]).expand(H, W, 3).contiguous(), ref


def grey(H, W, seed):
    img, ref = natural(H, W, seed)
    return img[..., 1:2].expand(H, W, 3).contiguous(), ref


BUILDERS = {f.__name__: f for f in (natural, half_clipped, zero_img_channel, saturated_ref_channel, constant, grey)}


@functools.lru_cache(maxsize=None)
def case(kind, H, W, seed, num_iters=5):
    """One input pair and its restatement, computed once and shared (treat as read-only)."""
    img, ref = BUILDERS[kind](H, W, seed)
    return {"img": img, "ref": ref, **restate(img, ref, num_iters)}
