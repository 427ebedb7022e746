"""The flow supervision's two kernels (csrc/flow_disp.hip through ``ops.flow_displacement``, csrc/flow_loss.hip through
``ops.flow_l1``) restated in plain torch, closed form, forward and backward, in float64 or float32 -- a helper, not a test.
tests/parity_common.py has the protocol.

DISPLACEMENT (``restate_disp``; rows: the 2-norm of a row's difference over the 2-norm of the float64 row)

    p_t = R_t m_t + tau_t,  p_0 = R_0 m_0 + tau_0,  Delta = p_t - p_0     (one camera: Delta = R (m_t - m_0), p_t = p_0 + Delta)
    valid = z_t > near and z_0 > near and both centres f p / z + c within ``margin`` pixels of the image
    disp  = f (Delta_xy z_0 - p_0xy Delta_z) / (z_t z_0)                   (exact zeros where not valid)
    g_means_t = R_t^T (a, b, -(a x_t + b y_t) / z_t),  (a, b) = g f / z_t;   g_means_0 = -R_0^T (a0, b0, -(a0 x_0 + b0 y_0) / z_0)

``naive=True`` is the textbook form -- mu = K p / z twice and subtract -- whose float64 autograd the host test compares with
and whose fp32 value the GPU test records beside the kernel's at small motion.

``disp_case``: 4096 rows.  256 are invalid by construction (64 each: behind the current camera, behind frame 0's, the current
centre outside the margin, frame 0's outside); 3840 are live, labelled by DEPTH class (z_0 from 1.05 near to 1e3) and by MOTION
class (|Delta| / z_0 from 1e-6 to 1): a row lies in one regime of each kind.  Two modes over the same rows: ``same`` (one camera)
and ``two`` (frame 0 under a camera a small step away); validity is each mode's own.

LOSS (``restate_l1``; per element)

    t = box mean of the d x d source block / d;  w = 0 where the block holds a non-finite value, else the mask's box mean
    loss = sum w (|dx| + |dy|) / (2 max(sum w, tiny));  g_pred = w sign(pred - t) / (2 max(sum w, tiny))
    denominators: the value's absolute accumulation sum w (|p_x| + |t_x| + |p_y| + |t_y|) / (2 sum w); a gradient element's own
    magnitude (a single product).
"""
import functools
import math

import torch

import parity_common as P

FLOOR = 16 * 2.0**-24
# 4 x the worst ratio of a recording run on an MI355X, rounded up to a power of two (profiles/flow_supervision_parity.md);
# None = the recording run itself.  Recorded: displacement worst ratio 1.01 (disp, one camera, 0.02..1) -> 4.04 -> 8; loss worst
# ratio 0.11 (g_pred, 33 x 17, d = 2, float32 mask, partial weight) -> 0.44 -> 1 (the smallest F the rule gives)
F_DISP = 8.0
F_LOSS = 1.0
TINY = 1e-30

# ---------------------------------------------------------------------------------------------------------------------
# displacement

DISP_ARRAYS = ("disp", "g_means_t", "g_means_0")
DEPTHS = (("near..2near", 1.05e-2, 2e-2), ("0.02..1", 2e-2, 1.0), ("1..30", 1.0, 30.0), ("30..1e3", 30.0, 1e3))
MOTIONS = (("1e-6..1e-4", 1e-6, 1e-4), ("1e-4..1e-2", 1e-4, 1e-2), ("1e-2..1", 1e-2, 1.0))
DEPTH_NAMES, MOTION_NAMES = tuple(d[0] for d in DEPTHS), tuple(m[0] for m in MOTIONS)
SMALL_MOTION = MOTION_NAMES[:2]
INVALID_KINDS = ("behind_t", "behind_0", "outside_t", "outside_0")
ROWS, INVALID_PER_KIND = 4096, 64
MODES = ("same", "two")
WIDTH, HEIGHT, NEAR, MARGIN = 640, 480, 0.01, 64.0
CLEAR = 8.0  # pixels every centre keeps from the grown rectangle's edge, on either side

DISP_MUTANTS = {
    "cx_left_in": ("disp",),  # K p formed for Delta but not for p_0: c Delta_z / z_t stays in the value
    "frame0_gradient_sign": ("g_means_0",),  # g_means_0 with the sign of g_means_t
}


def _rot(ax, ay, az):
    def r(a, i, j):
        m = torch.eye(3, dtype=torch.float64)
        m[i, i] = m[j, j] = math.cos(a)
        m[i, j], m[j, i] = -math.sin(a), math.sin(a)
        return m

    return r(az, 0, 1) @ r(ay, 2, 0) @ r(ax, 1, 2)


def _viewmat(R, t):
    V = torch.eye(4, dtype=torch.float64)
    V[:3, :3], V[:3, 3] = R, t
    return V


def cameras():
    """(viewmat_t, viewmat_0, K) as float32 [4,4], [4,4], [3,3]: a general rotation, frame 0's camera a small step away."""
    Rt = _rot(0.3, -0.2, 0.1)
    tt = torch.tensor([2e-3, -1e-3, 5e-4], dtype=torch.float64)
    R0 = _rot(4e-3, -3e-3, 5e-3) @ Rt
    t0 = tt + torch.tensor([3e-3, -2e-3, 1e-3], dtype=torch.float64)
    K = torch.tensor([[520.0, 0.0, 317.3], [0.0, 530.0, 243.9], [0.0, 0.0, 1.0]], dtype=torch.float64)
    return _viewmat(Rt, tt).float(), _viewmat(R0, t0).float(), K.float()


def restate_disp(mt, m0, Vt, V0, K, g, dtype, mutant=None, naive=False, width=WIDTH, height=HEIGHT, near=NEAR, margin=MARGIN):
    """-> {"disp" [N,2], "g_means_t" [N,3], "g_means_0" [N,3], "valid" [N] bool}: every operation in ``dtype``.  ``V0`` None:
    one camera for both frames."""
    assert mutant is None or mutant in DISP_MUTANTS
    mt, m0, Vt, K, g = (a.to(dtype) for a in (mt, m0, Vt, K, g))
    same = V0 is None
    V0 = Vt if same else V0.to(dtype)
    Rt, tt, R0, t0 = Vt[:3, :3], Vt[:3, 3], V0[:3, :3], V0[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    f = torch.stack([fx, fy])
    p0 = m0 @ R0.T + t0
    if same and not naive:
        delta = (mt - m0) @ Rt.T
        pt = p0 + delta
    else:
        pt = mt @ Rt.T + tt
        delta = pt - p0
    zt, z0 = pt[:, 2:3], p0[:, 2:3]
    ct = f * pt[:, :2] / zt + torch.stack([cx, cy])
    c0 = f * p0[:, :2] / z0 + torch.stack([cx, cy])
    lo = torch.tensor([-margin, -margin], dtype=dtype)
    hi = torch.tensor([width + margin, height + margin], dtype=dtype)
    inside = ((ct >= lo) & (ct <= hi) & (c0 >= lo) & (c0 <= hi)).all(-1)
    valid = (zt[:, 0] > near) & (z0[:, 0] > near) & inside
    if naive:
        disp = ct - c0
    else:
        num = delta[:, :2] * z0 - p0[:, :2] * delta[:, 2:3]
        if mutant == "cx_left_in":
            num = num + torch.stack([cx, cy]) / f * delta[:, 2:3] * z0
        disp = f * num / (zt * z0)
    ab = g * f / zt
    gpt = torch.cat([ab, -(ab * pt[:, :2]).sum(-1, keepdim=True) / zt], -1)
    ab0 = g * f / z0
    gp0 = -torch.cat([ab0, -(ab0 * p0[:, :2]).sum(-1, keepdim=True) / z0], -1)
    g_t, g_0 = gpt @ Rt, gp0 @ R0
    if mutant == "frame0_gradient_sign":
        g_0 = -g_0
    zero = torch.zeros((), dtype=dtype)
    v = valid[:, None]
    return {"disp": torch.where(v, disp, zero), "g_means_t": torch.where(v, g_t, zero), "g_means_0": torch.where(v, g_0, zero),
            "valid": valid}  # fmt: skip


def _project64(p, K):
    return torch.stack([K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]], -1)


def _clear_inside(c):
    lo = -MARGIN + CLEAR
    return ((c[:, 0] >= lo) & (c[:, 0] <= WIDTH + MARGIN - CLEAR) & (c[:, 1] >= lo) & (c[:, 1] <= HEIGHT + MARGIN - CLEAR))


@functools.lru_cache(maxsize=None)
def disp_case(seed: int = 0) -> dict:
    """float32 ``mt, m0`` [4096,3], ``g`` [4096,2], the cameras; ``depth`` / ``motion`` / ``kind`` labels per row (None where the
    other applies); per mode in ``MODES``: ``r64`` / ``r32`` / ``naive32`` the restatements, ``masks`` {regime: [4096] bool, live
    rows only}, ``d32`` / ``e32`` per array.  Shared: leave it unchanged."""
    gen = torch.Generator().manual_seed(2000 + seed)
    Vt32, V032, K32 = cameras()
    Vt, K = Vt32.double(), K32.double()
    Rt, tt = Vt[:3, :3], Vt[:3, 3]
    live = ROWS - INVALID_PER_KIND * len(INVALID_KINDS)
    per = live // (len(DEPTHS) * len(MOTIONS))
    depth, motion = [], []
    for dn in DEPTH_NAMES:
        for mn in MOTION_NAMES:
            depth += [dn] * per
            motion += [mn] * per
    while len(depth) < live:  # the remainder: the first regimes once more
        depth.append(DEPTH_NAMES[len(depth) % len(DEPTHS)])
        motion.append(MOTION_NAMES[len(motion) % len(MOTIONS)])
    kind = [None] * live
    for k in INVALID_KINDS:  # an invalid row starts as a live one of the two middle depth classes and the largest motion
        depth += [DEPTH_NAMES[1 + len(depth) % 2]] * INVALID_PER_KIND
        motion += [MOTION_NAMES[2]] * INVALID_PER_KIND
        kind += [k] * INVALID_PER_KIND
    rng = lambda n: torch.rand(n, generator=gen, dtype=torch.float64)  # noqa: E731
    dlo = torch.tensor([dict((d[0], d[1]) for d in DEPTHS)[n] for n in depth], dtype=torch.float64)
    dhi = torch.tensor([dict((d[0], d[2]) for d in DEPTHS)[n] for n in depth], dtype=torch.float64)
    mlo = torch.tensor([dict((m[0], m[1]) for m in MOTIONS)[n] for n in motion], dtype=torch.float64)
    mhi = torch.tensor([dict((m[0], m[2]) for m in MOTIONS)[n] for n in motion], dtype=torch.float64)
    z0 = torch.exp(rng(ROWS) * torch.log(dhi * 0.999 / (dlo * 1.001)) + torch.log(dlo * 1.001))
    uv = torch.stack([20 + rng(ROWS) * (WIDTH - 40), 20 + rng(ROWS) * (HEIGHT - 40)], -1)
    p0 = torch.stack([(uv[:, 0] - K[0, 2]) / K[0, 0] * z0, (uv[:, 1] - K[1, 2]) / K[1, 1] * z0, z0], -1)
    rel = torch.exp(rng(ROWS) * torch.log(mhi * 0.999 / (mlo * 1.001)) + torch.log(mlo * 1.001))
    delta = torch.zeros(ROWS, 3, dtype=torch.float64)
    todo = torch.ones(ROWS, dtype=torch.bool)
    for _ in range(64):  # directions are drawn again until the moved centre is in front of the camera and clear inside
        d = torch.randn(ROWS, 3, generator=gen, dtype=torch.float64)
        d = d / d.norm(dim=-1, keepdim=True) * (rel * z0)[:, None]
        d[:, 2] = torch.where(z0 + d[:, 2] < 1.05 * NEAR, d[:, 2].abs(), d[:, 2])
        delta = torch.where(todo[:, None], d, delta)
        pt = p0 + delta
        todo = ~(_clear_inside(_project64(pt, K)) & (pt[:, 2] >= 1.05 * NEAR))
        if not bool(todo.any()):
            break
    assert not bool(todo.any())
    pt = p0 + delta
    # the invalid rows: one frame's point behind the camera (half the near plane, or as far behind as in front), or its centre
    # CLEAR + 20 pixels and more outside the grown rectangle
    for i, k in enumerate(kind):
        if k is None:
            continue
        p = pt if k.endswith("_t") else p0
        if k.startswith("behind"):
            p[i, 2] = 0.5 * NEAR if i % 2 else -p[i, 2]
        else:
            side = i % 4
            u = (-MARGIN - CLEAR - 20 - 50 * (i % 3), WIDTH + MARGIN + CLEAR + 20 + 50 * (i % 3))[side % 2]
            if side < 2:
                p[i, 0] = (u - K[0, 2]) / K[0, 0] * p[i, 2]
            else:
                u = u if side == 2 else HEIGHT + MARGIN + CLEAR + 20 + 50 * (i % 3)
                p[i, 1] = (u - K[1, 2]) / K[1, 1] * p[i, 2]
    perm = torch.randperm(ROWS, generator=gen)
    p0, pt = p0[perm], pt[perm]
    depth, motion, kind = ([x[i] for i in perm.tolist()] for x in (depth, motion, kind))
    m0 = ((p0 - tt) @ Rt).float()  # R^T (p - tau) per row
    mt = (m0.double() + (pt - p0) @ Rt).float()
    g = torch.randn(ROWS, 2, generator=gen, dtype=torch.float64).float()
    out = {"mt": mt, "m0": m0, "g": g, "Vt": Vt32, "V0": V032, "K": K32, "depth": depth, "motion": motion, "kind": kind}
    labelled = {**P.masks_of_labels([d if k is None else None for d, k in zip(depth, kind)]),
                **P.masks_of_labels([m if k is None else None for m, k in zip(motion, kind)])}  # fmt: skip
    labelled.pop(None, None)
    for mode in MODES:
        V0 = None if mode == "same" else V032
        r64 = restate_disp(mt, m0, Vt32, V0, K32, g, torch.float64)
        r32 = restate_disp(mt, m0, Vt32, V0, K32, g, torch.float32)
        naive32 = restate_disp(mt, m0, Vt32, V0, K32, g, torch.float32, naive=True)
        live_rows = r64["valid"] & ~P.zero_rows(r64["disp"])
        masks = {name: labelled[name] & live_rows for name in DEPTH_NAMES + MOTION_NAMES}
        d32 = {a: P.distance(r32[a], r64[a], r64[a], rows=True) for a in DISP_ARRAYS}
        e32 = {a: P.yardstick(masks, d32[a], FLOOR) for a in DISP_ARRAYS}
        out[mode] = {"r64": r64, "r32": r32, "naive32": naive32, "masks": masks, "d32": d32, "e32": e32, "live": live_rows}
    return out


def smallest_e32(case_mode: dict, array: str) -> torch.Tensor:
    """Per row: the smallest E32 among the regimes it carries (the GPU test checks it under each)."""
    e = torch.full((ROWS,), math.inf, dtype=torch.float64)
    for name, mask in case_mode["masks"].items():
        e = torch.where(mask, torch.minimum(e, torch.tensor(case_mode["e32"][array][name], dtype=torch.float64)), e)
    return e


def disp_mutant_caps(seed: int = 0) -> dict:
    """{(mutant, array, mode): three_quarter_cap} over the live rows."""
    c = disp_case(seed)
    caps = {}
    for mode in MODES:
        V0 = None if mode == "same" else c["V0"]
        for mutant, arrays in DISP_MUTANTS.items():
            rm = restate_disp(c["mt"], c["m0"], c["Vt"], V0, c["K"], c["g"], torch.float64, mutant)
            for a in arrays:
                r64 = c[mode]["r64"][a]
                ratios = (P.distance(rm[a], r64, r64, rows=True) / smallest_e32(c[mode], a))[c[mode]["live"]]
                caps[mutant, a, mode] = P.three_quarter_cap(ratios)
    return caps


# ---------------------------------------------------------------------------------------------------------------------
# loss

LOSS_SIZES = ((1, 1), (7, 5), (16, 16), (33, 17))  # (H, W) of the render
LOSS_DOWNSCALES = (1, 2, 4, 8)
MASK_KINDS = (None, "bool", "uint8", "float32")
LOSS_REGIMES = ("full weight", "partial weight")
LOSS_MUTANTS = {
    "missing_one_over_d": "value",  # the target is the block's mean, not the mean / d
    "weight_not_normalised": "g_pred",  # divided by the number of pixels, not by the sum of the weights
    "nan_pixel_counted": "g_pred",  # a non-finite source value taken as 0 and its block weighted as any other
}


def restate_l1(pred, flows, mask, d, dtype, mutant=None):
    """-> {"loss": 0-d, "g_pred": [H,W,2], "A": 0-d, "w": [H,W]} of ``dtype``.  ``mask`` None or [H0,W0(,1)] of any dtype."""
    assert mutant is None or mutant in LOSS_MUTANTS
    H, W, _ = pred.shape
    pred = pred.to(dtype)
    blocks = flows[: H * d, : W * d].to(dtype).reshape(H, d, W, d, 2)
    finite = torch.isfinite(blocks).all(dim=4).all(dim=3).all(dim=1)
    blocks = torch.where(torch.isfinite(blocks), blocks, torch.zeros((), dtype=dtype))
    t = blocks.sum(dim=(1, 3)) / (d * d)
    if mutant != "missing_one_over_d":
        t = t / d
    if mask is None:
        w = torch.ones(H, W, dtype=dtype)
    else:
        w = mask.reshape(mask.shape[0], mask.shape[1])[: H * d, : W * d].to(dtype).reshape(H, d, W, d).sum(dim=(1, 3)) / (d * d)
    if mutant != "nan_pixel_counted":
        w = torch.where(finite, w, torch.zeros((), dtype=dtype))
        t = torch.where(finite[..., None], t, torch.zeros((), dtype=dtype))
    diff = pred - t
    total = w.sum()
    den = 2 * torch.clamp(total, min=TINY)
    if mutant == "weight_not_normalised":
        den = torch.tensor(2.0 * H * W, dtype=dtype)
    loss = (w[..., None] * diff.abs()).sum() / den
    A = (w[..., None] * (pred.abs() + t.abs())).sum() / den
    g = torch.where(w[..., None] != 0, w[..., None] * torch.sign(diff) / den, torch.zeros((), dtype=dtype))
    return {"loss": loss, "g_pred": g, "A": A, "w": w}


@functools.lru_cache(maxsize=None)
def loss_case(H: int, W: int, d: int, mask_kind, bad: str = "some", seed: int = 0) -> dict:
    """One case: ``pred`` [H,W,2] float32, ``flows`` [H d + r, W d + r', 2] float32 with nonzero remainders at d > 1 (full-resolution
    magnitudes: a few pixels x d), the mask of ``mask_kind`` (about a fifth zero, so that blocks of partial weight occur at
    d > 1), and NaN / inf source pixels: ``bad`` = "some" (about one block in eight), "none", or "all" (every block).
    ``r64`` / ``r32``; ``masks`` of the gradient's regimes; ``e32``.  Shared: leave it unchanged."""
    gen = torch.Generator().manual_seed(3000 + seed + 7 * H + 13 * W + 101 * d + 1009 * MASK_KINDS.index(mask_kind))
    r, rp = (0, 0) if d == 1 else (1 + (H % (d - 1)), d - 1)
    H0, W0 = H * d + r, W * d + rp
    pred = torch.randn(H, W, 2, generator=gen) * 3
    flows = torch.randn(H0, W0, 2, generator=gen) * 3 * d
    if bad != "none":
        hit = torch.rand(H0, W0, generator=gen) < (1.0 if bad == "all" else 0.125 / (d * d))
        if bad == "all":  # one source pixel of every block (and the remainder rows and columns, which are never read)
            hit = torch.zeros(H0, W0, dtype=torch.bool)
            hit[d - 1 :: d, 0::d] = True
        which = torch.randint(0, 3, (H0, W0), generator=gen)
        vals = torch.tensor([math.nan, math.inf, -math.inf])[which]
        chan = torch.randint(0, 2, (H0, W0), generator=gen)
        for c in range(2):
            flows[..., c] = torch.where(hit & (chan == c), vals, flows[..., c])
    mask = None
    if mask_kind is not None:
        keep = torch.rand(H0, W0, generator=gen) < 0.8
        mask = {"bool": keep, "uint8": keep.to(torch.uint8), "float32": keep.float() * (0.25 + 0.75 * torch.rand(H0, W0, generator=gen))}[mask_kind]
        if mask_kind != "bool" and H > 1:
            mask = mask.reshape(H0, W0, 1)  # (both shapes the op takes)
    r64, r32 = restate_l1(pred, flows, mask, d, torch.float64), restate_l1(pred, flows, mask, d, torch.float32)
    w = r64["w"]
    masks = {"full weight": w == 1, "partial weight": (w != 0) & (w != 1)}
    d32 = P.distance(r32["g_pred"], r64["g_pred"], r64["g_pred"].abs())
    e32 = P.yardstick(masks, d32, FLOOR)
    v32 = float(P.distance(r32["loss"].reshape(1), r64["loss"].reshape(1), r64["A"].reshape(1))[0])
    return {"pred": pred, "flows": flows, "mask": mask, "d": d, "r64": r64, "r32": r32, "masks": masks, "e32": e32,
            "e32_value": max(v32 if math.isfinite(v32) else 0.0, FLOOR)}  # fmt: skip


def loss_cases():
    """The (H, W, d, mask kind) of every GPU case: every size at every downscale, the mask kinds going round."""
    out = []
    for i, (H, W) in enumerate(LOSS_SIZES):
        for j, d in enumerate(LOSS_DOWNSCALES):
            out.append((H, W, d, MASK_KINDS[(i + j) % len(MASK_KINDS)]))
    for kind in MASK_KINDS:  # and every mask kind at the largest size, d = 2
        if (33, 17, 2, kind) not in out:
            out.append((33, 17, 2, kind))
    return out


def loss_mutant_caps() -> dict:
    """{mutant: three_quarter_cap} over the elements each concerns, all cases together: ``missing_one_over_d`` the values of
    the cases with d > 1; ``weight_not_normalised`` the gradient elements with weight, of the cases where some pixel has less
    than full weight; ``nan_pixel_counted`` the gradient elements of the blocks that hold a non-finite value."""
    ratios = {m: [] for m in LOSS_MUTANTS}
    for H, W, d, kind in loss_cases():
        c = loss_case(H, W, d, kind)
        r64 = c["r64"]
        for mutant in LOSS_MUTANTS:
            rm = restate_l1(c["pred"], c["flows"], c["mask"], d, torch.float64, mutant)
            if mutant == "missing_one_over_d":
                if d > 1 and float(r64["w"].sum()) > 0:
                    ratios[mutant].append(P.distance(rm["loss"].reshape(1), r64["loss"].reshape(1), r64["A"].reshape(1)) / c["e32_value"])
                continue
            e = torch.full(r64["w"].shape, math.inf, dtype=torch.float64)
            for name, m in c["masks"].items():
                e = torch.where(m, torch.tensor(c["e32"][name], dtype=torch.float64), e)
            e = torch.where(torch.isinf(e), torch.tensor(FLOOR, dtype=torch.float64), e)  # (zero-weight elements: the floor)
            dist = P.distance(rm["g_pred"], r64["g_pred"], r64["g_pred"].abs()) / e[..., None]
            if mutant == "weight_not_normalised":
                if bool((r64["w"] != 1).any()):
                    ratios[mutant].append(dist[r64["w"] != 0].reshape(-1))
            else:
                blocks = c["flows"][: H * d, : W * d].reshape(H, d, W, d, 2)
                bad = ~torch.isfinite(blocks).all(dim=4).all(dim=3).all(dim=1)
                hit = bad & (rm["w"] != 0)
                ratios[mutant].append(dist[hit].reshape(-1))
    return {m: P.three_quarter_cap(torch.cat(v)) if v else 0.0 for m, v in ratios.items()}
