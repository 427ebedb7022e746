"""Plain-torch restatement of the per-Gaussian stage (csrc/preprocess.hip + csrc/project_math.h): activations, EWA
projection, SH colour, record packing -- in any dtype, differentiable by autograd.  A helper, not a test; nothing of the
package under test is imported here.  Built from ``oracle.raster_oracle`` (``project``, ``sh_eval``).

    stage(...)          radii, means2d, depths, conics and the 16-float record of every row
    regime_scene(seed)  ~200 rows drawn from named regimes (clamped, sub-pixel, culled, ...), one oblique camera
    margins(...)        how far every row is from each branch boundary of the stage
    GROUPS / cotangents one set of output gradients at a time, everything else zero
    MUTANTS             autograd-level wrong derivatives of the restatement (CPU only: they prove that the bound has teeth)

RECORD LAYOUT (include/fgraster.h).  The forward record the stage writes is fg_pack_splats':
    [x, y, opacity (x compensation when antialiased), conic a b c, colour(3) | depth | extra, 0 ...]      features from slot 6
The GRADIENT record fg_preprocess_bwd reads is fg_raster_bwd's: [v_x, v_y, v_opacity, v_conic a b c, |v_x|, |v_y|, v_f0 ...]
-- features from slot 8, xy slots ignored in favour of v_means2d.  ``stage`` returns the forward record; a test that drives the
kernel's backward translates a cotangent of the forward record into the gradient record (``to_gradient_record``), which is what
the raster backward does in production.
"""
import contextlib
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from oracle import raster_oracle as O

WIDTH, HEIGHT = 64, 48
REC = 16
FEAT0 = 6  # first feature slot of the forward record
GRAD_FEAT0 = 8  # ... of the gradient record
FLOOR = 16 * 2.0**-24  # floor of the fp32 yardstick E32
MARGIN = 1e-3  # every row is at least this far from every branch boundary (pixels, or relative to the quantity compared)
NEAR = 0.01

# The GPU bound is F * E32(regime, group, tensor).  Set from the MI355X run recorded in profiles/per_gaussian_row_parity.md:
# 4 x the worst recorded ratio (HIP row distance) / E32 = 4 x 3.87, rounded up to a power of two; capped by the host test's
# mutant assertion (every mutant is at least 4 * F * E32 away on the rows it concerns: F <= 81 on this scene).  None: record
# only.  The row distance of this family is |g - g64|_2 / |g64|_2 (tests/parity_common.py has the protocol).
F: Optional[float] = 16.0

CULLED = ("behind", "offscreen")
FORMS = ("plain", "raw", "raw_delta")
SH_DEGREES = (0, 1, 3)  # the degrees the path table uses (margins are taken at each)


# ---------------------------------------------------------------------------------------------------------------------
# the stage


class _StraightThrough(torch.autograd.Function):
    """value in the forward, the whole gradient to ``source`` in the backward: a step whose derivative is taken as 1."""

    @staticmethod
    def forward(ctx, value, source):
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        return None, g


class _TorchProxy:
    """``torch`` with a few functions replaced: what the oracle module sees while a mutant is active."""

    def __init__(self, **over):
        self._over = over

    def __getattr__(self, name):
        over = self.__dict__["_over"]
        return over[name] if name in over else getattr(torch, name)


@contextlib.contextmanager
def _oracle_sees(**over):
    if not over:
        yield
        return
    O.torch = _TorchProxy(**over)
    try:
        yield
    finally:
        O.torch = torch


def _projection_overrides(mutant):
    if mutant == "clamp_derivative":  # O._project_core: minimum(lim, maximum(-lim, x / z)) -- derivative 1 outside the limit
        return dict(maximum=lambda a, b: _StraightThrough.apply(torch.maximum(a, b), b),
                    minimum=lambda a, b: _StraightThrough.apply(torch.minimum(a, b), b))  # fmt: skip
    if mutant == "quat_projection":  # O._project_core takes four square roots, |q| first: |q| as a constant
        calls = [0]

        def sqrt(x):
            calls[0] += 1
            r = torch.sqrt(x)
            return r.detach() if calls[0] % 4 == 1 else r

        return dict(sqrt=sqrt)
    return {}


MUTANTS = ("clamp_derivative", "compensation", "quat_projection", "raw_quat_projection", "sh_mask", "view_dir_projection",
           "depth_channel")  # fmt: skip


def stage(inp: Dict[str, torch.Tensor], viewmat, K, *, form: str, sh_degree: int, antialiased: bool = False,
          with_depth: bool = False, mutant: Optional[str] = None, width: int = WIDTH, height: int = HEIGHT):  # fmt: skip
    """-> dict(radii [N] int32, means2d [N,2], depths [N], conics [N,3], record [N,16], compensations [N]).
    ``inp``: the plain inputs (means, quats, scales, opacities, colors, extra) or the raw ones (means, quats, log_scales,
    opacity_logits, features_dc, features_rest, optional d_quats / d_scales added after normalisation / exp, extra); ``colors``
    are [N,k_stored,3] SH coefficients, or [N,3] direct channels for sh_degree = -1.  Culled rows are zeros, zero gradient."""
    assert form in FORMS and mutant in (None,) + MUTANTS
    means = inp["means"]
    if form == "plain":
        quats, scales, opac, coeffs = inp["quats"], inp["scales"], inp["opacities"], inp.get("colors")
    else:
        q = inp["quats"]
        n = O._sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])[:, None]
        quats = q / (n.detach() if mutant == "raw_quat_projection" else n)
        scales = torch.exp(inp["log_scales"])
        if inp.get("d_quats") is not None:
            quats = quats + inp["d_quats"]
        if inp.get("d_scales") is not None:
            scales = scales + inp["d_scales"]
        opac = 1.0 / (1.0 + torch.exp(-inp["opacity_logits"]))
        coeffs = torch.cat([inp["features_dc"][:, None, :], inp["features_rest"]], 1)
    with _oracle_sees(**_projection_overrides(mutant)):
        proj = O.project(means, quats, scales, viewmat, K, width, height)
    visible = proj.radii > 0
    comp = proj.compensations
    if antialiased:
        opac = opac * (comp.detach() if mutant == "compensation" else comp)
    if sh_degree >= 0:
        campos = torch.linalg.inv(viewmat)[:3, 3]
        dirs = means - campos[None, :]
        safe = torch.where(visible[:, None], dirs, torch.ones_like(dirs))
        over = dict(sqrt=lambda x: torch.sqrt(x).detach()) if mutant == "view_dir_projection" else {}
        with _oracle_sees(**over):
            pre = O.sh_eval(sh_degree, safe, coeffs) + 0.5
        rgb = torch.clamp_min(pre, 0.0)
        if mutant == "sh_mask":
            rgb = _StraightThrough.apply(rgb, pre)
    else:
        rgb = coeffs
    chans = [proj.means2d, opac[:, None], proj.conics, rgb]
    if with_depth:
        chans.append((proj.depths.detach() if mutant == "depth_channel" else proj.depths)[:, None])
    if inp.get("extra") is not None:
        chans.append(inp["extra"])
    rec = torch.cat(chans, -1)
    assert rec.shape[1] <= FEAT0 + 8
    rec = torch.cat([rec, torch.zeros(rec.shape[0], REC - rec.shape[1], dtype=rec.dtype)], -1)
    rec = torch.where(visible[:, None], rec, torch.zeros_like(rec))
    return dict(radii=proj.radii, means2d=proj.means2d, depths=proj.depths, conics=proj.conics, record=rec,
                compensations=comp)  # fmt: skip


# ---------------------------------------------------------------------------------------------------------------------
# the regime scene


@dataclass
class RegimeScene:
    raw: Dict[str, torch.Tensor]  # fp32: means, quats, log_scales, opacity_logits, features_dc [N,3], features_rest [N,15,3],
    #                               d_quats, d_scales, direct [N,3], extra [N,2]
    viewmat: torch.Tensor  # [4,4] fp32
    K: torch.Tensor  # [3,3] fp32
    labels: List[str]
    width: int = WIDTH
    height: int = HEIGHT

    def rows(self, *regimes) -> torch.Tensor:
        return torch.tensor([i for i, l in enumerate(self.labels) if l in regimes], dtype=torch.long)

    def take(self, idx) -> "RegimeScene":
        """The rows ``idx`` (a slice or an index tensor; repeats allowed): every row of the stage stands alone."""
        if isinstance(idx, slice):
            idx = torch.arange(len(self.labels))[idx]
        return RegimeScene({k: v[idx].contiguous() for k, v in self.raw.items()}, self.viewmat, self.K,
                           [self.labels[int(i)] for i in idx], self.width, self.height)  # fmt: skip

    def inputs(self, form: str, sh_degree: int, k_stored: int, n_extra: int, dtype=torch.float32) -> Dict[str, torch.Tensor]:
        """The input tensors of a path, in call order; fp32 values (cast to ``dtype``): the float64 reference sees the very
        numbers the kernel sees."""
        r = self.raw
        extra = r["extra"][:, :n_extra].contiguous() if n_extra else None
        if form == "plain":
            coeffs = torch.cat([r["features_dc"][:, None, :], r["features_rest"]], 1)
            d = dict(means=r["means"], quats=r["quats"], scales=torch.exp(r["log_scales"]),
                     opacities=torch.sigmoid(r["opacity_logits"]),
                     colors=r["direct"] if sh_degree < 0 else coeffs[:, :k_stored].contiguous(), extra=extra)  # fmt: skip
        else:
            assert sh_degree >= 0
            d = dict(means=r["means"], quats=r["quats"], log_scales=r["log_scales"], opacity_logits=r["opacity_logits"],
                     features_dc=r["features_dc"], features_rest=r["features_rest"][:, : k_stored - 1].contiguous())  # fmt: skip
            if form == "raw_delta":
                d.update(d_quats=r["d_quats"], d_scales=r["d_scales"])
            d["extra"] = extra
        return {k: v.detach().clone().to(dtype) for k, v in d.items() if v is not None}


COUNTS = dict(ordinary=40, clamp_x=16, clamp_y=16, clamp_xy=16, near_limit=16, subpixel=16, sh_clamped=24, saturated=16,
              behind=16, offscreen=16)  # fmt: skip
VISIBLE_REGIMES = tuple(k for k in COUNTS if k not in CULLED)


def camera():
    """One camera that is not axis-aligned: 64 x 48, non-square focal lengths, off-centre principal point."""
    q = torch.tensor([[0.9, 0.25, -0.3, 0.18]], dtype=torch.float64)
    vm = torch.eye(4, dtype=torch.float64)
    vm[:3, :3] = O.quat_to_rotmat(q)[0]
    vm[:3, 3] = torch.tensor([0.3, -0.2, 0.5], dtype=torch.float64)
    K = torch.tensor([[70.0, 0.0, 30.5], [0.0, 55.0, 25.25], [0.0, 0.0, 1.0]])
    return vm.float(), K


def regime_scene(seed: int = 0) -> RegimeScene:
    g = torch.Generator().manual_seed(seed)
    vm, K = camera()
    fx, fy = float(K[0, 0]), float(K[1, 1])
    tanx, tany = 0.5 * WIDTH / fx, 0.5 * HEIGHT / fy
    limx, limy = O.FOV_CLAMP * tanx, O.FOV_CLAMP * tany

    def U(n, lo, hi):
        return lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)

    def logU(n, lo, hi):
        return torch.exp(U(n, float(torch.log(torch.tensor(lo))), float(torch.log(torch.tensor(hi)))))

    def sign(n):
        return torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()

    def axes(f):  # three per-axis scale factors
        return torch.stack([f(), f(), f()], -1)

    parts, labels = [], []
    for name, n in COUNTS.items():
        rx, ry, z = U(n, -0.8, 0.8) * tanx, U(n, -0.8, 0.8) * tany, U(n, 2.0, 8.0)
        s = z[:, None] * axes(lambda: logU(n, 0.01, 0.08))  # 0.7 .. 5.6 px
        if name in ("clamp_x", "clamp_xy"):
            rx = sign(n) * U(n, 1.05, 1.6) * limx
        if name in ("clamp_y", "clamp_xy"):
            ry = sign(n) * U(n, 1.05, 1.6) * limy
        if name.startswith("clamp"):
            z = U(n, 2.0, 6.0)
            s = z[:, None] * axes(lambda: U(n, 0.3, 0.5))  # large enough to reach back into the image
            if name == "clamp_x":
                ry = U(n, -0.7, 0.7) * tany
            if name == "clamp_y":
                rx = U(n, -0.7, 0.7) * tanx
        if name == "near_limit":  # 0.9 .. 0.998 of the limit in x, in y, or in both
            which = torch.arange(n) % 3
            nx, ny = sign(n) * U(n, 0.9, 0.998) * limx, sign(n) * U(n, 0.9, 0.998) * limy
            rx = torch.where(which != 1, nx, U(n, -0.7, 0.7) * tanx)
            ry = torch.where(which != 0, ny, U(n, -0.7, 0.7) * tany)
            s = z[:, None] * axes(lambda: U(n, 0.1, 0.25))
        if name == "subpixel":  # compensation ~ s1 s2 / 0.3 (px^2): 3e-4 .. 6e-3
            z = U(n, 2.0, 6.0)
            sigma = torch.sqrt(0.3 * logU(n, 3e-4, 6e-3))
            s = (sigma * z / (fx * fy) ** 0.5)[:, None] * axes(lambda: U(n, 0.85, 1.18))
        if name == "behind":
            rx, ry, z = U(n, -0.5, 0.5), U(n, -0.5, 0.5), -U(n, 0.5, 5.0)
        if name == "offscreen":
            which = torch.arange(n) % 2
            rx = torch.where(which == 0, sign(n) * U(n, 2.0, 3.0) * tanx, rx)
            ry = torch.where(which == 1, sign(n) * U(n, 2.0, 3.0) * tany, ry)
            s = z[:, None] * axes(lambda: U(n, 0.005, 0.02))
        pc = torch.stack([rx * z, ry * z, z], -1)
        means = (pc - vm[:3, 3].double()[None, :]) @ vm[:3, :3].double()  # R^T (pc - t)
        q = torch.randn(n, 4, generator=g, dtype=torch.float64)
        q = q / q.norm(dim=1, keepdim=True) * logU(n, 0.2, 5.0)[:, None]
        logit = U(n, -2.0, 3.0)
        rel = U(n, -0.05, 0.05)[:, None] * torch.ones(n, 3, dtype=torch.float64)
        dc = U(3 * n, 0.0, 2.0).reshape(n, 3)
        if name == "saturated":  # opacity logits of +-12, log-scale deltas of both signs
            logit = sign(n) * 12.0
            rel = (sign(3 * n) * U(3 * n, 0.1, 0.3)).reshape(n, 3)
        if name == "sh_clamped":  # one, two or three channels below -0.5 before the offset
            k = torch.arange(n) % 3 + 1
            first = torch.arange(n) // 3 % 3
            chan = (torch.arange(3)[None, :] - first[:, None]) % 3
            dc = torch.where(chan < k[:, None], -U(3 * n, 4.0, 6.0).reshape(n, 3), dc)
        parts.append(dict(
            means=means, quats=q, log_scales=torch.log(s), opacity_logits=logit, features_dc=dc,
            features_rest=U(45 * n, -0.08, 0.08).reshape(n, 15, 3), d_quats=U(4 * n, -0.1, 0.1).reshape(n, 4),
            d_scales=rel * s, direct=U(3 * n, 0.0, 1.0).reshape(n, 3),
            extra=torch.randn(n, 2, generator=g, dtype=torch.float64)))  # fmt: skip
        labels += [name] * n
    perm = torch.randperm(len(labels), generator=g)  # regimes interleave within a 64-row workgroup
    raw = {k: torch.cat([p[k] for p in parts])[perm].float().contiguous() for k in parts[0]}
    return RegimeScene(raw, vm, K, [labels[int(i)] for i in perm])


# ---------------------------------------------------------------------------------------------------------------------
# branch margins


def margins(scene: RegimeScene, form: str) -> Dict[str, torch.Tensor]:
    """-> name -> [N] float64: the distance of every row from each branch boundary of the stage (pixels, or relative to the
    quantity compared; colour units for the SH clamp), +inf where the boundary does not decide the row.  A culled row is
    decided by its cull alone (``cull``: the widest margin among the comparisons that cull it; an off-screen comparison
    gives one pixel away, the most a knife-edge radius could move it); a visible row by all of them:

        near        z against the near plane                                   (relative)
        left right top bottom   the four off-screen comparisons                (pixels)
        ceil        3 sqrt(v1) against the integers around it                  (pixels)
        clamp_x clamp_y   |x/z|, |y/z| against 1.3 x the tangent of the half field of view   (relative)
        disc        b*b - det against the 0.01 floor                           (relative)
        sh<deg>     min over channels of |sh + 0.5| at SH degrees 0, 1, 3 (SH paths)
    z <= far (1e10) and det > 0 (the blurred determinant is at least 0.09) are never near."""
    inp = scene.inputs(form, 3, 16, 0, torch.float64)
    vm, K = scene.viewmat.double(), scene.K.double()
    inf = torch.tensor(float("inf"), dtype=torch.float64)
    with torch.no_grad():
        if form == "plain":
            quats, scales = inp["quats"], inp["scales"]
            coeffs = inp["colors"]
        else:
            quats = inp["quats"] / inp["quats"].norm(dim=1, keepdim=True) + inp.get("d_quats", 0.0)
            scales = torch.exp(inp["log_scales"]) + inp.get("d_scales", 0.0)
            coeffs = torch.cat([inp["features_dc"][:, None, :], inp["features_rest"]], 1)
        m2x, m2y, z, ca, cb, cc, _, det, r = O._project_core(inp["means"], quats, scales, vm, K, scene.width, scene.height,
                                                            O.EPS2D)  # fmt: skip
        W, H = float(scene.width), float(scene.height)
        c00, c01, c11 = cc * det, -cb * det, ca * det
        b = 0.5 * (c00 + c11)
        disc = b * b - det
        r_raw = 3.0 * torch.sqrt(b + torch.sqrt(torch.clamp_min(disc, 0.01)))
        pc = inp["means"] @ vm[:3, :3].T + vm[:3, 3][None, :]
        limx, limy = O.FOV_CLAMP * 0.5 * W / K[0, 0], O.FOV_CLAMP * 0.5 * H / K[1, 1]
        out = dict(
            near=(z - NEAR).abs() / torch.clamp_min(z.abs(), NEAR),
            left=(m2x + r).abs(), right=(m2x - r - W).abs(), top=(m2y + r).abs(), bottom=(m2y - r - H).abs(),
            ceil=torch.minimum(r_raw - torch.floor(r_raw), torch.ceil(r_raw) - r_raw),
            clamp_x=((pc[:, 0] / pc[:, 2]).abs() / limx - 1.0).abs(), clamp_y=((pc[:, 1] / pc[:, 2]).abs() / limy - 1.0).abs(),
            disc=(disc - 0.01).abs() / 0.01)  # fmt: skip
        campos = torch.linalg.inv(vm)[:3, 3]
        for deg in SH_DEGREES:
            out[f"sh{deg}"] = (O.sh_eval(deg, inp["means"] - campos[None, :], coeffs) + 0.5).abs().min(dim=1).values
        behind = z < NEAR
        off = dict(left=m2x + r <= 0, right=m2x - r >= W, top=m2y + r <= 0, bottom=m2y - r >= H)
        culled = behind | off["left"] | off["right"] | off["top"] | off["bottom"]
        cull = torch.where(behind, out["near"], -inf)
        for k, hit in off.items():
            cull = torch.maximum(cull, torch.where(hit & ~behind, out[k] - 1.0, -inf))
        out = {k: torch.where(culled, inf, v) for k, v in out.items()}
        out["cull"] = torch.where(culled, cull, inf)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cotangent groups

GROUPS = ("means2d", "xy", "depths", "depth_channel", "conics_out", "conics_rec", "opacity", "colour", "extra", "all")


def record_slots(with_depth: bool, n_extra: int) -> Dict[str, List[int]]:
    """Slots of the FORWARD record per cotangent group (three colour channels on every path)."""
    s = dict(xy=[0, 1], opacity=[2], conics_rec=[3, 4, 5], colour=[6, 7, 8])
    if with_depth:
        s["depth_channel"] = [9]
    if n_extra:
        s["extra"] = list(range(9 + int(with_depth), 9 + int(with_depth) + n_extra))
    return s


def groups_of(with_depth: bool, n_extra: int) -> List[str]:
    slots = record_slots(with_depth, n_extra)
    return [g for g in GROUPS if g in ("means2d", "depths", "conics_out", "all") or g in slots]


def cotangents(n: int, group: str, with_depth: bool, n_extra: int, seed: int = 0) -> Dict[str, torch.Tensor]:
    """-> the output gradients of a group, float64, keyed by output (means2d, depths, conics, record); outputs the group
    does not drive are ABSENT (no gradient arrives for them).  The same random numbers whatever the group."""
    g = torch.Generator().manual_seed(1000 + seed)
    full = dict(means2d=torch.randn(n, 2, generator=g, dtype=torch.float64),
                depths=torch.randn(n, generator=g, dtype=torch.float64),
                conics=torch.randn(n, 3, generator=g, dtype=torch.float64),
                record=torch.randn(n, REC, generator=g, dtype=torch.float64))  # fmt: skip
    slots = record_slots(with_depth, n_extra)
    used = sorted(i for v in slots.values() for i in v)
    if group == "all":
        rec = torch.zeros_like(full["record"])
        rec[:, used] = full["record"][:, used]
        return dict(full, record=rec)
    direct = dict(means2d="means2d", depths="depths", conics_out="conics")
    if group in direct:
        return {direct[group]: full[direct[group]]}
    rec = torch.zeros_like(full["record"])
    rec[:, slots[group]] = full["record"][:, slots[group]]
    return dict(record=rec)


def to_gradient_record(v_record: torch.Tensor) -> torch.Tensor:
    """A cotangent of the forward record as the gradient record the raster backward hands fg_preprocess_bwd: features move
    from slot 6 to slot 8, slots 6-7 (absgrad) stay zero; the xy slots are where v_means2d points."""
    g = torch.zeros_like(v_record)
    g[:, :FEAT0] = v_record[:, :FEAT0]
    g[:, GRAD_FEAT0:] = v_record[:, FEAT0 : REC - 2]
    return g


# ---------------------------------------------------------------------------------------------------------------------
# gradients


def gradients(scene: RegimeScene, path: dict, dtype, groups=None, mutant=None, pose: bool = False, seed: int = 0):
    """-> (outs, {group: {tensor: grad}}): one forward of the restatement in ``dtype``, one backward per cotangent group.
    ``path``: form, sh_degree, k_stored, antialiased, with_depth, n_extra.  Gradients that autograd leaves out are zeros.
    ``pose``: the camera pose takes a gradient too (key "viewmat", [4,4])."""
    inp = scene.inputs(path["form"], path["sh_degree"], path["k_stored"], path["n_extra"], dtype)
    for v in inp.values():
        v.requires_grad_(True)
    vm = scene.viewmat.to(dtype).clone().requires_grad_(pose)
    outs = stage(inp, vm, scene.K.to(dtype), form=path["form"], sh_degree=path["sh_degree"], antialiased=path["antialiased"],
                 with_depth=path["with_depth"], mutant=mutant, width=scene.width, height=scene.height)  # fmt: skip
    wrt = dict(inp, viewmat=vm) if pose else inp
    res = {}
    for group in groups or groups_of(path["with_depth"], path["n_extra"]):
        ct = cotangents(len(scene.labels), group, path["with_depth"], path["n_extra"], seed)
        loss = sum((outs[k] * v.to(dtype)).sum() for k, v in ct.items())
        gs = torch.autograd.grad(loss, list(wrt.values()), retain_graph=True, allow_unused=True)
        res[group] = {k: (torch.zeros_like(t) if g is None else g) for (k, t), g in zip(wrt.items(), gs)}
    return {k: v.detach() for k, v in outs.items()}, res


def vector_distance(g: torch.Tensor, g64: torch.Tensor) -> float:
    g, g64 = g.detach().cpu().double().reshape(-1), g64.double().reshape(-1)
    return float((g - g64).norm() / g64.norm())


# The path table: every value of every column at least twice (form; sh_degree -1 = three direct colours; k_stored
# (deg+1)^2 and 16; antialiased; with_depth; n_extra 0 and 2; note = backward from the forward's SH note / from the rows).
def _p(form, sh_degree, k_stored, antialiased, with_depth, n_extra, note):
    return dict(form=form, sh_degree=sh_degree, k_stored=k_stored, antialiased=bool(antialiased), with_depth=bool(with_depth),
                n_extra=n_extra, note=bool(note))  # fmt: skip


PATHS = {
    "plain-direct": _p("plain", -1, 0, 0, 0, 0, 1),
    "plain-direct-aa-depth-extra": _p("plain", -1, 0, 1, 1, 2, 0),
    "plain-sh0-k1-depth": _p("plain", 0, 1, 0, 1, 0, 1),
    "plain-sh0-k16-aa-extra-rows": _p("plain", 0, 16, 1, 0, 2, 0),
    "plain-sh1-k4-aa-depth": _p("plain", 1, 4, 1, 1, 0, 1),
    "plain-sh1-k16-extra-rows": _p("plain", 1, 16, 0, 0, 2, 0),
    "plain-sh3-depth-extra": _p("plain", 3, 16, 0, 1, 2, 1),
    "plain-sh3-aa-rows": _p("plain", 3, 16, 1, 0, 0, 0),
    "raw-sh0-k1-aa-depth-extra": _p("raw", 0, 1, 1, 1, 2, 1),
    "raw-sh1-k4-rows": _p("raw", 1, 4, 0, 0, 0, 0),
    "raw-sh3-aa-depth-extra": _p("raw", 3, 16, 1, 1, 2, 1),
    "delta-sh1-k16-aa-extra": _p("raw_delta", 1, 16, 1, 0, 2, 1),
    "delta-sh3-depth-rows": _p("raw_delta", 3, 16, 0, 1, 0, 0),
    "delta-sh0-k16-aa-depth-extra-rows": _p("raw_delta", 0, 16, 1, 1, 2, 0),
}
