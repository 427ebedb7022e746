"""Plain-torch restatement of the compositing stage (csrc/raster.hip: fg_pack_splats, fg_raster_fwd, fg_raster_bwd,
fg_unpack_grads) in any dtype, on one tiny image with explicit lists.  A helper, not a test; nothing of the package under
test is imported here.  Written from ``oracle.raster_oracle`` (``_tile_terms``, ``_composite_state`` and the algebra of
``rasterize_backward(alpha_out=...)``: the reference's walk-back semantics, T rebuilt from ``1 - alpha_out``).

    regime_scene(seed)   2-D splats drawn from named regimes (faint, sub-pixel, needle, deep list, wall, ...), 72 x 40 pixels
    margins(scene)       how far every pixel is from each decision of its walk; which pixels are KEPT
    composite(...)       render, alpha, last_ids (+ the per-pixel weight sum the render yardstick divides by)
    backward(...)        the five gradients and, beside each, its ABSOLUTE ACCUMULATION (every per-pixel term by magnitude)
    cotangents(...)      one cotangent group at a time (render / alpha / both), zero on excluded pixels
    MUTANTS              wrong restatements (float64, CPU only: they prove that the bound has teeth)
    composite_scene, epilogue, epilogue_backward, EPILOGUE_CASES, epilogue_gradients
                         the post-composite folded into the kernels (``Composite``: background, clamp, clamp mask)

ROW DISTANCE.  |g - g64|_2 / |A64|_2 over a row's columns, A the absolute accumulation of the same tensor (for ``means2d``
that is absgrad itself).  A gradient row is a signed sum over pixels that cancels, and the kernel's float atomics arrive in
a varying order: both act at the scale of A, not of |g|.  With |g64| as the denominator the yardstick would be decided by
whichever row happens to cancel best.  tests/parity_common.py has the protocol.

LISTS.  The raster takes its lists as given: they are built with ``O.isect_tiles`` / ``O.isect_offsets`` from radii chosen
per regime (generous for most; the deep, wall and occluded rows' boxes stay inside their one tile) and the deep tile's list
leaves out the rows of the regimes with high opacities (DENSE_REGIMES), so that it is long and its pixels never stop.

MUTANTS (``mutant=`` of ``composite`` / ``backward``):
    clamp_passes_gradient   opacity * vis > 0.999 still feeds g_sigma and g_opacity
    stop_entry_composited   the entry that brings T to <= 1e-4 is composited instead of dropped -- and so is every later
                            entry, each of which brings T to <= 1e-4 as well (the stop rule drops nothing: the forward changes)
    suffix_includes_self    the suffix sum S_i includes the entry's own term
    conic_b_halved          the conic-b gradient is halved
    absgrad_abs_of_sum      absgrad is |sum over a tile's pixels| instead of the sum of magnitudes
of ``epilogue`` / ``epilogue_backward``:
    blocked_channel_passes_gradient          a channel clamped at a bound keeps its cotangent
    background_missing_from_alpha_gradient   the alpha cotangent lacks - sum_c v[c] * background[c]
    mask_bit_of_next_channel                 channel c is blocked by the mask bit of channel c + 1
    clamp_reaches_channel_n_clamp            the clamp (and its mask bit) covers channel n_clamp as well

EXCLUDED PIXELS.  A pixel one of whose decisions (alpha against 1/255 and 0.999, sigma against 0, T against 1e-4) lies within
rounding of its threshold may legitimately take the other branch under another exp(): it is excluded -- not compared in the
forward, and its cotangents are zero.  The backward is linear in every pixel's cotangents, so an excluded pixel drops out
of every gradient on both sides, whatever the kernel did there.  The composite epilogue adds one decision, a clamped channel's
value against 0 and against 1: a pixel within CLAMP_MARGIN (absolute) of either is excluded in the same way.
"""
from dataclasses import dataclass, replace
from typing import Dict, List, Optional

import torch

import parity_common as P
from oracle import raster_oracle as O

WIDTH, HEIGHT, TILE = 72, 40, 16
TILE_W, TILE_H = 5, 3  # partial tiles on the right (8 columns) and at the bottom (8 rows)
DEEP_TILE = 1 * TILE_W + 1  # the tile that holds the deep list
WALL_TILE = 1 * TILE_W + 3  # the tile that holds the wall
FLOOR = 16 * 2.0**-24  # floor of the fp32 yardstick E32
ALPHA_MARGIN = 1e-4  # relative distance of opacity * exp(-sigma) from 1/255 and from 0.999
SIGMA_MARGIN = 1e-4  # absolute distance of sigma from 0
T_MARGIN = 1e-3  # relative distance of T from 1e-4
CLAMP_MARGIN = 1e-4  # absolute distance of a clamped channel's value from 0 and from 1 (the composite epilogue)
SEED = 2  # the scene the tests use (tests/test_raster_rows_host.py checks its exclusions)

# The GPU bound is F * E32(regime, group, tensor) -- E32(pixel class) in the forward.  Set from the MI355X run recorded in
# profiles/raster_row_parity.md: 4 x the worst recorded ratio (HIP distance) / E32 = 4 x 1.73, rounded up to a power of two;
# capped by the host test's mutant assertion (every wrong restatement is at least 4 * F * E32 away on three quarters of the
# rows it concerns: F <= 21 on this scene).  None: record only (how the run F was set from was made).
F: Optional[float] = 8.0

TENSORS = ("means2d", "absgrad", "conics", "features", "opacities")
GROUPS = ("render", "alpha", "both")
PIXEL_CLASSES = ("partial", "deep", "wall", "other")
COUNTS = dict(plain=40, opaque=12, faint=12, barely=12, subpixel=12, huge=6, needle=12, edge=12, deep=300, wall=14,
              occluded=8, indefinite=6)  # fmt: skip
DENSE_REGIMES = ("plain", "opaque", "needle", "edge", "indefinite")  # (left out of the deep tile's list)
MUTANTS = ("clamp_passes_gradient", "stop_entry_composited", "suffix_includes_self", "conic_b_halved", "absgrad_abs_of_sum",
           "blocked_channel_passes_gradient", "background_missing_from_alpha_gradient", "mask_bit_of_next_channel",
           "clamp_reaches_channel_n_clamp")  # fmt: skip


# ---------------------------------------------------------------------------------------------------------------------
# the regime scene


@dataclass
class RegimeScene:
    means2d: torch.Tensor  # [N,2] fp32
    conics: torch.Tensor  # [N,3] fp32 (a, b, c)
    opacities: torch.Tensor  # [N] fp32
    depths: torch.Tensor  # [N] fp32
    radii: torch.Tensor  # [N] int32: what the lists are built from, nothing else
    colours: torch.Tensor  # [N,8] fp32
    labels: List[str]
    offsets: torch.Tensor  # [n_tiles + 1] int32
    flatten_ids: torch.Tensor  # [I] int32
    width: int = WIDTH
    height: int = HEIGHT

    def rows(self, *regimes) -> torch.Tensor:
        return torch.tensor([i for i, l in enumerate(self.labels) if l in regimes], dtype=torch.long)

    def features(self, channels: int) -> torch.Tensor:
        return self.colours[:, :channels].contiguous()

    def take(self, idx) -> "RegimeScene":
        """The rows ``idx`` with their lists rebuilt (compositing couples rows: a sub-scene has its own reference)."""
        idx = torch.as_tensor(idx, dtype=torch.long)
        return with_lists(self.means2d[idx], self.conics[idx], self.opacities[idx], self.depths[idx], self.radii[idx],
                          self.colours[idx], [self.labels[int(i)] for i in idx], self.width, self.height)  # fmt: skip

    def without_lists(self) -> "RegimeScene":
        """The same rows, every tile list empty (I = 0)."""
        n_tiles = ((self.width + TILE - 1) // TILE) * ((self.height + TILE - 1) // TILE)
        return RegimeScene(self.means2d, self.conics, self.opacities, self.depths, self.radii, self.colours, self.labels,
                           torch.zeros(n_tiles + 1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), self.width,
                           self.height)  # fmt: skip


def with_lists(means2d, conics, opacities, depths, radii, colours, labels, width=WIDTH, height=HEIGHT) -> RegimeScene:
    tw, th = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    _, keys, vals = O.isect_tiles(means2d, radii, depths, TILE, tw, th)
    # the lists are given, not derived: the deep tile's leaves out the rows of the regimes with opacities above 0.25, so that
    # none of its pixels comes near the transmittance stop
    dense = torch.tensor([l in DENSE_REGIMES for l in labels], dtype=torch.bool)
    keep = ~(((keys >> 32) == DEEP_TILE) & dense[vals.long()])
    keys, vals = keys[keep], vals[keep]
    offsets = O.isect_offsets(keys, tw * th)
    cont = lambda t: t.contiguous()  # noqa: E731
    return RegimeScene(cont(means2d), cont(conics), cont(opacities), cont(depths), cont(radii), cont(colours), list(labels),
                       offsets, vals.contiguous(), width, height)  # fmt: skip


def conic_of(sx, sy, rho):
    """The inverse of the covariance [[sx^2, rho sx sy], [rho sx sy, sy^2]] as (a, b, c)."""
    k = 1.0 / (1.0 - rho * rho)
    return torch.stack([k / (sx * sx), -rho * k / (sx * sy), k / (sy * sy)], -1)


def regime_scene(seed: int = SEED) -> RegimeScene:
    g = torch.Generator().manual_seed(seed)
    W, H = float(WIDTH), float(HEIGHT)

    def U(n, lo, hi):
        return lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)

    def sign(n):
        return torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()

    def tile_box(tile, inset):
        ty, tx = divmod(tile, TILE_W)
        return tx * TILE + inset, (tx + 1) * TILE - inset, ty * TILE + inset, (ty + 1) * TILE - inset

    def inside_tile(n, tile, inset):
        x0, x1, y0, y1 = tile_box(tile, inset)
        return torch.stack([U(n, x0, x1), U(n, y0, y1)], -1)

    def radius_within(xy, tile):  # the largest integer radius whose box stays inside the tile: the row is in ONE list
        x0, x1, y0, y1 = tile_box(tile, 0)
        d = torch.stack([xy[:, 0] - x0, x1 - xy[:, 0], xy[:, 1] - y0, y1 - xy[:, 1]], -1).min(dim=1).values
        return torch.floor(d).clamp_min(1.0)

    parts, labels = [], []
    for name, n in COUNTS.items():
        xy = torch.stack([U(n, 2.0, W - 2.0), U(n, 2.0, H - 2.0)], -1)
        sx, sy, rho = U(n, 1.5, 5.0), U(n, 1.5, 5.0), U(n, -0.6, 0.6)
        op, depth = U(n, 0.3, 0.8), U(n, 1.0, 10.0)
        radius = None
        if name == "opaque":
            # the mean 0.02 .. 0.033 sigma (per axis) from a pixel centre: sigma = 1.5e-4 .. 7.8e-4 there, so exp(-sigma) is
            # above 0.999 by more than the margin at that pixel and below it at every other
            op = torch.ones(n, dtype=torch.float64)
            sx, sy, rho = U(n, 2.5, 6.0), U(n, 2.5, 6.0), U(n, -0.3, 0.3)
            ang, r = U(n, 0.0, 6.2831853), U(n, 0.02, 0.033)
            xy = torch.floor(xy) + 0.5 + torch.stack([r * sx * torch.cos(ang), r * sy * torch.sin(ang)], -1)
        if name == "faint":  # below 1/255 = 0.00392 everywhere
            op = U(n, 0.002, 0.0037)
        if name == "barely":  # alpha >= 1/255 up to sigma = ln(255 o) = 0.24 .. 1.6: a few pixels each
            op = U(n, 0.005, 0.02)
            sx, sy = U(n, 1.5, 3.0), U(n, 1.5, 3.0)
        if name == "subpixel":
            sx, sy, rho = U(n, 0.2, 0.45), U(n, 0.2, 0.45), U(n, -0.3, 0.3)
        if name == "huge":  # every tile: the atomics of a row arrive from all workgroups
            sx, sy, rho, op = U(n, 40.0, 90.0), U(n, 40.0, 90.0), U(n, -0.3, 0.3), U(n, 0.05, 0.2)
        if name == "needle":  # long in x or in y
            long_, short = U(n, 8.0, 20.0), U(n, 0.3, 0.6)
            along_x = torch.arange(n) % 2 == 0
            sx, sy = torch.where(along_x, long_, short), torch.where(along_x, short, long_)
            rho = sign(n) * U(n, 0.5, 0.95)
        if name == "edge":  # centres 1 .. 6 px outside the left and the right border
            out = U(n, 1.0, 6.0)
            xy[:, 0] = torch.where(torch.arange(n) % 2 == 0, -out, W + out)
            sx, sy = U(n, 2.0, 5.0), U(n, 2.0, 5.0)
        if name == "deep":  # one list of more than 256 entries that does not reach the transmittance stop
            xy = inside_tile(n, DEEP_TILE, 2.0)
            sx, sy, rho, op = U(n, 3.0, 8.0), U(n, 3.0, 8.0), U(n, -0.4, 0.4), U(n, 0.01, 0.03)
            radius = radius_within(xy, DEEP_TILE)
        if name == "wall":  # nearest of all; covers its whole tile at nearly its peak alpha
            xy = inside_tile(n, WALL_TILE, 5.0)
            sx, sy, rho, op = U(n, 25.0, 40.0), U(n, 25.0, 40.0), U(n, -0.3, 0.3), U(n, 0.85, 0.95)
            depth = U(n, 0.1, 0.2)
            radius = radius_within(xy, WALL_TILE)
        if name == "occluded":  # farthest of all, behind the wall: never reached
            xy = inside_tile(n, WALL_TILE, 2.0)
            sx, sy = U(n, 1.0, 2.5), U(n, 1.0, 2.5)
            depth = U(n, 100.0, 200.0)
            radius = radius_within(xy, WALL_TILE)
        con = conic_of(sx, sy, rho)
        if name == "indefinite":  # b^2 > a c: sigma < 0 in two opposite sectors of the footprint
            a, c = U(n, 0.03, 0.06), U(n, 0.03, 0.06)
            con = torch.stack([a, sign(n) * torch.sqrt(a * c) * U(n, 1.15, 1.5), c], -1)
            xy = torch.stack([U(n, 10.0, W - 10.0), U(n, 8.0, H - 8.0)], -1)
            op = U(n, 0.3, 0.6)
            radius = torch.full((n,), 14.0, dtype=torch.float64)
        if radius is None:  # generous: 3.5 sigma of the longer marginal and a pixel
            radius = torch.ceil(3.5 * torch.maximum(sx, sy)) + 1.0
        parts.append(dict(means2d=xy, conics=con, opacities=op, depths=depth, radii=radius, colours=U(8 * n, 0.0, 1.0).reshape(n, 8)))
        labels += [name] * n
    perm = torch.randperm(len(labels), generator=g)  # regimes interleave in the row order (the lists are by depth)
    cat = {k: torch.cat([p[k] for p in parts])[perm] for k in parts[0]}
    return with_lists(cat["means2d"].float(), cat["conics"].float(), cat["opacities"].float(), cat["depths"].float(),
                      cat["radii"].to(torch.int32), cat["colours"].float(), [labels[int(i)] for i in perm])  # fmt: skip


# ---------------------------------------------------------------------------------------------------------------------
# the walk of one tile


def _tiles(scene: RegimeScene):
    tw = (scene.width + TILE - 1) // TILE
    th = (scene.height + TILE - 1) // TILE
    for t in range(tw * th):
        s, e = int(scene.offsets[t]), int(scene.offsets[t + 1])
        ty, tx = divmod(t, tw)
        y0, x0 = ty * TILE, tx * TILE
        yield t, s, e, y0, min(y0 + TILE, scene.height), x0, min(x0 + TILE, scene.width)


def _pixel_centres(y0, y1, x0, x1, dtype):
    yy, xx = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
    return xx.reshape(-1).to(dtype) + 0.5, yy.reshape(-1).to(dtype) + 0.5


def _walk(px, py, xy, con, op, mutant=None):
    """sigma, alpha, validity and the include / stop decisions of [P] pixels over [L] list entries."""
    dx, dy, sigma, alpha, valid = O._tile_terms(px, py, xy, con, op)
    a, T_excl, include, stopped = O._composite_state(alpha, valid)
    if mutant == "stop_entry_composited":
        # the stop rule drops nothing: the entry that brings T to <= 1e-4 is composited -- and so is every later one, each
        # of which brings T to <= 1e-4 as well
        include = valid
    return dx, dy, sigma, a, T_excl, include, stopped


def pixel_class() -> torch.Tensor:
    """[H,W] long: index into PIXEL_CLASSES."""
    cls = torch.full((HEIGHT, WIDTH), PIXEL_CLASSES.index("other"), dtype=torch.long)
    cls[(HEIGHT // TILE) * TILE :, :] = PIXEL_CLASSES.index("partial")
    cls[:, (WIDTH // TILE) * TILE :] = PIXEL_CLASSES.index("partial")
    for tile, name in ((DEEP_TILE, "deep"), (WALL_TILE, "wall")):
        ty, tx = divmod(tile, TILE_W)
        cls[ty * TILE : (ty + 1) * TILE, tx * TILE : (tx + 1) * TILE] = PIXEL_CLASSES.index(name)
    return cls


# ---------------------------------------------------------------------------------------------------------------------
# margins


def margins(scene: RegimeScene) -> Dict[str, torch.Tensor]:
    """float64, per pixel: the smallest distance, over the list entries the pixel's walk EVALUATES (everything up to and
    including the entry that stops it), of
        skip    opacity * exp(-sigma) from 1/255      (relative; entries with sigma >= 0)
        clamp   opacity * exp(-sigma) from 0.999      (relative; entries with sigma >= 0)
        stop    T behind the entry from 1e-4          (relative; valid entries)
        sigma   sigma from 0                          (absolute)
    each [H,W], +inf where nothing is evaluated; ``kept`` [H,W] bool: skip, clamp >= ALPHA_MARGIN, sigma >= SIGMA_MARGIN and
    stop >= T_MARGIN; ``evaluated`` / ``contributing``: tile -> [P,L] bool."""
    inf = float("inf")
    out = {k: torch.full((scene.height, scene.width), inf, dtype=torch.float64) for k in ("skip", "clamp", "stop", "sigma")}
    evaluated, contributing = {}, {}
    m2, con, op = scene.means2d.double(), scene.conics.double(), scene.opacities.double()
    for t, s, e, y0, y1, x0, x1 in _tiles(scene):
        if e <= s:
            continue
        ids = scene.flatten_ids[s:e].long()
        px, py = _pixel_centres(y0, y1, x0, x1, torch.float64)
        _, _, sigma, a, _, include, stopped = _walk(px, py, m2[ids], con[ids], op[ids])
        valid = a > 0
        T_incl = torch.cumprod(1.0 - a, dim=1)
        stop = valid & (T_incl <= O.T_STOP)
        ev = (torch.cumsum(stop.to(torch.int32), dim=1) - stop.to(torch.int32)) == 0  # nothing stopped BEFORE the entry
        raw = op[ids][None, :] * torch.exp(-sigma)
        big = torch.full_like(sigma, inf)
        d = dict(skip=torch.where(ev & (sigma >= 0), (raw - O.ALPHA_SKIP).abs() / O.ALPHA_SKIP, big),
                 clamp=torch.where(ev & (sigma >= 0), (raw - O.ALPHA_MAX).abs() / O.ALPHA_MAX, big),
                 stop=torch.where(ev & valid, (T_incl - O.T_STOP).abs() / O.T_STOP, big),
                 sigma=torch.where(ev, sigma.abs(), big))  # fmt: skip
        for k, v in d.items():
            out[k][y0:y1, x0:x1] = v.min(dim=1).values.reshape(y1 - y0, x1 - x0)
        evaluated[t], contributing[t] = ev, include
    out["kept"] = ((out["skip"] >= ALPHA_MARGIN) & (out["clamp"] >= ALPHA_MARGIN) & (out["sigma"] >= SIGMA_MARGIN)
                   & (out["stop"] >= T_MARGIN))  # fmt: skip
    out["evaluated"], out["contributing"] = evaluated, contributing
    return out


# ---------------------------------------------------------------------------------------------------------------------
# forward


def composite(scene: RegimeScene, channels: int, dtype, mutant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """-> render [H,W,C], alpha [H,W] (formed as 1 - T), last_ids [H,W] int32 (the tile's start - 1 where nothing
    contributes), weight [H,W] = sum_i w_i |c_i|_inf (what the render yardstick divides by), stopped [H,W] bool (the pixel
    met the stop rule), include: tile -> [P,L] bool."""
    W, H = scene.width, scene.height
    m2, con, op, col = scene.means2d.to(dtype), scene.conics.to(dtype), scene.opacities.to(dtype), scene.features(channels).to(dtype)
    render = torch.zeros(H, W, channels, dtype=dtype)
    alpha = torch.zeros(H, W, dtype=dtype)
    weight = torch.zeros(H, W, dtype=dtype)
    last_ids = torch.zeros(H, W, dtype=torch.int32)
    stopped_px = torch.zeros(H, W, dtype=torch.bool)
    includes = {}
    for t, s, e, y0, y1, x0, x1 in _tiles(scene):
        if e <= s:
            last_ids[y0:y1, x0:x1] = s - 1
            continue
        ids = scene.flatten_ids[s:e].long()
        px, py = _pixel_centres(y0, y1, x0, x1, dtype)
        _, _, _, a, T_excl, include, stopped = _walk(px, py, m2[ids], con[ids], op[ids], mutant)
        wgt = torch.where(include, a * T_excl, torch.zeros_like(a))
        T_final = torch.where(include, 1.0 - a, torch.ones_like(a)).prod(dim=1)
        idx = torch.arange(e - s)[None, :].expand_as(include)
        last = torch.where(include, idx, torch.full_like(idx, -1)).max(dim=1).values + s
        shape = (y1 - y0, x1 - x0)
        render[y0:y1, x0:x1] = (wgt @ col[ids]).reshape(*shape, channels)
        alpha[y0:y1, x0:x1] = (1.0 - T_final).reshape(shape)
        weight[y0:y1, x0:x1] = (wgt @ col[ids].abs().max(dim=1).values).reshape(shape)
        last_ids[y0:y1, x0:x1] = last.reshape(shape).to(torch.int32)
        stopped_px[y0:y1, x0:x1] = stopped.any(dim=1).reshape(shape)
        includes[t] = include
    return dict(render=render, alpha=alpha, last_ids=last_ids, weight=weight, stopped=stopped_px, include=includes)


# ---------------------------------------------------------------------------------------------------------------------
# backward


def backward(scene: RegimeScene, channels: int, v_render, v_alpha, alpha_out, dtype, mutant: Optional[str] = None):
    """-> (grads, accum): name -> [N,k] for means2d (2), absgrad (2), conics (3), features (C), opacities (1).
    ``v_render`` [H,W,C], ``v_alpha`` [H,W], ``alpha_out`` [H,W]: the forward's alpha image, from which every T is rebuilt
    walking back (T = 1 - alpha_out; T *= 1 / (1 - alpha_i) from the last entry to the first).  ``accum``: the same sums over
    pixels with every per-pixel term replaced by its magnitude."""
    N = scene.means2d.shape[0]
    m2, con_all, op_all, col_all = (scene.means2d.to(dtype), scene.conics.to(dtype), scene.opacities.to(dtype),
                                    scene.features(channels).to(dtype))  # fmt: skip
    v_render, v_alpha, alpha_out = v_render.to(dtype), v_alpha.to(dtype), alpha_out.to(dtype)
    sizes = dict(means2d=2, absgrad=2, conics=3, features=channels, opacities=1)
    grads = {k: torch.zeros(N, n, dtype=dtype) for k, n in sizes.items()}
    accum = {k: torch.zeros(N, n, dtype=dtype) for k, n in sizes.items()}
    for t, s, e, y0, y1, x0, x1 in _tiles(scene):
        if e <= s:
            continue
        ids = scene.flatten_ids[s:e].long()
        px, py = _pixel_centres(y0, y1, x0, x1, dtype)
        xy, con, op, col = m2[ids], con_all[ids], op_all[ids], col_all[ids]
        dx, dy, sigma, a, _, include, _ = _walk(px, py, xy, con, op, mutant)
        zero = torch.zeros_like(a)
        T_final = 1.0 - alpha_out[y0:y1, x0:x1].reshape(-1)
        r_inc = torch.where(include, 1.0 / (1.0 - a), torch.ones_like(a))
        seq = torch.cat([T_final[:, None], torch.flip(r_inc, [1])], 1)
        T_excl = torch.flip(torch.cumprod(seq, 1)[:, 1:], [1])  # T in front of entry i
        fac = torch.where(include, a * T_excl, zero)  # [P,L]
        vr = v_render[y0:y1, x0:x1].reshape(-1, channels)
        va = v_alpha[y0:y1, x0:x1].reshape(-1)
        cdot = (col @ vr.t()).t()  # [P,L] = <c_j, v_render>
        contrib = fac * cdot
        suffix = torch.flip(torch.cumsum(torch.flip(contrib, [1]), 1), [1])
        if mutant != "suffix_includes_self":
            suffix = suffix - contrib
        ra = 1.0 / (1.0 - a)
        g_alpha = torch.where(include, (T_excl * cdot - suffix * ra) + (T_final * va)[:, None] * ra, zero)
        vis = torch.where(include, torch.exp(-sigma), zero)  # (exp(-sigma) of a skipped sigma < 0 may overflow)
        open_ = include if mutant == "clamp_passes_gradient" else include & ((op[None, :] * vis) <= O.ALPHA_MAX)
        g_op = torch.where(open_, vis * g_alpha, zero)
        g_sigma = torch.where(open_, -(op[None, :] * vis) * g_alpha, zero)
        terms = dict(
            conics=[0.5 * g_sigma * dx * dx, g_sigma * dx * dy * (0.5 if mutant == "conic_b_halved" else 1.0), 0.5 * g_sigma * dy * dy],
            means2d=[g_sigma * (con[None, :, 0] * dx + con[None, :, 1] * dy), g_sigma * (con[None, :, 1] * dx + con[None, :, 2] * dy)],
            opacities=[g_op])  # fmt: skip
        for k, cols in terms.items():
            grads[k].index_add_(0, ids, torch.stack([c.sum(0) for c in cols], -1))
            accum[k].index_add_(0, ids, torch.stack([c.abs().sum(0) for c in cols], -1))
        grads["features"].index_add_(0, ids, fac.t() @ vr)
        accum["features"].index_add_(0, ids, fac.t() @ vr.abs())
        ab = torch.stack([c.sum(0).abs() if mutant == "absgrad_abs_of_sum" else c.abs().sum(0) for c in terms["means2d"]], -1)
        grads["absgrad"].index_add_(0, ids, ab)
    accum["absgrad"] = accum["means2d"].clone()
    return grads, accum


def cotangents(channels: int, group: str, kept: torch.Tensor, seed: int = 0):
    """-> (v_render [H,W,C], v_alpha [H,W]) float64 of a group: the same random numbers whatever the group, zero on the
    pixels that are not kept and on the output the group does not drive."""
    assert group in GROUPS
    g = torch.Generator().manual_seed(2000 + seed)
    H, W = kept.shape
    vr = torch.randn(H, W, 8, generator=g, dtype=torch.float64)[..., :channels] * kept[..., None]
    va = torch.randn(H, W, generator=g, dtype=torch.float64) * kept
    if group == "render":
        va = torch.zeros_like(va)
    if group == "alpha":
        vr = torch.zeros_like(vr)
    return vr.contiguous(), va


def gradients(scene: RegimeScene, channels: int, dtype, kept: torch.Tensor, mutant: Optional[str] = None, groups=GROUPS):
    """-> (forward, {group: (grads, accum)}): one forward of the restatement in ``dtype``, one backward per group (from
    that forward's own alpha image, as in production)."""
    fwd = composite(scene, channels, dtype, mutant)
    res = {}
    for group in groups:
        vr, va = cotangents(channels, group, kept)
        res[group] = backward(scene, channels, vr, va, fwd["alpha"], dtype, mutant)
    return fwd, res


# ---------------------------------------------------------------------------------------------------------------------
# the forward's distances


def forward_distance(fwd, fwd64) -> Dict[str, torch.Tensor]:
    """-> render [H,W]: |r - r64|_inf / sum_i w_i |c_i|_inf (where nothing contributes r64 is exactly 0: 0 if r is too, else
    inf); alpha [H,W]: |a - a64| (absolute: alpha is formed as 1 - T)."""
    r, a = fwd["render"].detach().cpu().double(), fwd["alpha"].detach().cpu().double().reshape(fwd64["alpha"].shape)
    err = (r - fwd64["render"]).abs().max(dim=-1).values  # (the largest channel's error is what the weight sum bounds)
    return dict(render=P.distance(err, torch.zeros_like(err), fwd64["weight"]),
                alpha=P.distance(a, fwd64["alpha"], torch.ones_like(a)))  # fmt: skip


def pixel_masks(fwd64, kept) -> Dict[str, Dict[str, torch.Tensor]]:
    """{output: {pixel class: [H,W] bool}}: the kept pixels of each class -- for the render those something contributes to
    (the others must be exactly zero, which the GPU test asserts, and take no part in the class's maximum)."""
    cls = P.masks_of_index(pixel_class(), PIXEL_CLASSES)
    return dict(render=P.restrict(cls, kept & (fwd64["weight"] > 0)), alpha=P.restrict(cls, kept))


# ---------------------------------------------------------------------------------------------------------------------
# the composite epilogue (``Composite`` in csrc/raster.hip: fg_raster_composite_fwd / _bwd)


def composite_scene(scene: Optional[RegimeScene] = None) -> RegimeScene:
    """The sibling of ``scene`` (the regime scene of SEED) the epilogue cases run on: the same rows and the same lists, the
    colours c (U(0,1): over a background in [0,1] they never leave [0,1]) mapped to 2 c in channel 0, 1.75 c in channels 1 and 2
    and 2 c - 1 (signed, as flow and depth residuals are) in channels 3-7, so that a bound is crossed on a good share of the
    pixels but never on most.  (2 c in channels 1 and 2 as well: 73 % of the pixels above 1 over a white background, beyond what
    tests/test_raster_rows_host.py allows; this seed's channel 0 is the darkest.)"""
    scene = regime_scene(SEED) if scene is None else scene
    c = scene.colours.double()
    return replace(scene, colours=torch.cat([2.0 * c[:, :1], 1.75 * c[:, 1:3], 2.0 * c[:, 3:] - 1.0], 1).float().contiguous())


def background_in(background, dtype) -> Optional[torch.Tensor]:
    """The background as the kernels get it -- fp32 values -- in ``dtype``; None stays None."""
    return None if background is None else torch.as_tensor(background, dtype=torch.float32).to(dtype)


def epilogue(fwd, background, n_clamp: int, dtype, mutant: Optional[str] = None, exact_channels=()):
    """``fwd``: what ``composite`` returned.  -> out [H,W,C] = render + (1 - alpha) * background, its first ``n_clamp`` channels
    clamped to [0,1]; blocked [H,W,C] bool: the clamped channel's value lies STRICTLY outside [0,1] (torch.clamp's gradient
    rule: it passes at the bounds themselves); bound_distance [H,W]: the smallest min(|v|, |v - 1|) over the clamped channels
    before clamping, inf without any -- ``exact_channels``: channels left out of it, whose value sits ON a bound by
    construction (colours and background identically zero: 0 in every arithmetic); weight [H,W]: what an unblocked channel's
    error is measured by, sum_i w_i |c_i|_inf + (1 - alpha) |background|_inf."""
    render, alpha = fwd["render"].to(dtype), fwd["alpha"].to(dtype)
    C = render.shape[-1]
    om = 1.0 - alpha
    out = render.clone()
    weight = fwd["weight"].to(dtype).clone()
    if background is not None:
        bg = background_in(background, dtype)
        out = out + om[..., None] * bg
        weight = weight + om * bg.abs().max()
    if mutant == "clamp_reaches_channel_n_clamp":
        n_clamp = min(n_clamp + 1, C)
    blocked = torch.zeros_like(out, dtype=torch.bool)
    bound_distance = torch.full(alpha.shape, float("inf"), dtype=dtype)
    if n_clamp > 0:
        v = out[..., :n_clamp]
        blocked[..., :n_clamp] = (v < 0) | (v > 1)
        near = torch.minimum(v.abs(), (v - 1.0).abs())
        for c in exact_channels:
            near[..., c] = float("inf")
        bound_distance = near.min(dim=-1).values
        out[..., :n_clamp] = v.clamp(0.0, 1.0)
    return dict(out=out, blocked=blocked, bound_distance=bound_distance, weight=weight)


def epilogue_backward(v_out, v_alpha, blocked, background, mutant: Optional[str] = None):
    """-> (v_render_eff, v_alpha_eff), which feed ``backward`` unchanged: the blocked channels' cotangents zeroed, and
    v_alpha - sum_c v_render_eff[c] * background[c] (d/d alpha of (1 - alpha) * background)."""
    if mutant == "mask_bit_of_next_channel":  # channel c reads bit c + 1 (the last one a bit nobody set)
        blocked = torch.cat([blocked[..., 1:], torch.zeros_like(blocked[..., :1])], -1)
    if mutant == "blocked_channel_passes_gradient":
        blocked = torch.zeros_like(blocked)
    v_render = torch.where(blocked, torch.zeros_like(v_out), v_out)
    if background is None or mutant == "background_missing_from_alpha_gradient":
        return v_render, v_alpha.clone()
    return v_render, v_alpha - (v_render * background_in(background, v_out.dtype)).sum(-1)


@dataclass(frozen=True)
class EpilogueCase:
    name: str
    channels: int
    background: Optional[tuple]
    n_clamp: int


EPILOGUE_CASES = (
    EpilogueCase("model-rgb", 3, (1.0, 0.25, 0.0), 3),  # the model's path; background components exactly at both bounds
    EpilogueCase("model-rgbd", 4, (1.0, 1.0, 1.0, 0.0), 3),  # RGB+ED: the depth channel unclamped and signed
    EpilogueCase("bg-only", 3, (0.2, 0.3, 0.4), 0),  # no mask: only the alpha-cotangent term
    EpilogueCase("clamp-only", 3, None, 3),  # mask without a background
    EpilogueCase("flow-6", 6, (0.5, 0.5, 0.5, 0.0, 0.0, 0.0), 3),  # three unclamped signed channels behind the mask
    EpilogueCase("all-8", 8, (0.25,) * 8, 8),  # all eight mask bits; channels 3-7 are blocked below 0
    EpilogueCase("one", 1, (0.25,), 1),  # a single channel
)
CASE = {c.name: c for c in EPILOGUE_CASES}
# THE BOUND ITSELF: channel 0 of every row is 0 and so is its background -- the value is 0 in every arithmetic, ON the bound,
# where the clamp passes the gradient (``bound_scene``; channel 0 is an ``exact_channels`` entry: it excludes no pixel)
BOUND_CASE = EpilogueCase("bound", 3, (0.0, 0.25, 1.0), 3)


def bound_scene(scene: RegimeScene) -> RegimeScene:
    colours = scene.colours.clone()
    colours[:, 0] = 0.0
    return replace(scene, colours=colours)


def epilogue_gradients(scene: RegimeScene, case: EpilogueCase, dtype, kept: torch.Tensor, mutant: Optional[str] = None,
                       groups=GROUPS, exact_channels=()):  # fmt: skip
    """One forward of the restatement with the case's epilogue in ``dtype`` and one backward per group.
    -> (forward, epilogue, compared, {group: (grads, accum)}).  ``compared`` [H,W] bool: ``kept`` and farther than CLAMP_MARGIN
    from either bound in FLOAT64 (the same pixels whatever ``dtype`` or ``mutant``); the cotangents are zero elsewhere.
    ``accum`` is ``backward``'s with every cotangent by magnitude: |v_render_eff| and |v_alpha| + sum_c |v_render_eff[c] *
    background[c]| -- the alpha cotangent the walk sees is itself a sum that cancels."""
    fwd = composite(scene, case.channels, dtype)
    ep = epilogue(fwd, case.background, case.n_clamp, dtype, mutant, exact_channels)
    if dtype == torch.float64 and mutant is None:
        near = ep["bound_distance"]
    else:
        near = epilogue(composite(scene, case.channels, torch.float64), case.background, case.n_clamp, torch.float64,
                        exact_channels=exact_channels)["bound_distance"]  # fmt: skip
    compared = kept & (near > CLAMP_MARGIN)
    bg = background_in(case.background, dtype)
    res = {}
    for group in groups:
        vo, va = cotangents(case.channels, group, compared)
        vo, va = vo.to(dtype), va.to(dtype)
        vr_eff, va_eff = epilogue_backward(vo, va, ep["blocked"], bg, mutant)
        grads, _ = backward(scene, case.channels, vr_eff, va_eff, fwd["alpha"], dtype)
        va_abs = va.abs() if bg is None else va.abs() + (vr_eff * bg).abs().sum(-1)
        _, accum = backward(scene, case.channels, vr_eff.abs(), va_abs, fwd["alpha"], dtype)
        res[group] = (grads, accum)
    return fwd, ep, compared, res


def epilogue_forward_distance(out, ep64) -> torch.Tensor:
    """[H,W]: the largest |out - out64| / weight over a pixel's UNBLOCKED channels (a blocked channel is exactly 0 or 1: the
    GPU test asserts that; it takes no part here).  0 where every channel is blocked."""
    d = P.distance(out.detach().cpu().double(), ep64["out"], ep64["weight"][..., None].expand_as(ep64["out"]))
    return torch.where(ep64["blocked"], torch.zeros_like(d), d).max(dim=-1).values
