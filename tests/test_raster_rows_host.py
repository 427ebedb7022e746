"""The compositing stage's restatement (tests/raster_restatement.py) and its regime scene, checked on the CPU: the fp32
restatement is the pinned oracle's ``rasterize`` / ``rasterize_backward(alpha_out=)``, every regime is what it is named for,
the pixels left out for sitting on a decision threshold are few and cost no row more than a fifth of its footprint, fp32 and
float64 take the same decisions on every pixel that is kept, and the row-wise bound the GPU test applies (F x the fp32
restatement's own row distance from float64, per regime, cotangent group and tensor; tests/parity_common.py has the
protocol) catches each wrong restatement.  The composite epilogue (``R.epilogue`` / ``R.epilogue_backward``, the named cases of
``R.EPILOGUE_CASES`` on ``R.composite_scene``): the pair is autograd's clamp(render + (1 - alpha) * bg, 0, 1) exactly, fp32 and
float64 agree on the mask, few pixels are left out, every clamped channel is blocked on a good share of the pixels and open on
most, and its four mutants are caught in the same way."""
import functools

import pytest
import torch

import parity_common as P
import raster_restatement as R
from oracle import raster_oracle as O

C = 3


@functools.lru_cache(maxsize=None)
def _scene():
    return R.regime_scene(R.SEED)


@functools.lru_cache(maxsize=None)
def _margins():
    return R.margins(_scene())


@functools.lru_cache(maxsize=None)
def _grads(dtype, mutant=None, channels=C):
    return R.gradients(_scene(), channels, dtype, _margins()["kept"], mutant=mutant)


@functools.lru_cache(maxsize=None)
def _composite_scene():
    return R.composite_scene(_scene())


@functools.lru_cache(maxsize=None)
def _epilogue(case, dtype, mutant=None):
    """(forward, epilogue, compared, {group: (grads, accum)}) of a named epilogue case on the composite scene."""
    return R.epilogue_gradients(_composite_scene(), R.CASE[case], dtype, _margins()["kept"], mutant=mutant)


def _tile_pixels(tile):
    ty, tx = divmod(tile, R.TILE_W)
    return slice(ty * R.TILE, (ty + 1) * R.TILE), slice(tx * R.TILE, (tx + 1) * R.TILE)


def _footprints():
    """[N] pixels each row contributes to (float64), and how many of them are kept."""
    sc, m = _scene(), _margins()
    total, kept = torch.zeros(len(sc.labels)), torch.zeros(len(sc.labels))
    for t, s, e, y0, y1, x0, x1 in R._tiles(sc):
        if e > s:
            ids = sc.flatten_ids[s:e].long()
            inc = m["contributing"][t].float()
            total.index_add_(0, ids, inc.sum(0))
            kept.index_add_(0, ids, (inc * m["kept"][y0:y1, x0:x1].reshape(-1, 1).float()).sum(0))
    return total, kept


@pytest.mark.parametrize("channels", [1, 3, 8])
def test_fp32_restatement_is_the_pinned_oracle(channels):
    """Measured: bit for bit -- forward, last_ids and all five gradients (the formulae and their order are the oracle's)."""
    sc = _scene()
    kept = _margins()["kept"]
    feats = sc.features(channels)
    r, a, last = O.rasterize(sc.means2d, sc.conics, feats, sc.opacities, sc.width, sc.height, R.TILE, sc.offsets, sc.flatten_ids)
    fwd = R.composite(sc, channels, torch.float32)
    assert torch.equal(fwd["render"], r) and torch.equal(fwd["alpha"], a[..., 0]) and torch.equal(fwd["last_ids"], last)
    vr, va = R.cotangents(channels, "both", kept)
    ref = O.rasterize_backward(sc.means2d, sc.conics, feats, sc.opacities, sc.width, sc.height, R.TILE, sc.offsets,
                               sc.flatten_ids, vr.float(), va.float(), alpha_out=a)  # fmt: skip
    grads, _ = R.backward(sc, channels, vr, va, fwd["alpha"], torch.float32)
    for name, x in zip(("means2d", "absgrad", "conics", "features", "opacities"), ref):
        assert bool(torch.isfinite(x).all()), name
        assert torch.equal(grads[name].reshape(x.shape), x), name


def test_census_every_regime_is_what_it_is_named_for():
    sc, m = _scene(), _margins()
    for name, n in R.COUNTS.items():
        assert len(sc.rows(name)) == n
    assert (sc.width, sc.height) == (72, 40) and sc.offsets.numel() == R.TILE_W * R.TILE_H + 1
    lens = (sc.offsets[1:] - sc.offsets[:-1]).long()
    total, _ = _footprints()
    f64, g64 = _grads(torch.float64)
    # faint and occluded: exactly zero in every group and tensor; no pixel takes them
    for name in ("faint", "occluded"):
        rows = sc.rows(name)
        assert bool((total[rows] == 0).all())
        for group in R.GROUPS:
            for tensor in R.TENSORS:
                assert bool(P.zero_rows(g64[group][0][tensor])[rows].all()), (name, group, tensor)
    assert bool((sc.opacities[sc.rows("faint")] < O.ALPHA_SKIP).all())
    # every other regime has rows that contribute; barely: a few pixels each
    for name in R.COUNTS:
        if name not in ("faint", "occluded"):
            assert bool((total[sc.rows(name)] > 0).any()), name
    barely = total[sc.rows("barely")]
    assert 0 < float(barely[barely > 0].median()) <= 40
    # opaque: the 0.999 clamp holds on pixels that take the row; plain rows are never clamped
    clamped = torch.zeros(len(sc.labels))
    reach = {}
    for t, s, e, y0, y1, x0, x1 in R._tiles(sc):
        if e > s:
            ids = sc.flatten_ids[s:e].long()
            px, py = R._pixel_centres(y0, y1, x0, x1, torch.float64)
            _, _, sigma, _, _, include, stopped = R._walk(px, py, sc.means2d.double()[ids], sc.conics.double()[ids], sc.opacities.double()[ids])
            over = include & (sc.opacities.double()[ids][None, :] * torch.exp(-sigma.clamp_min(0)) > O.ALPHA_MAX)
            clamped.index_add_(0, ids, over.float().sum(0))
            reach[t] = (sigma, include, stopped, ids)
    assert bool((sc.opacities[sc.rows("opaque")] == 1.0).all()) and int((clamped[sc.rows("opaque")] > 0).sum()) >= 8
    assert bool((clamped[sc.rows("plain", "deep", "needle", "edge", "subpixel")] == 0).all())
    # deep: one list beyond 256 entries (the staging batch of every pixels-per-lane body is 64, 128 or 256), nothing stops
    assert int(lens[R.DEEP_TILE]) > 256 and int(lens.argmax()) == R.DEEP_TILE
    ys, xs = _tile_pixels(R.DEEP_TILE)
    assert not bool(f64["stopped"][ys, xs].any())
    sigma, include, _, ids = reach[R.DEEP_TILE]
    deep_here = torch.tensor([sc.labels[int(i)] == "deep" for i in ids])
    assert int(deep_here.sum()) == R.COUNTS["deep"] and int(include[:, deep_here].any(0).sum()) > 256
    assert int(include[:, 256:].any(0).sum()) > 32  # entries beyond the first 256 are taken
    # wall: every pixel of its tile stops, inside the wall
    ys, xs = _tile_pixels(R.WALL_TILE)
    assert bool(f64["stopped"][ys, xs].all())
    _, include, _, ids = reach[R.WALL_TILE]
    assert all(sc.labels[int(i)] == "wall" for i in ids[include.any(0)])
    assert set(sc.labels[int(i)] for i in ids) >= {"wall", "occluded"}
    # indefinite: b^2 > a c; every row has pixels it skips for sigma < 0 and pixels that take it
    ind = sc.rows("indefinite")
    con = sc.conics.double()[ind]
    assert bool((con[:, 1] ** 2 > con[:, 0] * con[:, 2]).all())
    skipped, taken = torch.zeros(len(sc.labels)), torch.zeros(len(sc.labels))
    for t, (sigma, include, stopped, ids) in reach.items():
        skipped.index_add_(0, ids, ((sigma < 0) & m["evaluated"][t]).float().sum(0))
        taken.index_add_(0, ids, include.float().sum(0))
    assert bool((skipped[ind] > 0).all()) and bool((taken[ind] > 0).all())
    assert bool((skipped[sc.rows(*[k for k in R.COUNTS if k != "indefinite"])] == 0).all())
    # partial tiles hold contributing rows; no tile is empty (the huge rows reach every one)
    cls = R.pixel_class()
    partial = cls == R.PIXEL_CLASSES.index("partial")
    assert int(partial.sum()) == 72 * 40 - 64 * 32 and bool((f64["weight"][partial] > 0).float().mean() > 0.9)
    assert bool((lens > 0).all())
    huge_lists = torch.zeros(len(sc.labels))
    huge_lists.index_add_(0, sc.flatten_ids.long(), torch.ones(sc.flatten_ids.numel()))
    assert bool((huge_lists[sc.rows("huge")] == R.TILE_W * R.TILE_H).all())
    # edge: centres outside the image, still contributing
    ex = sc.means2d[sc.rows("edge"), 0]
    assert bool(((ex < 0) | (ex > sc.width)).all()) and bool((total[sc.rows("edge")] > 0).all())
    # sub-pixel: a 3 x 3 block of pixels at the most
    assert bool((total[sc.rows("subpixel")] <= 9).all())


def test_exclusions_are_few_and_cost_no_row_much():
    """Conditions on the chosen seed, not measurements: at most 1.5 % of the pixels excluded; every contributing row keeps at
    least 80 % of the pixels it contributes to."""
    m = _margins()
    excluded = 1.0 - float(m["kept"].float().mean())
    total, kept = _footprints()
    share = (kept / total)[total > 0]
    print(f"excluded {int((~m['kept']).sum())} of {m['kept'].numel()} pixels ({100 * excluded:.2f} %): "
          + ", ".join(f"{k} {int((m[k] < (R.T_MARGIN if k == 'stop' else R.ALPHA_MARGIN)).sum())}" for k in ("skip", "clamp", "stop", "sigma"))
          + f"; smallest kept share of a row {float(share.min()):.3f}; {int((total > 0).sum())} contributing rows")  # fmt: skip
    assert 0 < excluded <= 0.015
    assert float(share.min()) >= 0.8


def test_fp32_and_float64_decide_alike_on_kept_pixels():
    sc, kept = _scene(), _margins()["kept"]
    f32, f64 = R.composite(sc, C, torch.float32), R.composite(sc, C, torch.float64)
    assert torch.equal(f32["last_ids"][kept], f64["last_ids"][kept])
    assert torch.equal(f32["stopped"][kept], f64["stopped"][kept])
    for t, s, e, y0, y1, x0, x1 in R._tiles(sc):
        if e > s:
            k = kept[y0:y1, x0:x1].reshape(-1)
            assert torch.equal(f32["include"][t][k], f64["include"][t][k]), t


def test_yardsticks_are_floored_and_finite():
    for channels in (1, 3, 4, 8):
        f32, g32 = _grads(torch.float32, None, channels)
        f64, g64 = _grads(torch.float64, None, channels)
        d, masks = R.forward_distance(f32, f64), R.pixel_masks(f64, _margins()["kept"])
        for what in d:
            assert set(masks[what]) == set(R.PIXEL_CLASSES)
            for cls, e in P.yardstick(masks[what], d[what], R.FLOOR).items():
                assert R.FLOOR <= e < 1e-4, (channels, what, cls, e)
        for group in R.GROUPS:
            grads, accum = g64[group]
            for tensor in R.TENSORS:
                assert bool(torch.isfinite(grads[tensor]).all()) and bool((accum[tensor] >= 0).all())
                # a row is exactly zero where its accumulation is
                assert bool(P.zero_rows(grads[tensor])[P.zero_rows(accum[tensor])].all())
                assert bool((g32[group][0][tensor][P.zero_rows(grads[tensor])] == 0).all()), (group, tensor)
                d32 = P.distance(g32[group][0][tensor], grads[tensor], accum[tensor], rows=True)
                for regime, e in P.yardstick(P.live_row_masks(_scene().labels, grads[tensor]), d32, R.FLOOR).items():
                    assert R.FLOOR <= e < 1e-3, (channels, group, tensor, regime, e)


LIVE = tuple(k for k in R.COUNTS if k not in ("faint", "occluded"))
GEOMETRY = ("means2d", "absgrad", "conics", "opacities")
# (mutant, cotangent groups that drive it, tensors it reaches, regimes it concerns)
NOT_WALL = tuple(k for k in LIVE if k != "wall")
MANY_PIXELS = tuple(k for k in LIVE if k not in ("barely", "subpixel"))
# (mutant, cotangent groups that drive it, tensors it reaches, regimes it concerns, epilogue case or None: the plain raster)
MUTANT_CASES = [
    # the clamped pixel of an opaque row is the one its mean sits in: dx, dy ~ 0.03 sigma there and the position and
    # shape gradients through it vanish; the opacity gradient does not
    ("clamp_passes_gradient", R.GROUPS, ("opacities",), ("opaque",), None),
    # the rows the stop rule drops at every pixel: the wall's rear rows and everything behind it
    ("stop_entry_composited", R.GROUPS, R.TENSORS, ("wall", "occluded"), None),
    # (the alpha group has no suffix sums: v_render = 0)
    ("suffix_includes_self", ("render", "both"), GEOMETRY, LIVE, None),
    ("conic_b_halved", R.GROUPS, ("conics",), LIVE, None),
    ("absgrad_abs_of_sum", R.GROUPS, ("absgrad",), LIVE, None),
    # the composite epilogue (the alpha group has v_out = 0: neither the mask nor the background term acts).  A blocked
    # channel's cotangent reaches every tensor: the colours directly, the others through <c_j, v> and the alpha term.  (Over
    # white and in the signed channels every regime's rows hold blocked pixels; over model-rgb's background the deep tile,
    # which averages 300 faint rows, has none.)
    ("blocked_channel_passes_gradient", ("render", "both"), R.TENSORS, LIVE, "model-rgbd"),
    ("blocked_channel_passes_gradient", ("render", "both"), R.TENSORS, LIVE, "all-8"),
    # the alpha cotangent reaches a row as T_final * v_alpha: nothing of it is left behind the wall (T_final <= 1e-4), and
    # the colour gradient does not see it
    ("background_missing_from_alpha_gradient", ("render", "both"), GEOMETRY, NOT_WALL, "bg-only"),
    ("background_missing_from_alpha_gradient", ("render", "both"), GEOMETRY, NOT_WALL, "model-rgb"),
    ("mask_bit_of_next_channel", ("render", "both"), R.TENSORS, LIVE, "model-rgbd"),
    ("mask_bit_of_next_channel", ("render", "both"), R.TENSORS, LIVE, "all-8"),
    # the unclamped signed channel leaves [0,1] on a third of the pixels: of the rows of a few pixels (barely, sub-pixel)
    # fewer than three quarters hold one
    ("clamp_reaches_channel_n_clamp", ("render", "both"), R.TENSORS, MANY_PIXELS, "model-rgbd"),
]


def _reference_and_mutant(mutant, case):
    """-> (g32, g64, gm): {group: (grads, accum)} of the fp32, the float64 and the mutant's float64 restatement."""
    if case is None:
        return _grads(torch.float32)[1], _grads(torch.float64)[1], _grads(torch.float64, mutant)[1]
    return _epilogue(case, torch.float32)[3], _epilogue(case, torch.float64)[3], _epilogue(case, torch.float64, mutant)[3]


def mutant_shares(factor):
    """-> {(mutant, group, tensor, regime, case): (caught, rows, smallest caught-making F)}: a row of the mutant's float64
    gradient is CAUGHT when the GPU test would flag it -- not zero where the true row is exactly zero, or at least 4 * factor *
    E32 from the true row.  Rows that are zero in both do not count (the mutant does not reach them)."""
    sc = _scene()
    out = {}
    for mutant, groups, tensors, regimes, case in MUTANT_CASES:
        g32, g64, gm = _reference_and_mutant(mutant, case)
        for group in groups:
            for tensor in tensors:
                ref, acc = g64[group][0][tensor], g64[group][1][tensor]
                e32 = P.yardstick(P.live_row_masks(sc.labels, ref), P.distance(g32[group][0][tensor], ref, acc, rows=True), R.FLOOR)
                d = P.distance(gm[group][0][tensor], ref, acc, rows=True)
                zero, zero_m = P.zero_rows(ref), P.zero_rows(gm[group][0][tensor])
                for regime in regimes:
                    rows = sc.rows(regime)
                    rows = rows[~(zero[rows] & zero_m[rows])]
                    if len(rows) == 0 and group == "alpha" and tensor == "features":
                        continue  # (no colour gradient without v_render)
                    caught = torch.where(zero[rows], ~zero_m[rows], d[rows] >= 4 * factor * e32[regime])
                    ratios = torch.where(zero[rows], torch.full_like(d[rows], float("inf")), d[rows] / e32[regime])
                    out[(mutant, group, tensor, regime, case)] = (int(caught.sum()), len(rows), P.three_quarter_cap(ratios))
    return out


def test_every_mutant_is_listed():
    assert {c[0] for c in MUTANT_CASES} == set(R.MUTANTS)


def test_mutants_are_caught_by_the_row_bound():
    """On at least three quarters of the rows of each regime a mutant concerns, in each cotangent group that drives it, the
    mutant's float64 gradient is at least 4 * F * E32 from the true one, or not zero where the true one is exactly zero
    (cancellation may hide it on single rows): the GPU bound F * E32 has teeth, and this caps F.  Only
    ``stop_entry_composited`` changes the forward."""
    f64, _ = _grads(torch.float64)
    for mutant in R.MUTANTS:
        fm, _ = _grads(torch.float64, mutant)
        assert torch.equal(fm["render"], f64["render"]) == (mutant != "stop_entry_composited"), mutant
    # (of the epilogue's mutants only ``clamp_reaches_channel_n_clamp`` changes the finished image)
    for mutant, _, _, _, case in MUTANT_CASES:
        if case is not None:
            same = torch.equal(_epilogue(case, torch.float64, mutant)[1]["out"], _epilogue(case, torch.float64)[1]["out"])
            assert same == (mutant != "clamp_reaches_channel_n_clamp"), (mutant, case)
    factor = 1.0 if R.F is None else R.F
    shares = mutant_shares(factor)
    cap = min(v[2] for v in shares.values())
    worst = {}
    for (mutant, group, tensor, regime, case), (caught, rows, c) in shares.items():
        key = (mutant, regime) if case is None else (mutant, regime, case)
        if key not in worst or c < worst[key][4]:
            worst[key] = (caught, rows, group, tensor, c)
    for (mutant, regime, *case), (caught, rows, group, tensor, c) in worst.items():
        print(f"{mutant} {regime}{' ' + case[0] if case else ''}: {caught}/{rows} rows caught at F = {factor:g} in its weakest cell ({group}, {tensor}), which caps F at {c:.1f}")
    print(f"the cap on F: {cap:.1f}")
    failures = [f"{k}: {v[0]}/{v[1]}" for k, v in shares.items() if v[1] == 0 or 4 * v[0] < 3 * v[1]]
    assert not failures, "\n".join(failures)
    assert R.F is None or R.F <= cap
    # where the true gradient is exactly zero the mutant's is not: the wall's rear rows and everything behind it
    sc = _scene()
    _, g64 = _grads(torch.float64)
    _, gm = _grads(torch.float64, "stop_entry_composited")
    for group in R.GROUPS:
        for tensor in R.TENSORS:
            if group == "alpha" and tensor == "features":
                continue  # (no colour gradient without v_render)
            zero = P.zero_rows(g64[group][0][tensor])
            for regime in ("wall", "occluded"):
                rows = sc.rows(regime)
                rows = rows[zero[rows]]
                assert len(rows) >= 4 and not bool(P.zero_rows(gm[group][0][tensor])[rows].any()), (group, tensor, regime)


# ---------------------------------------------------------------------------------------------------------------------
# the composite epilogue


@pytest.mark.parametrize("case", R.EPILOGUE_CASES, ids=[c.name for c in R.EPILOGUE_CASES])
def test_epilogue_pair_is_autograd_of_clamp(case):
    """``epilogue`` / ``epilogue_backward`` against torch.autograd.grad of clamp(render + (1 - alpha) * bg, 0, 1) with the
    unclamped channels concatenated behind the clamped ones, render and alpha float64 leaves: exactly."""
    fwd = R.composite(_composite_scene(), case.channels, torch.float64)
    render, alpha = fwd["render"].clone().requires_grad_(True), fwd["alpha"].clone().requires_grad_(True)
    bg = torch.zeros(case.channels, dtype=torch.float64) if case.background is None else R.background_in(case.background, torch.float64)
    pre = render + (1.0 - alpha)[..., None] * bg
    n = case.n_clamp
    out = torch.cat([torch.clamp(pre[..., :n], 0.0, 1.0), pre[..., n:]], -1)
    ep = R.epilogue(fwd, case.background, n, torch.float64)
    assert torch.equal(ep["out"], out.detach())
    assert not bool(ep["blocked"][..., n:].any()) and bool(ep["blocked"].any()) == (n > 0)
    assert bool(torch.isinf(ep["bound_distance"]).all()) == (n == 0)
    everything = torch.ones(R.HEIGHT, R.WIDTH, dtype=torch.bool)
    for group in R.GROUPS:
        vo, va = R.cotangents(case.channels, group, everything)
        g_render, g_alpha = torch.autograd.grad((out * vo).sum() + (alpha * va).sum(), (render, alpha), retain_graph=True)
        vr_eff, va_eff = R.epilogue_backward(vo, va, ep["blocked"], None if case.background is None else bg)
        assert torch.equal(vr_eff, g_render), (case.name, group)
        assert torch.equal(va_eff, g_alpha), (case.name, group)


def test_epilogue_fp32_and_float64_agree_on_the_mask():
    for case in R.EPILOGUE_CASES:
        _, e32, c32, _ = _epilogue(case.name, torch.float32)
        _, e64, compared, _ = _epilogue(case.name, torch.float64)
        assert torch.equal(c32, compared)
        assert torch.equal(e32["blocked"][compared], e64["blocked"][compared]), case.name


def test_epilogue_exclusions_are_few():
    """Conditions on the inputs: in every case at most 2 % of the image's 2880 pixels are left out in total (the walk's margins
    and CLAMP_MARGIN together)."""
    kept = _margins()["kept"]
    for case in R.EPILOGUE_CASES:
        _, _, compared, _ = _epilogue(case.name, torch.float64)
        assert compared.numel() == 2880 and not bool((compared & ~kept).any())
        out = int((~compared).sum())
        print(f"{case.name}: {out} of 2880 pixels left out ({100 * out / 2880:.2f} %), {int((kept & ~compared).sum())} of them "
              f"for lying within {R.CLAMP_MARGIN:g} of a bound")  # fmt: skip
        assert out <= 0.02 * 2880, case.name
        if case.n_clamp == 0:
            assert torch.equal(compared, kept)


def test_epilogue_cases_clamp_on_both_sides_of_every_channel():
    """Conditions on the inputs: in every case meant to clamp, each clamped channel is blocked on at least 5 % of the compared
    pixels and not blocked on at least 30 %; the signed channels are blocked BELOW 0, the doubled ones above 1."""
    for case in R.EPILOGUE_CASES:
        fwd, ep, compared, _ = _epilogue(case.name, torch.float64)
        for c in range(case.n_clamp):
            share = float(ep["blocked"][..., c][compared].float().mean())
            low = bool((ep["out"][..., c][compared & ep["blocked"][..., c]] == 0.0).all())
            print(f"{case.name} channel {c}: blocked on {100 * share:.1f} % of the compared pixels, {'below 0' if low else 'above 1'}")
            assert 0.05 <= share <= 0.70, (case.name, c, share)
            assert low == (c >= 3), (case.name, c)
    # bit 7 of the mask byte is set alone and together with others
    _, ep, compared, _ = _epilogue("all-8", torch.float64)
    b = ep["blocked"][compared]
    assert bool((b[:, 7] & ~b[:, :7].any(dim=1)).any()) and bool((b[:, 7] & b[:, :7].any(dim=1)).any()) and bool((~b[:, 7]).any())


def test_epilogue_yardsticks_are_floored_and_finite():
    sc = _composite_scene()
    for case in R.EPILOGUE_CASES:
        f32, e32, _, g32 = _epilogue(case.name, torch.float32)
        f64, e64, compared, g64 = _epilogue(case.name, torch.float64)
        d = R.epilogue_forward_distance(e32["out"], e64)
        for cls, e in P.yardstick(P.restrict(P.masks_of_index(R.pixel_class(), R.PIXEL_CLASSES), compared), d, R.FLOOR).items():
            assert R.FLOOR <= e < 1e-4, (case.name, cls, e)
        blocked = compared[..., None] & e64["blocked"]
        assert torch.equal(e32["out"][blocked].double(), e64["out"][blocked])  # exactly 0 or 1, on the same side
        for group in R.GROUPS:
            grads, accum = g64[group]
            for tensor in R.TENSORS:
                assert bool(torch.isfinite(grads[tensor]).all()) and bool((accum[tensor] >= 0).all())
                assert bool(P.zero_rows(grads[tensor])[P.zero_rows(accum[tensor])].all())
                assert bool((g32[group][0][tensor][P.zero_rows(grads[tensor])] == 0).all()), (case.name, group, tensor)
                d32 = P.distance(g32[group][0][tensor], grads[tensor], accum[tensor], rows=True)
                for regime, e in P.yardstick(P.live_row_masks(sc.labels, grads[tensor]), d32, R.FLOOR).items():
                    assert R.FLOOR <= e < 1e-3, (case.name, group, tensor, regime, e)


def test_epilogue_bound_scene_sits_on_the_bound_and_passes_the_gradient():
    """Conditions on the inputs of the GPU test's 'bound itself' sub-scene: channel 0 is exactly 0 on every pixel in both
    arithmetics, never blocked, excludes no pixel -- and its colour gradient is not zero on at least 90 % of the rows that
    contribute anywhere."""
    sc, kept = R.bound_scene(_composite_scene()), _margins()["kept"]
    total, _ = _footprints()
    res = {}
    for dtype in (torch.float32, torch.float64):
        res[dtype] = R.epilogue_gradients(sc, R.BOUND_CASE, dtype, kept, exact_channels=(0,))
        _, ep, compared, _ = res[dtype]
        assert bool((ep["out"][..., 0] == 0).all()) and not bool(ep["blocked"][..., 0].any())
        assert int((~compared).sum()) <= 0.02 * 2880
    for group in ("render", "both"):
        g0 = res[torch.float64][3][group][0]["features"][:, 0]
        live = total > 0
        share = float((g0[live] != 0).float().mean())
        print(f"{group}: the channel-0 colour gradient is not zero on {100 * share:.1f} % of the {int(live.sum())} contributing rows")
        assert share >= 0.9
        assert bool((g0[~live] == 0).all())
