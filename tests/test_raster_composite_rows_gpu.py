"""The composite epilogue folded into the raster kernels (``Composite`` in csrc/raster.hip: out[c] = render[c] + (1 - alpha) *
background[c], the first n_clamp channels clamped to [0,1], a per-pixel clamp-mask byte the backward reads) in isolation:
records packed by fg_pack_splats, ``ops.rasterize_splats(..., background=, n_clamp=)`` -- fg_raster_composite_fwd / _bwd, the
classic launches, no job lists (fg_raster_jobs_words == 0 is asserted) -- on the composite scene of tests/raster_restatement.py
(the regime scene's rows and lists, colours that leave [0,1]), for every named case of ``R.EPILOGUE_CASES``, every pixel and
every row compared with the float64 restatement, one cotangent group at a time.

A pixel is COMPARED if the walk's margins keep it and no clamped channel lies within R.CLAMP_MARGIN of a bound in float64
(tests/test_raster_rows_host.py: at least 98 % of the image in every case); the cotangents are zero elsewhere.
FORWARD, on every compared pixel:
    last_ids equal the float64 restatement's; alpha is bit-identical to the forward of the same records without an epilogue;
    a channel float64 blocks is exactly 0.0 or exactly 1.0, on float64's side;
    every other channel:  |out - out64| / (sum_i w_i |c_i|_inf + (1 - alpha64) |bg|_inf)  <=  F * E32(pixel class)
BACKWARD, per cotangent group (render / alpha / both), per tensor (the five slices of the gradient record, include/fgraster.h):
    a row whose float64 gradient is exactly zero is zero on the GPU;
    every other row:  |g_hip - g64|_2 / |A64|_2  <=  F * E32(regime, group, tensor)
    ``render`` forms its loss from the image alone: v_alphas reaches the kernel as NULL while a background is present;
    means2d.grad and means2d.absgrad are slots 0-1 and 6-7 of the record gradient, bit for bit.
tests/parity_common.py has the protocol; F and FLOOR are raster_restatement's, E32 comes from the fp32 restatement of the same
case, the recorded table is the section "composite epilogue" of profiles/raster_row_parity.md.  Each backward runs twice and
both runs are held to the bound; the forward is bit-identical across all of them.

``python tests/test_raster_composite_rows_gpu.py REPORT.jsonl`` turns the records of a run under FG_PARITY_REPORT into that
section's tables.
"""
import functools
import sys

import pytest
import torch

import parity_common as P
import raster_restatement as R
from freegaussian_amd import _lib, ops
from parity_common import need_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOTS = dict(means2d=slice(0, 2), opacities=slice(2, 3), conics=slice(3, 6), absgrad=slice(6, 8))  # features: from slot 8


@functools.lru_cache(maxsize=None)
def _scene():
    return R.composite_scene(R.regime_scene(R.SEED))


@functools.lru_cache(maxsize=None)
def _kept():
    return R.margins(_scene())["kept"]


def _reference_of(sc, case, kept, exact_channels=()):
    """The float64 restatement of a case and the fp32 restatement's distances from it: dict(f64, ep64, compared, g64,
    forward_e32 {pixel class}, masks {pixel class: compared pixels}, e32 [group][tensor]{regime})."""
    _, ep32, _, g32 = R.epilogue_gradients(sc, case, torch.float32, kept, exact_channels=exact_channels)
    f64, ep64, compared, g64 = R.epilogue_gradients(sc, case, torch.float64, kept, exact_channels=exact_channels)
    masks = P.restrict(P.masks_of_index(R.pixel_class(), R.PIXEL_CLASSES), compared)
    forward_e32 = P.yardstick(masks, R.epilogue_forward_distance(ep32["out"], ep64), R.FLOOR)
    e32 = {g: {t: _row_e32(sc.labels, g32[g][0][t], g64[g][0][t], g64[g][1][t]) for t in R.TENSORS} for g in R.GROUPS}
    return dict(f64=f64, ep64=ep64, compared=compared, g64=g64, forward_e32=forward_e32, masks=masks, e32=e32)


@functools.lru_cache(maxsize=None)
def _reference(case_name):
    """Of a named case on the full scene; computed once."""
    return _reference_of(_scene(), R.CASE[case_name], _kept())


def _row_e32(labels, x32, x64, a64):
    return P.yardstick(P.live_row_masks(labels, x64), P.distance(x32, x64, a64, rows=True), R.FLOOR)


def _records(sc, channels):
    """[N,16] packed records (fg_pack_splats) of the scene's rows on the GPU."""
    n = sc.means2d.shape[0]
    m2, con, op, ft = (x.to(DEV).contiguous() for x in (sc.means2d, sc.conics, sc.opacities, sc.features(channels)))
    rec = torch.zeros(n, ops.SPLAT_FLOATS, dtype=torch.float32, device=DEV)
    ops._call("fg_pack_splats", n, channels, ops._ptr(m2), ops._ptr(con), ops._ptr(op), ops._ptr(ft), ops._ptr(rec), ops._stream())
    torch.cuda.synchronize()
    expect = torch.zeros(n, ops.SPLAT_FLOATS)
    expect[:, 0:2], expect[:, 2], expect[:, 3:6], expect[:, 6 : 6 + channels] = sc.means2d, sc.opacities, sc.conics, sc.features(channels)
    assert torch.equal(rec.cpu(), expect)
    return rec


def _background(case):
    return None if case.background is None else torch.tensor(case.background, dtype=torch.float32, device=DEV)


def _split(v_splats, channels):
    """The gradient record [N,16] as the five tensors of R.TENSORS; the slots behind the features must be zero."""
    v = v_splats.detach().cpu()
    assert v.shape[1] == ops.SPLAT_FLOATS and bool((v[:, 8 + channels :] == 0).all())
    out = {k: v[:, s].contiguous() for k, s in SLOTS.items()}
    out["features"] = v[:, 8 : 8 + channels].contiguous()
    return out


def _cotangents_on_gpu(channels, group, compared):
    """(v_out or None, v_alpha or None) in fp32 on the GPU: None for the output the group does not drive."""
    vo, va = R.cotangents(channels, group, compared)
    return (None if group == "alpha" else vo.float().to(DEV)), (None if group == "render" else va.float().to(DEV))


def _run_hip(sc, case, policy, compared, groups=R.GROUPS, repeats=2):
    """``ops.rasterize_splats`` under ``policy``, which must need no job list.  -> (forward, alpha of the same records without
    an epilogue, {(group, repeat): {tensor: grad}}) on the CPU.  Every backward has a forward of its own; the forwards must
    all be bit-identical."""
    C, W, H = case.channels, sc.width, sc.height
    ctx = ops.RasterContext(env={}, policy=ops.launch_policy(**policy))
    assert int(_lib.load().fg_raster_jobs_words(W, H, R.TILE, ctx.cfg())) == 0, "this policy builds a job list"
    offs, ids, rec, bg = sc.offsets.to(DEV), sc.flatten_ids.to(DEV), _records(sc, C), _background(case)
    res = {}
    with ops.use(ctx):
        with torch.no_grad():
            _, a0, _ = ops.rasterize_splats(rec, sc.means2d.to(DEV), C, W, H, R.TILE, offs, ids)
            plain_alpha = a0.cpu()[..., 0]
            r, a, last = ops.rasterize_splats(rec, sc.means2d.to(DEV), C, W, H, R.TILE, offs, ids, background=bg, n_clamp=case.n_clamp)
            fwd = dict(out=r.cpu(), alpha=a.cpu()[..., 0], last_ids=last.cpu())
        for group in groups:
            vo, va = _cotangents_on_gpu(C, group, compared)
            for rep in range(repeats):
                s, m = rec.clone().requires_grad_(True), sc.means2d.to(DEV).requires_grad_(True)
                r, a, last = ops.rasterize_splats(s, m, C, W, H, R.TILE, offs, ids, absgrad=True, background=bg, n_clamp=case.n_clamp)
                assert r.shape == (H, W, C) and a.shape == (H, W, 1) and last.shape == (H, W)
                out = dict(out=r.detach().cpu(), alpha=a.detach().cpu()[..., 0], last_ids=last.cpu())
                for k in fwd:
                    assert torch.equal(fwd[k], out[k]), f"the forward's {k} differs between two calls"
                # (render: the loss is formed from the image alone -- v_alphas reaches the kernel as NULL)
                loss = sum(x for x in ((r * vo).sum() if vo is not None else None, (a[..., 0] * va).sum() if va is not None else None)
                           if x is not None)  # fmt: skip
                loss.backward()
                torch.cuda.synchronize()
                assert torch.equal(m.grad, s.grad[:, 0:2]), "means2d.grad is not slots 0-1 of the record gradient"
                assert torch.equal(m.absgrad, s.grad[:, 6:8]), "means2d.absgrad is not slots 6-7 of the record gradient"
                res[(group, rep)] = _split(s.grad, C)
    return fwd, plain_alpha, res


def _run_entry_points(sc, case, policy, compared, groups=R.GROUPS, repeats=2):
    """The C entry points fg_raster_composite_fwd / _bwd called directly under ``policy``: no job list exists on this route
    whatever the policy (a mixed policy gives the positional one-wavefront-per-job launches).  -> as ``_run_hip`` without the
    plain alpha."""
    C, W, H, n = case.channels, sc.width, sc.height, sc.means2d.shape[0]
    cfg = ops.launch_policy(**policy)
    offs, ids, rec, bg = sc.offsets.to(DEV), sc.flatten_ids.to(DEV), _records(sc, C), _background(case)
    fwd, res = None, {}
    for group in groups:
        vo, va = _cotangents_on_gpu(C, group, compared)
        vo = torch.zeros(H, W, C, device=DEV) if vo is None else vo.contiguous()
        for rep in range(repeats):
            image, alphas = torch.empty(H, W, C, device=DEV), torch.empty(H, W, device=DEV)
            last, mask = torch.empty(H, W, dtype=torch.int32, device=DEV), torch.empty(H, W, dtype=torch.uint8, device=DEV)
            ops._call("fg_raster_composite_fwd", C, W, H, R.TILE, ops._ptr(rec), ops._ptr(offs), ops._ptr(ids), ops._ptr(bg),
                      case.n_clamp, ops._ptr(image), ops._ptr(alphas), ops._ptr(last), ops._ptr(mask), cfg.ptr(), ops._stream())  # fmt: skip
            v_splats = torch.zeros(n, ops.SPLAT_FLOATS, device=DEV)
            ops._call("fg_raster_composite_bwd", C, W, H, R.TILE, ops._ptr(rec), ops._ptr(offs), ops._ptr(ids), ops._ptr(bg),
                      case.n_clamp, ops._ptr(mask), ops._ptr(alphas), ops._ptr(last), ops._ptr(vo), ops._ptr(va), ops._ptr(v_splats),
                      cfg.ptr(), ops._stream())  # fmt: skip
            torch.cuda.synchronize()
            out = dict(out=image.cpu(), alpha=alphas.cpu(), last_ids=last.cpu())
            if fwd is None:
                fwd = out
            for k in fwd:
                assert torch.equal(fwd[k], out[k]), f"the forward's {k} differs between two calls"
            res[(group, rep)] = _split(v_splats, C)
    return fwd, res


def _check_forward(tag, fwd, plain_alpha, ref, failures):
    compared, ep64 = ref["compared"], ref["ep64"]
    if not torch.equal(fwd["last_ids"][compared], ref["f64"]["last_ids"][compared]):
        bad = ((fwd["last_ids"] != ref["f64"]["last_ids"]) & compared).nonzero()
        failures.append(f"{tag}: last_ids differ from float64 on {len(bad)} compared pixels, first (y, x) = {bad[0].tolist()}")
    if plain_alpha is not None and not torch.equal(fwd["alpha"], plain_alpha):
        failures.append(f"{tag}: alpha differs from the forward without an epilogue on {int((fwd['alpha'] != plain_alpha).sum())} pixels")
    blocked = compared[..., None] & ep64["blocked"]
    if not torch.equal(fwd["out"][blocked].double(), ep64["out"][blocked]):
        bad = (blocked & (fwd["out"].double() != ep64["out"])).nonzero()
        failures.append(f"{tag}: {len(bad)} blocked channels are not exactly float64's bound, first (y, x, c) = {bad[0].tolist()}")
    P.check(f"{tag}|forward|out|{{regime}}", ref["masks"], R.epilogue_forward_distance(fwd["out"], ep64), ref["forward_e32"], R.F, failures)


def _check_rows(tag, labels, group, tensor, x, x64, a64, e32, failures):
    """One tensor's rows against float64: the exact-zero rule, then F * E32 per regime.  Every ratio is recorded before
    anything is asserted."""
    assert x.shape == x64.shape, (tag, tensor, x.shape, x64.shape)
    wrong = P.exact_zero_rule(x, x64)
    if bool(wrong.any()):
        failures.append(f"{tag} {group} {tensor}: rows {wrong.nonzero().flatten().tolist()[:8]} "
                        f"({sorted(set(labels[int(i)] for i in wrong.nonzero().flatten()))}) are not zero where float64 is")  # fmt: skip
    d = P.distance(x, x64, a64, rows=True)
    P.check(f"{tag}|{group}|{tensor}|{{regime}}", P.live_row_masks(labels, x64), d, e32, R.F, failures)


def _check_case(tag, sc, ref, fwd, plain_alpha, res, failures):
    _check_forward(tag, fwd, plain_alpha, ref, failures)
    for (group, rep), grads in res.items():
        for tensor in R.TENSORS:
            x64, a64 = ref["g64"][group]
            _check_rows(tag, sc.labels, group, tensor, grads[tensor], x64[tensor], a64[tensor], ref["e32"][group][tensor], failures)


@pytest.mark.parametrize("case", R.EPILOGUE_CASES, ids=[c.name for c in R.EPILOGUE_CASES])
def test_every_row_classic(case):
    """Every named case under the default policy: the classic launch at 15 tiles, one pixel per lane."""
    failures = []
    ref = _reference(case.name)
    fwd, plain_alpha, res = _run_hip(_scene(), case, {}, ref["compared"])
    _check_case(f"classic-{case.name}", _scene(), ref, fwd, plain_alpha, res, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("ppt", [2, 4])
@pytest.mark.parametrize("name", ["model-rgb", "all-8"])
def test_every_row_classic_pixels_per_lane(name, ppt):
    """Two and four pixels per lane (two wavefronts / one per tile: the mask byte is written and read per pixel slot, the
    partial tiles' reads are clamped per slot).  Same bounds; the forward bit-identical to the default launch's."""
    failures = []
    case, ref = R.CASE[name], _reference(name)
    fwd, plain_alpha, res = _run_hip(_scene(), case, dict(ppt_fwd=ppt, ppt_bwd=ppt), ref["compared"])
    _check_case(f"classic-{name}-ppt{ppt}", _scene(), ref, fwd, plain_alpha, res, failures)
    default, _, _ = _run_hip(_scene(), case, {}, ref["compared"], groups=())
    for k in fwd:
        assert torch.equal(fwd[k], default[k]), f"{k} with {ppt} pixels per lane differs from the default launch's"
    assert not failures, "\n".join(failures)


# the first and the last pair of test_raster_rows_gpu.MIXED_CASES (tail4, tail2 | split4, split2 of both directions)
MIXED_CASES = [((7, 0), (20, 16)), ((2, 1), (0, 0))]


@pytest.mark.parametrize("tail,split", MIXED_CASES, ids=[f"tail{t[0]}-{t[1]}-split{s[0]}-{s[1]}" for t, s in MIXED_CASES])
def test_every_row_mixed_positional(tail, split):
    """The mixed launch (one wavefront per job: whole tiles, two-strip and single-strip jobs) with the epilogue, through the
    C entry points themselves: ``raster_fwd_any`` / ``raster_bwd_any`` get ``jobs = nullptr`` there, ``launch_*_mixed`` size
    the grid by ``mixed_grid`` ("positional jobs only") and every workgroup finds its job by ``job_of_block`` -- the route
    test_raster_rows_gpu.test_every_row_mixed takes for fg_raster_fwd.  (``ops.rasterize_splats`` would build a list under
    such a policy.)  Same row bounds; the forward bit-identical to the classic launch's."""
    policy = dict(tail4_fwd=tail[0], tail2_fwd=tail[1], tail4_bwd=tail[0], tail2_bwd=tail[1], split4_fwd=split[0],
                  split2_fwd=split[1], split4_bwd=split[0], split2_bwd=split[1])  # fmt: skip
    failures = []
    case, ref = R.CASE["model-rgb"], _reference("model-rgb")
    fwd, res = _run_entry_points(_scene(), case, policy, ref["compared"])
    _check_case(f"mixed-tail{tail[0]}-{tail[1]}", _scene(), ref, fwd, None, res, failures)
    classic, plain_alpha, _ = _run_hip(_scene(), case, {}, ref["compared"], groups=())
    for k in fwd:
        assert torch.equal(fwd[k], classic[k]), f"{k} of the mixed launch differs from the classic launch's"
    assert torch.equal(fwd["alpha"], plain_alpha)
    assert not failures, "\n".join(failures)


def _clamped_background(case):
    bg = torch.zeros(case.channels) if case.background is None else torch.tensor(case.background, dtype=torch.float32)
    bg[: case.n_clamp] = bg[: case.n_clamp].clamp(0.0, 1.0)
    return bg


def test_sub_scene_with_empty_tiles():
    """Without the huge rows -- and the rows listed in the first and in the last tile, which only the huge rows are sure to
    reach -- those tiles are empty: the image is exactly clamp(background) there, alpha exactly 0, last_ids the tile's
    start - 1.  Against the sub-scene's own reference (compositing couples rows)."""
    full, case = _scene(), R.CASE["model-rgb"]
    n_tiles = R.TILE_W * R.TILE_H
    corner = set(full.flatten_ids[: int(full.offsets[1])].tolist()) | set(full.flatten_ids[int(full.offsets[n_tiles - 1]) :].tolist())
    sc = full.take([i for i, l in enumerate(full.labels) if l != "huge" and i not in corner])
    lens = (sc.offsets[1:] - sc.offsets[:-1]).long()
    empty = (lens == 0).nonzero().flatten().tolist()
    assert {0, n_tiles - 1} <= set(empty) and int(lens.max()) > 256 and len(sc.labels) > 350
    failures = []
    ref = _reference_of(sc, case, R.margins(sc)["kept"])
    fwd, plain_alpha, res = _run_hip(sc, case, {}, ref["compared"])
    _check_case("no-huge", sc, ref, fwd, plain_alpha, res, failures)
    bg = _clamped_background(case)
    for t in empty:
        ty, tx = divmod(t, R.TILE_W)
        ys, xs = slice(ty * R.TILE, (ty + 1) * R.TILE), slice(tx * R.TILE, (tx + 1) * R.TILE)
        assert bool((fwd["out"][ys, xs] == bg).all()) and bool((fwd["alpha"][ys, xs] == 0).all()), t
        assert bool((fwd["last_ids"][ys, xs] == int(sc.offsets[t]) - 1).all()), t
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("n", [1, 70])
def test_empty_lists(n):
    """N >= 1 rows and every list empty: the whole image is exactly clamp(background), alpha 0, last_ids -1, and every
    gradient exactly zero in all three groups."""
    case = R.CASE["model-rgb"]
    sc = _scene().take(torch.arange(n)).without_lists()
    assert sc.flatten_ids.numel() == 0 and sc.means2d.shape[0] == n
    fwd, plain_alpha, res = _run_hip(sc, case, {}, torch.ones(sc.height, sc.width, dtype=torch.bool))
    assert bool((fwd["out"] == _clamped_background(case)).all()) and bool((fwd["alpha"] == 0).all())
    assert bool((plain_alpha == 0).all()) and bool((fwd["last_ids"] == -1).all())
    assert len(res) == 6
    for grads in res.values():
        for tensor in R.TENSORS:
            assert grads[tensor].shape[0] == n and bool((grads[tensor] == 0).all()), (n, tensor)


def test_the_bound_itself():
    """Channel 0 of every row is 0 and background[0] = 0: the channel is exactly 0 on every pixel, ON the bound, where the
    clamp passes the gradient (torch.clamp's rule; a non-strict comparison in the kernel would block it).  Its colour gradient
    obeys the row bound against float64 and is not zero on at least 90 % of the rows that contribute anywhere."""
    sc, case = R.bound_scene(_scene()), R.BOUND_CASE
    failures = []
    ref = _reference_of(sc, case, _kept(), exact_channels=(0,))
    fwd, plain_alpha, res = _run_hip(sc, case, {}, ref["compared"])
    _check_case("bound", sc, ref, fwd, plain_alpha, res, failures)
    assert bool((fwd["out"][..., 0] == 0).all())
    contributes = torch.zeros(len(sc.labels), dtype=torch.bool)
    for t, s, e, *_ in R._tiles(sc):
        if e > s:
            contributes[sc.flatten_ids[s:e].long()[ref["f64"]["include"][t].any(0)]] = True
    assert int(contributes.sum()) > 400
    _, ep32, _, g32 = R.epilogue_gradients(sc, case, torch.float32, _kept(), exact_channels=(0,))
    for (group, rep), grads in res.items():
        if group == "alpha":
            continue  # (no colour gradient without v_out)
        x64, a64 = (t["features"][:, :1] for t in ref["g64"][group])
        e32 = _row_e32(sc.labels, g32[group][0]["features"][:, :1], x64, a64)
        _check_rows("bound", sc.labels, group, "features0", grads["features"][:, :1], x64, a64, e32, failures)
        assert float((grads["features"][contributes, 0] != 0).float().mean()) >= 0.9, group
    assert not failures, "\n".join(failures)


def _report(path):
    """Markdown of a run's records (FG_PARITY_REPORT): per test case the compared and the blocked pixels, the worst row ratio
    and the worst forward ratio over both backward runs; per named case (group / tensor) x regime and pixel class with (E32)."""
    ratio, e32 = P.read_records(path, "test_raster_composite_rows_gpu")
    worst = max(ratio, key=ratio.get)
    print(f"Worst ratio {ratio[worst]:.2f} at {' | '.join(worst)}; {len(ratio)} (case, group, tensor, regime) cells; "
          f"{sum(v > R.F / 4 for v in ratio.values())} of them above F / 4 = {R.F / 4:g}.\n")  # fmt: skip
    tags = list(dict.fromkeys(k[0] for k in ratio))
    print("| case | compared pixels | blocked (pixels with a blocked channel; channels) | worst row ratio | at (group, tensor, regime) "
          "| worst forward ratio | at pixel class |\n|---|---|---|---|---|---|---|")  # fmt: skip
    for tag in tags:
        rows = {k: v for k, v in ratio.items() if k[0] == tag and k[1] != "forward"}
        fw = {k: v for k, v in ratio.items() if k[0] == tag and k[1] == "forward"}
        kr, kf = max(rows, key=rows.get), max(fw, key=fw.get)
        name = next((c.name for c in R.EPILOGUE_CASES if tag in (f"classic-{c.name}", f"classic-{c.name}-ppt2", f"classic-{c.name}-ppt4")),
                    "model-rgb" if tag.startswith("mixed") else None)  # fmt: skip
        counts = ("", "")
        if name is not None:
            ref = _reference(name)
            b = ref["ep64"]["blocked"][ref["compared"]]
            counts = (str(int(ref["compared"].sum())), f"{int(b.any(dim=1).sum())}; {int(b.sum())}")
        print(f"| {tag} | {counts[0]} | {counts[1]} | {rows[kr]:.2f} | {', '.join(kr[1:])} | {fw[kf]:.2f} | {kf[3]} |")
    print()
    regimes = [k for k in R.COUNTS]
    for tag in tags:
        if tag.count("-ppt") or not tag.startswith("classic"):
            continue
        print(f"### {tag}\n\n| output | " + " | ".join(R.PIXEL_CLASSES) + " |\n|---|" + "---|" * len(R.PIXEL_CLASSES))
        cells = [f"{ratio[(tag, 'forward', 'out', c)]:.2f} ({e32[(tag, 'forward', 'out', c)]:.1e})" for c in R.PIXEL_CLASSES]
        print("| out | " + " | ".join(cells) + " |")
        print("\n| group / tensor | " + " | ".join(regimes) + " |\n|---|" + "---|" * len(regimes))
        for group in R.GROUPS:
            for tensor in R.TENSORS:
                cells = [f"{ratio[(tag, group, tensor, r)]:.2f} ({e32[(tag, group, tensor, r)]:.1e})" if (tag, group, tensor, r) in ratio
                         else "" for r in regimes]  # fmt: skip
                print(f"| {group} / {tensor} | " + " | ".join(cells) + " |")
        print()


if __name__ == "__main__":
    _report(sys.argv[1])
