"""The compositing stage (csrc/raster.hip) in isolation: ``ops.rasterize_to_pixels`` -- fg_pack_splats, fg_raster_fwd,
fg_raster_bwd, fg_unpack_grads; no preprocess, no binning, no job lists -- on the regime scene of
tests/raster_restatement.py (72 x 40 pixels, explicit lists), every pixel and every row compared with the float64
restatement, one cotangent group at a time, the launch chosen through the policy alone.

FORWARD, on every kept pixel (tests/test_raster_rows_host.py: 99 % of them; the others sit on a decision threshold):
    last_ids equal the float64 restatement's -- no knife-edge quota;
    |render - r64|_inf / sum_i w_i |c_i|_inf  and  |alpha - a64|  <=  F * E32(pixel class)
BACKWARD, per cotangent group (render / alpha / both), per tensor (means2d, absgrad, conics, features, opacities):
    a row whose float64 gradient is exactly zero is zero on the GPU (faint rows, rows behind the wall, ...);
    every other row:  |g_hip - g64|_2 / |A64|_2  <=  F * E32(regime, group, tensor)
tests/parity_common.py has the protocol (A, E32, the floor, F); F and FLOOR are raster_restatement's, the recorded table is
in profiles/raster_row_parity.md.  Each backward runs twice (the order of its float atomics differs) and both runs are held
to the bound; the forward is bit-identical across all of them.

``python tests/test_raster_rows_gpu.py REPORT.jsonl`` turns the records of a run under FG_PARITY_REPORT into the tables of
profiles/raster_row_parity.md.
"""
import functools
import sys

import pytest
import torch

import parity_common as P
import raster_restatement as R
from freegaussian_amd import ops
from parity_common import need_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _scene():
    return R.regime_scene(R.SEED)


@functools.lru_cache(maxsize=None)
def _kept():
    return R.margins(_scene())["kept"]


@functools.lru_cache(maxsize=None)
def _reference(channels):
    """(f64, g64, forward E32 per pixel class, row E32[group][tensor][regime]) of the full scene; computed once."""
    sc, kept = _scene(), _kept()
    f32, g32 = R.gradients(sc, channels, torch.float32, kept)
    f64, g64 = R.gradients(sc, channels, torch.float64, kept)
    e32 = {g: {t: _row_e32(sc.labels, g32[g][0][t], g64[g][0][t], g64[g][1][t]) for t in R.TENSORS} for g in R.GROUPS}
    return f64, g64, _forward_e32(f32, f64, kept), e32


def _row_e32(labels, x32, x64, a64):
    return P.yardstick(P.live_row_masks(labels, x64), P.distance(x32, x64, a64, rows=True), R.FLOOR)


def _forward_e32(f32, f64, kept):
    d, masks = R.forward_distance(f32, f64), R.pixel_masks(f64, kept)
    return {what: P.yardstick(masks[what], d[what], R.FLOOR) for what in d}


def _run_hip(scene, channels, policy, kept, groups=R.GROUPS, repeats=2):
    """-> (forward, {(group, repeat): {tensor: grad}}) on the CPU.  Every backward has a forward of its own (the node hands
    ``absgrad`` to the tensor it was called with, once); the forwards must all be bit-identical."""
    ctx = ops.RasterContext(env={}, policy=ops.launch_policy(**policy))
    offs, ids = scene.offsets.to(DEV), scene.flatten_ids.to(DEV)
    fwd, res = None, {}
    with ops.use(ctx):
        for group in groups:
            vr, va = R.cotangents(channels, group, kept)
            for rep in range(repeats):
                m2, con, ft, op = (x.to(DEV).requires_grad_(True) for x in (scene.means2d, scene.conics, scene.features(channels),
                                                                            scene.opacities))  # fmt: skip
                r, a, last = ops.rasterize_to_pixels(m2, con, ft, op, scene.width, scene.height, R.TILE, offs, ids, absgrad=True)
                assert r.shape == (scene.height, scene.width, channels) and a.shape == (scene.height, scene.width, 1)
                out = dict(render=r.detach().cpu(), alpha=a.detach().cpu()[..., 0], last_ids=last.cpu())
                if fwd is None:
                    fwd = out
                for k in fwd:
                    assert torch.equal(fwd[k], out[k]), f"the forward's {k} differs between two calls"
                loss = 0.0
                if group != "alpha":
                    loss = loss + (r * vr.float().to(DEV)).sum()
                if group != "render":
                    loss = loss + (a[..., 0] * va.float().to(DEV)).sum()
                loss.backward()
                torch.cuda.synchronize()
                res[(group, rep)] = dict(means2d=m2.grad.cpu(), absgrad=m2.absgrad.cpu(), conics=con.grad.cpu(),
                                         features=ft.grad.cpu(), opacities=op.grad.cpu()[:, None])  # fmt: skip
    return fwd, res


def _check_forward(tag, fwd, f64, e32, kept, failures):
    if not torch.equal(fwd["last_ids"][kept], f64["last_ids"][kept]):
        bad = ((fwd["last_ids"] != f64["last_ids"]) & kept).nonzero()
        failures.append(f"{tag}: last_ids differ from float64 on {len(bad)} kept pixels, first (y, x) = {bad[0].tolist()}")
    d = R.forward_distance(fwd, f64)
    nothing = kept & (f64["weight"] == 0)
    if bool((fwd["render"][nothing] != 0).any()):
        failures.append(f"{tag}: render is not zero on pixels nothing contributes to")
    masks = R.pixel_masks(f64, kept)
    for what, v in d.items():
        P.check(f"{tag}|forward|{what}|{{regime}}", masks[what], v, e32[what], R.F, failures)


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


def _check_full_scene(tag, channels, policy, failures):
    sc, kept = _scene(), _kept()
    f64, g64, fwd_e32, e32 = _reference(channels)
    fwd, res = _run_hip(sc, channels, policy, kept)
    _check_forward(tag, fwd, f64, fwd_e32, kept, failures)
    for (group, rep), grads in res.items():
        for tensor in R.TENSORS:
            _check_rows(tag, sc.labels, group, tensor, grads[tensor], g64[group][0][tensor], g64[group][1][tensor],
                        e32[group][tensor], failures)  # fmt: skip
    return fwd, res


# channels, pixels per lane (0: the library's own choice at 15 tiles -- the classic launch, one pixel per lane)
CLASSIC_CASES = [(3, 0), (3, 2), (3, 4), (1, 0), (4, 0), (8, 0)]


@pytest.mark.parametrize("channels,ppt", CLASSIC_CASES)
def test_every_row_classic(channels, ppt):
    """The classic launch, four / two / one wavefronts per tile (staging batches of 256 / 128 / 64 entries: the deep list
    crosses each), one to eight channels."""
    failures = []
    _check_full_scene(f"classic-C{channels}-ppt{ppt}", channels, dict(ppt_fwd=ppt, ppt_bwd=ppt) if ppt else {}, failures)
    assert not failures, "\n".join(failures)


# tail4, tail2 | split4, split2 of both directions: the pairs of test_gpu_parity.test_mixed_launch_equals_classic_launch,
# and one that leaves whole-tile jobs (an XCD's band is one row of five tiles here: two whole-tile jobs, one tile as two
# two-strip jobs, two tiles as four single-strip jobs each; the first pair makes every tile four single-strip jobs, the
# second two tiles two-strip and three single-strip)
MIXED_CASES = [((7, 0), (20, 16)), ((3, 5), (2, 1)), ((2, 1), (0, 0))]


@pytest.mark.parametrize("tail,split", MIXED_CASES, ids=[f"tail{t[0]}-{t[1]}-split{s[0]}-{s[1]}" for t, s in MIXED_CASES])
def test_every_row_mixed(tail, split):
    """The mixed launch (one wavefront per job: whole tiles, two-strip and single-strip jobs) forced on this 5 x 3 grid.
    Through ``rasterize_to_pixels`` it has no job list: ``raster_fwd_any`` / ``raster_bwd_any`` pass ``jobs = nullptr`` and
    ``launch_*_mixed`` size the grid by ``mixed_grid`` ("positional jobs only"), every workgroup finding its job by
    ``job_of_block`` -- the content thresholds (split*) need a list and change nothing here.  Same row bounds; the forward
    bit-identical to the classic launch's."""
    policy = dict(tail4_fwd=tail[0], tail2_fwd=tail[1], tail4_bwd=tail[0], tail2_bwd=tail[1], split4_fwd=split[0],
                  split2_fwd=split[1], split4_bwd=split[0], split2_bwd=split[1])  # fmt: skip
    failures = []
    fwd, _ = _check_full_scene(f"mixed-tail{tail[0]}-{tail[1]}", 3, policy, failures)
    classic = _forward_only(_scene(), 3, {})
    for k in fwd:
        assert torch.equal(fwd[k], classic[k]), f"{k} of the mixed launch differs from the classic launch's"
    assert not failures, "\n".join(failures)


def _forward_only(scene, channels, policy):
    ctx = ops.RasterContext(env={}, policy=ops.launch_policy(**policy))
    with ops.use(ctx), torch.no_grad():
        r, a, last = ops.rasterize_to_pixels(scene.means2d.to(DEV), scene.conics.to(DEV), scene.features(channels).to(DEV),
                                             scene.opacities.to(DEV), scene.width, scene.height, R.TILE, scene.offsets.to(DEV),
                                             scene.flatten_ids.to(DEV))  # fmt: skip
        torch.cuda.synchronize()
    return dict(render=r.cpu(), alpha=a.cpu()[..., 0], last_ids=last.cpu())


def _check_sub_scene(tag, sc, failures):
    """A sub-scene against ITS OWN reference (compositing couples rows), default policy, three channels."""
    m = R.margins(sc)
    kept = m["kept"]
    f32, g32 = R.gradients(sc, 3, torch.float32, kept)
    f64, g64 = R.gradients(sc, 3, torch.float64, kept)
    fwd, res = _run_hip(sc, 3, {}, kept)
    _check_forward(tag, fwd, f64, _forward_e32(f32, f64, kept), kept, failures)
    for (group, rep), grads in res.items():
        for tensor in R.TENSORS:
            e32 = _row_e32(sc.labels, g32[group][0][tensor], g64[group][0][tensor], g64[group][1][tensor])
            _check_rows(tag, sc.labels, group, tensor, grads[tensor], g64[group][0][tensor], g64[group][1][tensor], e32, failures)
    return fwd, res, f64


def test_sub_scenes():
    full = _scene()
    failures = []
    # without the huge rows -- and the rows listed in the first and in the last tile, a whole one and a partial one, which
    # only the huge rows are sure to reach -- those tiles are empty: exactly zero there, last_ids = the tile's start - 1
    n_tiles = R.TILE_W * R.TILE_H
    corner = set(full.flatten_ids[: int(full.offsets[1])].tolist()) | set(full.flatten_ids[int(full.offsets[n_tiles - 1]) :].tolist())
    sc = full.take([i for i, l in enumerate(full.labels) if l != "huge" and i not in corner])
    lens = (sc.offsets[1:] - sc.offsets[:-1]).long()
    empty = (lens == 0).nonzero().flatten().tolist()
    assert {0, n_tiles - 1} <= set(empty) and int(lens.max()) > 256 and len(sc.labels) > 350
    fwd, _, _ = _check_sub_scene("no-huge", sc, failures)
    for t in empty:
        ty, tx = divmod(t, R.TILE_W)
        ys, xs = slice(ty * R.TILE, (ty + 1) * R.TILE), slice(tx * R.TILE, (tx + 1) * R.TILE)
        assert bool((fwd["render"][ys, xs] == 0).all()) and bool((fwd["alpha"][ys, xs] == 0).all()), t
        assert bool((fwd["last_ids"][ys, xs] == int(sc.offsets[t]) - 1).all()), t
    # one single splat
    one = full.take(full.rows("plain")[:1])
    fwd, res, f64 = _check_sub_scene("one-splat", one, failures)
    assert float(f64["alpha"].max()) > 0.2 and not bool(P.zero_rows(res[("both", 0)]["means2d"]).any())
    # N >= 1 rows and every list empty: images all zero, every gradient exactly zero
    for n in (1, 70):
        sc = full.take(torch.arange(n)).without_lists()
        assert sc.flatten_ids.numel() == 0 and sc.means2d.shape[0] == n
        fwd, res = _run_hip(sc, 3, {}, torch.ones(sc.height, sc.width, dtype=torch.bool))
        assert bool((fwd["render"] == 0).all()) and bool((fwd["alpha"] == 0).all()) and bool((fwd["last_ids"] == -1).all())
        for grads in res.values():
            for tensor in R.TENSORS:
                assert grads[tensor].shape[0] == n and bool((grads[tensor] == 0).all()), (n, tensor)
    assert not failures, "\n".join(failures)


def _report(path):
    """Markdown of a run's records (FG_PARITY_REPORT): per test case, (group / tensor) x regime and (output) x pixel class,
    the worst HIP ratio over both backward runs and (E32)."""
    ratio, e32 = P.read_records(path, "test_raster_rows_gpu")
    worst = max(ratio, key=ratio.get)
    print(f"Worst ratio {ratio[worst]:.2f} at {' | '.join(worst)}; {len(ratio)} (case, group, tensor, regime) cells.\n")
    tags = list(dict.fromkeys(k[0] for k in ratio))
    print("| case | worst row ratio | at (group, tensor, regime) | worst forward ratio | at (output, pixel class) |\n|---|---|---|---|---|")
    for tag in tags:
        rows = {k: v for k, v in ratio.items() if k[0] == tag and k[1] != "forward"}
        fw = {k: v for k, v in ratio.items() if k[0] == tag and k[1] == "forward"}
        kr, kf = max(rows, key=rows.get), max(fw, key=fw.get)
        print(f"| {tag} | {rows[kr]:.2f} | {', '.join(kr[1:])} | {fw[kf]:.2f} | {', '.join(kf[2:])} |")
    print()
    regimes = [k for k in R.COUNTS]
    for tag in tags:
        if not tag.startswith(("classic", "mixed")):
            continue
        print(f"### {tag}\n\n| output | " + " | ".join(R.PIXEL_CLASSES) + " |\n|---|" + "---|" * len(R.PIXEL_CLASSES))
        for what in ("render", "alpha"):
            cells = [f"{ratio[(tag, 'forward', what, c)]:.2f} ({e32[(tag, 'forward', what, c)]:.1e})" for c in R.PIXEL_CLASSES]
            print(f"| {what} | " + " | ".join(cells) + " |")
        print("\n| group / tensor | " + " | ".join(regimes) + " |\n|---|" + "---|" * len(regimes))
        for group in R.GROUPS:
            for tensor in R.TENSORS:
                cells = [f"{ratio[(tag, group, tensor, r)]:.2f} ({e32[(tag, group, tensor, r)]:.1e})" if (tag, group, tensor, r) in ratio
                         else "" for r in regimes]  # fmt: skip
                print(f"| {group} / {tensor} | " + " | ".join(cells) + " |")
        print()


if __name__ == "__main__":
    _report(sys.argv[1])
