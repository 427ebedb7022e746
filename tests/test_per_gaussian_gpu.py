"""The per-Gaussian stage (csrc/preprocess.hip, csrc/project_math.h) in isolation: ``ops.preprocess`` / ``ops.preprocess_raw``
called directly -- no binning, no raster -- on the regime scene of tests/per_gaussian_restatement.py, every row compared with
the float64 restatement, one cotangent group at a time.

BACKWARD, per row, for every input tensor and every cotangent group:
    a row whose float64 gradient is exactly zero is zero on the GPU (no NaN, no denormal noise; the sign of a zero aside);
    every other row:  |g_hip - g64|_2 / |g64|_2  <=  F * E32(regime, group, tensor)
tests/parity_common.py has the protocol (E32, the floor, F); here the denominator is the float64 row itself.  E32 is 1e-6 on
most regimes and 5e-4 on the compensation gradient of the clamped rows, where the blur is nothing against the covariance and
the three terms cancel.  F and FLOOR are per_gaussian_restatement's, the recorded table is in
profiles/per_gaussian_row_parity.md; the host test proves that every autograd-level mutant of the restatement is at least
4 * F * E32 away.  NO row is left out: tests/test_per_gaussian_host.py asserts that no row is within 1e-3 of a branch boundary.

The cotangents reach the kernel as in production: ``(out * cotangent).sum()``, outputs a group does not drive get no gradient
(``v_depths`` / ``v_conics`` arrive as None), and the record's cotangent passes a stand-in for the raster backward (``_RecordTap``)
that hands on the GRADIENT record (features from slot 8) and, as the gradient of ``means2d``, the strided view of its xy slots.

FORWARD: plain form -- radii and tiles_touched equal the fp32 oracle's, means2d / depths / conics equal the fp32 restatement
bit for bit (on clamped and sub-pixel rows too); raw form -- radii equal, every output row within F x the fp32 restatement's
own row distance from float64.  Record rows: by that rule in both forms; slots beyond the channel count exactly 0.

``python tests/test_per_gaussian_gpu.py REPORT.jsonl`` turns the records of a run under FG_PARITY_REPORT into the table of
profiles/per_gaussian_row_parity.md.
"""
import functools
import sys

import pytest
import torch

import parity_common as P
import per_gaussian_restatement as R
from freegaussian_amd import ops
from oracle import raster_oracle as O
from parity_common import need_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 0  # (tests/test_per_gaussian_host.py checks this scene's margins)
TILE = 16


@functools.lru_cache(maxsize=None)
def _scene():
    return R.regime_scene(SEED)


@functools.lru_cache(maxsize=None)
def _reference(path_name, pose=False):
    """(o32, g32, o64, g64, E32) of a path on the full scene; E32[group][tensor][regime]."""
    sc = _scene()
    o32, g32 = R.gradients(sc, R.PATHS[path_name], torch.float32, pose=pose)
    o64, g64 = R.gradients(sc, R.PATHS[path_name], torch.float64, pose=pose)
    e32 = {g: {t: _row_e32(sc.labels, g32[g][t], g64[g][t]) for t in g64[g] if t != "viewmat"} for g in g64}
    return o32, g32, o64, g64, e32


def _row_e32(labels, x32, x64):
    return P.yardstick(P.live_row_masks(labels, x64), P.distance(x32, x64, x64.abs(), rows=True), R.FLOOR)


class _RecordTap(torch.autograd.Function):
    """Stands where ops.rasterize_splats stands in production: consumes the records (and ``means2d``, a routing input);
    its backward returns the gradient record -- features from slot 8 -- and the strided xy view of it for ``means2d``."""

    @staticmethod
    def forward(ctx, splats, means2d):
        ctx.m2_shape = means2d.shape
        return splats.clone()

    @staticmethod
    def backward(ctx, v_record):
        v_splats = R.to_gradient_record(v_record)
        return v_splats, v_splats[:, 0:2].view(ctx.m2_shape)


def _run_hip(scene, path, groups=None, pose=False, index=None):
    """-> (outs, {group: {tensor: grad}}) on the CPU, from one forward call and one backward per cotangent group.
    ``index``: ``scene`` is these rows of the full scene -- every row keeps the cotangents it has there."""
    ctx = ops.RasterContext()
    ctx.sh_jacobian = path["note"]
    inp = {k: v.to(DEV).requires_grad_(True) for k, v in scene.inputs(path["form"], path["sh_degree"], path["k_stored"],
                                                                      path["n_extra"]).items()}  # fmt: skip
    vm = scene.viewmat.to(DEV).requires_grad_(pose)
    K = scene.K.to(DEV)
    kw = dict(antialiased=path["antialiased"], with_depth=path["with_depth"], tile_size=TILE)
    with ops.use(ctx):
        if path["form"] == "plain":
            out = ops.preprocess(inp["means"], inp["quats"], inp["scales"], inp["opacities"], inp["colors"], inp.get("extra"), vm,
                                 K, scene.width, scene.height, sh_degree=path["sh_degree"], **kw)  # fmt: skip
        else:
            out = ops.preprocess_raw(inp["means"], inp["quats"], inp["log_scales"], inp["opacity_logits"], inp["features_dc"],
                                     inp["features_rest"], vm, K, scene.width, scene.height, path["sh_degree"],
                                     d_quats=inp.get("d_quats"), d_scales=inp.get("d_scales"), extra=inp.get("extra"), **kw)  # fmt: skip
        radii, means2d, depths, conics, tiles, splats = out
        outs = dict(means2d=means2d, depths=depths, conics=conics, record=_RecordTap.apply(splats, means2d))
        wrt = dict(inp, viewmat=vm) if pose else inp
        res = {}
        for group in groups or R.groups_of(path["with_depth"], path["n_extra"]):
            ct = R.cotangents(len(_scene().labels), group, path["with_depth"], path["n_extra"])
            ct = ct if index is None else {k: v[index] for k, v in ct.items()}
            loss = sum((outs[k] * v.float().to(DEV)).sum() for k, v in ct.items())
            gs = torch.autograd.grad(loss, list(wrt.values()), retain_graph=True, allow_unused=True)
            res[group] = {k: (torch.zeros_like(t) if g is None else g).cpu() for (k, t), g in zip(wrt.items(), gs)}
        torch.cuda.synchronize()
    outs = {k: v.detach().cpu() for k, v in dict(outs, radii=radii, tiles=tiles, record=splats).items()}
    return outs, res


def _check_rows(tag, labels, what, x, x32_e, x64, failures):
    """One tensor's rows against float64: the exact-zero rule, then F * E32 per regime (``x32_e``: regime -> E32).  Every
    ratio is recorded before anything is asserted."""
    wrong = P.exact_zero_rule(x, x64)
    if bool(wrong.any()):
        failures.append(f"{tag} {what}: rows {wrong.nonzero().flatten().tolist()[:8]} are not zero where float64 is")
    d = P.distance(x, x64, x64.abs(), rows=True)
    P.check(f"{tag}|{{regime}}|{what}", P.live_row_masks(labels, x64), d, x32_e, R.F, failures)


def _check_backward(tag, scene, path_name, hip, failures, index=None):
    _, _, _, g64, e32 = _reference(path_name)
    for group, tensors in hip.items():
        for tensor, g in tensors.items():
            if tensor == "viewmat":
                continue
            ref = g64[group][tensor] if index is None else g64[group][tensor][index]
            assert g.shape == ref.shape, (group, tensor)
            _check_rows(tag, scene.labels, f"{group}|{tensor}", g, e32[group][tensor], ref, failures)


def _output_yardstick(path_name):
    sc = _scene()
    o32, _, o64, _, _ = _reference(path_name)
    return {k: _row_e32(sc.labels, o32[k], o64[k]) for k in ("means2d", "depths", "conics", "record")}


def _check_forward(tag, scene, path_name, outs, failures, index=None):
    path = R.PATHS[path_name]
    o32, _, o64, _, _ = _reference(path_name)
    pick = (lambda t: t) if index is None else (lambda t: t[index])
    assert torch.equal(outs["radii"], pick(o32["radii"])) and torch.equal(outs["radii"], pick(o64["radii"]))
    tw, th = (scene.width + TILE - 1) // TILE, (scene.height + TILE - 1) // TILE
    x0, y0, x1, y1 = O.tile_rects(pick(o32["means2d"]), pick(o32["radii"]), TILE, tw, th)
    assert torch.equal(outs["tiles"].long(), (x1 - x0) * (y1 - y0))
    assert torch.equal(outs["record"][:, :2], outs["means2d"]) and torch.equal(outs["record"][:, 3:6], outs["conics"])
    channels = 3 + path["with_depth"] + path["n_extra"]
    assert bool((outs["record"][:, R.FEAT0 + channels :] == 0).all())
    assert bool((outs["record"][outs["radii"] == 0] == 0).all())
    if path["form"] == "plain":
        for k in ("means2d", "depths", "conics"):
            assert torch.equal(outs[k], pick(o32[k])), f"{tag}: {k} differs from the fp32 restatement"
        if path["with_depth"]:
            assert torch.equal(outs["record"][:, R.FEAT0 + 3], outs["depths"])
    e32 = _output_yardstick(path_name)
    for k in ("means2d", "depths", "conics", "record"):
        _check_rows(tag, scene.labels, f"forward|{k}", outs[k], e32[k], pick(o64[k]), failures)


@pytest.mark.parametrize("path_name", list(R.PATHS))
def test_every_row_of_every_path(path_name):
    """Forward and backward of one path of the table on the full scene (192 rows, three workgroups), every cotangent group."""
    sc = _scene()
    outs, hip = _run_hip(sc, R.PATHS[path_name])
    failures = []
    _check_forward(path_name, sc, path_name, outs, failures)
    _check_backward(path_name, sc, path_name, hip, failures)
    assert not failures, "\n".join(failures)


EDGE_PATHS = ("plain-sh3-depth-extra", "delta-sh3-depth-rows", "raw-sh0-k1-aa-depth-extra", "plain-direct-aa-depth-extra")


@pytest.mark.parametrize("n", [1, 31, 33, 64, 65])
def test_row_block_edges(n):
    """The shuffled scene truncated to N rows: one row, a half slab less / more than one row, a whole workgroup, one row
    more -- every row still alone with its inputs (the reference is the full scene's, sliced)."""
    full = _scene()
    sc = full.take(slice(0, n))
    failures = []
    for path_name in EDGE_PATHS:
        outs, hip = _run_hip(sc, R.PATHS[path_name], index=slice(0, n))
        tag = f"N={n}|{path_name}"
        _check_forward(tag, sc, path_name, outs, failures, slice(0, n))
        _check_backward(tag, sc, path_name, hip, failures, slice(0, n))
    assert not failures, "\n".join(failures)


def _layout(kind):
    """Row order with a dead block, as an index into the scene (culled rows repeat to fill it): ``half`` -- rows 32..63 of
    the first workgroup all culled; ``group`` -- the whole second workgroup culled."""
    sc = _scene()
    dead, live = sc.rows(*R.CULLED), sc.rows(*R.VISIBLE_REGIMES)
    if kind == "half":
        assert len(dead) >= 32
        return torch.cat([live[:32], dead[:32], live[32:]])
    fill = dead.repeat(64 // len(dead) + 1)[:64]
    return torch.cat([live[:64], fill, live[64:]])


@pytest.mark.parametrize("kind", ["half", "group"])
def test_dead_blocks_backward_from_the_coefficient_rows(kind):
    """A whole half slab / a whole workgroup of culled rows, the backward recomputing the SH sums from the coefficient
    rows in two 32-row halves (no note): the live rows around the dead block are what they are in the shuffled scene.
    (With -DFG_PREPROCESS_SKIP_CULLED=1, a build-time switch that is off in the product build, these are the layouts in
    which a whole staging step of that backward has no live row to fetch.)"""
    index = _layout(kind)
    sc = _scene().take(index)
    radii = _reference("plain-sh3-aa-rows")[2]["radii"][index]
    block = slice(32, 64) if kind == "half" else slice(64, 128)
    assert bool((radii[block] == 0).all()) and bool((radii[:32] > 0).all()) and bool((radii[128:] > 0).all())
    failures = []
    for path_name in ("plain-sh3-aa-rows", "delta-sh3-depth-rows", "raw-sh1-k4-rows"):
        assert not R.PATHS[path_name]["note"]
        outs, hip = _run_hip(sc, R.PATHS[path_name], index=index)
        tag = f"dead-{kind}|{path_name}"
        _check_forward(tag, sc, path_name, outs, failures, index)
        _check_backward(tag, sc, path_name, hip, failures, index)
    assert not failures, "\n".join(failures)


POSE_PATHS = ("plain-direct-aa-depth-extra", "plain-sh3-depth-extra", "plain-sh3-aa-rows", "plain-sh1-k4-aa-depth",
              "raw-sh3-aa-depth-extra", "delta-sh1-k16-aa-extra", "delta-sh3-depth-rows")  # fmt: skip


@pytest.mark.parametrize("path_name", POSE_PATHS)
def test_pose_gradient(path_name):
    """``viewmat.requires_grad_()``: the 12 numbers of d loss / d [W | t] per cotangent group against the float64
    restatement's, within F x the fp32 restatement's own distance (floored like E32); exactly zero where float64 is (a
    group the pose does not reach).  The parameter gradients of the same call stay within their row bounds."""
    sc = _scene()
    _, g32, _, g64, _ = _reference(path_name, True)
    _, hip = _run_hip(sc, R.PATHS[path_name], pose=True)
    failures = []
    reached = 0
    for group in hip:
        v, v32, v64 = hip[group]["viewmat"][:3], g32[group]["viewmat"][:3], g64[group]["viewmat"][:3]
        if not bool((v64 != 0).any()):
            if bool((v != 0).any()):
                failures.append(f"{path_name} {group}: the pose gradient is not zero where float64 is")
            continue
        reached += 1
        e32 = max(R.vector_distance(v32, v64), R.FLOOR)
        ratio = R.vector_distance(v, v64) / e32
        P.check_cell(f"{path_name}|pose|{group}|viewmat", ratio, e32, R.F, failures, "the pose gradient")
    assert reached >= 4
    _check_backward(f"pose|{path_name}", sc, path_name, hip, failures)
    assert not failures, "\n".join(failures)


def _report(path):
    """Markdown of a run's records (FG_PARITY_REPORT): per path of the full-scene test, (group / tensor) x regime, the
    worst HIP ratio and (E32); one line per other test."""
    # (N=..|path, dead-..|path, pose|path: one field)
    ratio, e32 = ({k if k[0] in R.PATHS else (f"{k[0]} {k[1]}",) + k[2:]: v for k, v in d.items()}
                  for d in P.read_records(path, "test_per_gaussian_gpu"))  # fmt: skip
    worst = max(ratio, key=ratio.get)
    print(f"Worst ratio {ratio[worst]:.2f} at {' | '.join(worst)}; {len(ratio)} (test, path, regime, group, tensor) cells.\n")
    regimes = list(R.VISIBLE_REGIMES) + ["pose"]  # (pose: the 12 numbers of the camera-pose gradient, rows "<group> / viewmat")
    others = {}
    for key, v in ratio.items():
        if key[0] not in R.PATHS:
            others[key[0]] = max(others.get(key[0], (0.0, None)), (v, key[1:]))
    print("| test and path | worst ratio | at (regime, group, tensor) |\n|---|---|---|")
    for tag, (v, where) in others.items():
        print(f"| {tag} | {v:.2f} | {', '.join(where)} |")
    print()
    for tag in R.PATHS:
        print(f"### {tag}\n\n| group / tensor | " + " | ".join(regimes) + " |\n|---|" + "---|" * len(regimes))
        for what in dict.fromkeys(k[2:] for k in ratio if k[0] == tag):
            cells = [f"{ratio[(tag, r) + what]:.2f} ({e32[(tag, r) + what]:.1e})" if (tag, r) + what in ratio else "" for r in regimes]
            print(f"| {' / '.join(what)} | " + " | ".join(cells) + " |")
        print()


if __name__ == "__main__":
    _report(sys.argv[1])
