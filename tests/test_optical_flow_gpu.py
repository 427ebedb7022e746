"""``ops.optical_flow`` / ``ops.optical_flow_pyramid`` (csrc/optflow.hip) on the GPU against tests/optical_flow_restatement.py,
the CPU statement of include/fgraster.h "OF", under the float64 protocol of tests/parity_common.py.

1 PYRAMID      every level against float64, den = the absolute accumulation of the 25 taps (level 0: of the grey sum), uint8 RGB,
               float RGB and float grey at 97 x 131 and 64 x 80, regimes border (taps clamped) / interior: <= F_PYRAMID * E32.
2 ONE STEP     levels = 1, iters = 1, ``init`` given, no second direction: u1 per pixel and component against float64,
               den = |u0| + |G^-1| sum |It grad A|, regimes tercile of the smaller eigenvalue x border / interior window, at
               24 x 40 and 97 x 131 (windows clamped on all four sides, a partial tile, sub-pixel init): <= F_STEP * E32.
3 WHOLE CALL   the affine cases at 97 x 131 and 128 x 160 and the disc pair, 4 levels, the defaults.  Where kernel and float64
               restatement are both valid: |u - u64|_2 / (1 + |u64|_2) <= F_CALL * E32 per eigenvalue tercile, E32 the fp32
               restatement's distance over the same pixels.  Pixels whose validity differs: their share of the interior <=
               max(2 x the share by which the fp32 restatement differs from the float64 one, 0.1 %) -- another summation order
               tips other pixels on a basin or threshold edge.  Mean error against the analytic flow on the valid interior
               <= 1.05 x the float64 restatement's + 1e-3 px.
4 STRUCTURE    bit-equal runs; the flow does not depend on ``consistency``; never valid where x + u leaves the image; a
               constant image is invalid everywhere and finite; the smallest shapes run; one step beyond each range is refused;
               no host synchronisation.
5 USE          the disc pair through ``flow.optical_flow_since`` -> ``masks.flow_motion_labels`` -> ``ops.flow_l1``.

``PYTHONPATH=. python tests/test_optical_flow_gpu.py REPORT.jsonl`` turns the records of a run under FG_PARITY_REPORT into the
table of profiles/optical_flow_parity.md.
"""
import sys

import numpy as np
import pytest
import torch

import helpers
import optical_flow_restatement as R
import parity_common as P
from freegaussian_amd import _lib, flow, masks, ops
from parity_common import need_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)


def _host(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy()


# ---- 1 pyramid


@pytest.mark.parametrize("shape", R.PYRAMID_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", R.PYRAMID_KINDS)
def test_pyramid_every_level_by_regime(kind, shape):
    img = R.pyramid_input(kind, *shape)
    levels = ops.optical_flow_pyramid(_dev(img), R.PYRAMID_LEVELS)
    torch.cuda.synchronize()
    p64, p32, den = R.pyramid(img, R.PYRAMID_LEVELS, np.float64), R.pyramid(img, R.PYRAMID_LEVELS, np.float32), R.pyramid_den(img, R.PYRAMID_LEVELS)
    assert [tuple(x.shape) for x in levels] == R.level_shapes(*shape, R.PYRAMID_LEVELS)
    failures = []
    for l, (x, x64, x32, d) in enumerate(zip(levels, p64, p32, den)):
        assert x.dtype == torch.float32 and x.is_contiguous()
        regimes = R.border_masks(*x64.shape, 1)  # an output pixel within 1 of the edge has clamped taps (2 at the level above)
        e32 = P.yardstick(regimes, P.distance(x32, x64, d), R.FLOOR)
        P.check(f"pyramid|{kind}|{shape[0]}x{shape[1]}|L{l}|{{regime}}", regimes, P.distance(_host(x), x64, d), e32, R.F_PYRAMID, failures)
    assert not failures, "\n".join(failures)


# ---- 2 one update step


@pytest.mark.parametrize("shape", R.STEP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_update_step_by_regime(shape):
    a, b, init = R.step_inputs(*shape)
    u, valid = ops.optical_flow(_dev(a), _dev(b), levels=1, iters=1, consistency=None, init=_dev(init))
    torch.cuda.synchronize()
    u64, den, eig = R.one_step(*shape, "f64")
    u32, _, _ = R.one_step(*shape, "f32")
    regimes = R.step_masks(*shape, eig)
    e32 = P.yardstick(regimes, P.distance(u32, u64, den), R.FLOOR)
    failures = []
    P.check(f"step|{shape[0]}x{shape[1]}|{{regime}}", regimes, P.distance(_host(u), u64, den), e32, R.F_STEP, failures)
    assert not failures, "\n".join(failures)
    assert valid.dtype == torch.bool and tuple(valid.shape) == shape


# ---- 3 the whole call


def _call(case, H, W):
    a, b, truth = R.pair(case, H, W)
    u, valid = ops.optical_flow(_dev(a), _dev(b), levels=R.LEVELS)
    torch.cuda.synchronize()
    return _host(u), _host(valid), truth


@pytest.mark.parametrize("case,H,W", R.CALL_CASES, ids=lambda v: str(v))
def test_whole_call_against_the_restatement(case, H, W):
    u, valid, truth = _call(case, H, W)
    u64, v64, info = R.reference(case, H, W, "f64")
    u32, v32, _ = R.reference(case, H, W, "f32")
    inside = R.interior(H, W)
    both = valid & v64
    regimes = R.tercile_masks(info["eig"], both)
    e32 = P.yardstick(regimes, R.call_distance(u32, u64), R.FLOOR)
    failures = []
    P.check(f"call|{case}|{H}x{W}|{{regime}}", regimes, R.call_distance(u, u64), e32, R.F_CALL, failures)
    # validity: the yardstick is the restatement pair
    n = inside.sum()
    share, share32 = (inside & (valid != v64)).sum() / n, (inside & (v32 != v64)).sum() / n
    helpers._record(f"valid_share|{case}|{H}x{W}", share, 1)
    helpers._record(f"valid_share32|{case}|{H}x{W}", share32, 1)
    # the error against the analytic flow
    err = np.linalg.norm(u - truth, axis=-1)[inside & valid].mean()
    err64 = np.linalg.norm(u64 - truth, axis=-1)[inside & v64].mean()
    helpers._record(f"mean_err|{case}|{H}x{W}", err, 1)
    helpers._record(f"mean_err64|{case}|{H}x{W}", err64, 1)
    print(f"{case} {H}x{W}: validity differs on {share:.3%} of the interior (fp32 restatement {share32:.3%}); mean error {err:.5f} px "
          f"(float64 restatement {err64:.5f} px)")  # fmt: skip
    assert not failures, "\n".join(failures)
    assert share <= max(2 * share32, 1e-3), (share, share32)
    assert err <= 1.05 * err64 + 1e-3, (err, err64)


def test_validity_at_a_tight_threshold_depends_on_where_u_ba_is_sampled():
    """At the default threshold an affine pair cannot tell u_ba(x) from u_ba(x + u_ab) (tests/test_optical_flow_host.py, the
    mutant ``u_ba_at_x``); at this one the wrong sampling point changes 80 % of the map.  The same rule as above."""
    case, c = R.TIGHT_CASE, R.TIGHT_CONSISTENCY
    a, b, _ = R.pair(*case)
    _, valid = ops.optical_flow(_dev(a), _dev(b), levels=R.LEVELS, consistency=c)
    (u64, _, i64), (u32, _, i32) = R.reference(*case, "f64"), R.reference(*case, "f32")
    inside = R.interior(*case[1:])
    right = R.validity(u64, i64, c)
    share = (inside & (_host(valid) != right)).sum() / inside.sum()
    share32 = (inside & (R.validity(u32, i32, c) != right)).sum() / inside.sum()
    helpers._record(f"valid_share|tight|{case[1]}x{case[2]}", share, 1)
    print(f"consistency {c}: validity differs on {share:.3%} of the interior (fp32 restatement {share32:.3%})")
    assert share <= max(2 * share32, 1e-3), (share, share32)


# ---- 4 structure


def test_two_runs_and_both_call_shapes_give_the_same_bits():
    a, b, _ = R.pair("rotate_zoom", 97, 131)
    a, b = _dev(a), _dev(b)
    u1, v1 = ops.optical_flow(a, b, levels=R.LEVELS)
    u2, v2 = ops.optical_flow(a, b, levels=R.LEVELS)
    u3, v3 = ops.optical_flow(a, b, levels=R.LEVELS, consistency=None)
    assert torch.equal(u1, u2) and torch.equal(v1, v2)
    assert torch.equal(u1, u3)
    assert not bool((v1 & ~v3).any())  # the third test can only take pixels away
    assert all(torch.equal(x, y) for x, y in zip(ops.optical_flow_pyramid(a, 3), ops.optical_flow_pyramid(a, 3)))


def test_never_valid_where_the_target_leaves_the_image():
    for case in ("shift_large", "rotate_zoom"):
        H, W = 97, 131
        u, valid, _ = _call(case, H, W)
        y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
        px, py = x + u[..., 0], y + u[..., 1]
        outside = ~((px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1))
        assert outside.any() and not (valid & outside).any()


def test_a_constant_image_is_invalid_everywhere_and_finite():
    img = torch.full((40, 56), 0.37, device=DEV)
    u, valid = ops.optical_flow(img, img.clone())
    assert not bool(valid.any()) and bool(torch.isfinite(u).all())
    assert bool(torch.isnan(flow.optical_flow_since(img, img.clone())).all())


@pytest.mark.parametrize("H,W,levels", [(16, 16, 1), (16, 16, 2), (16, 40, 2), (33, 16, 2)])
def test_the_smallest_shapes_run(H, W, levels):
    a, b, truth = R.affine_pair(H, W, "shift_small", seed=5)
    u, valid = ops.optical_flow(_dev(a), _dev(b), levels=levels, radius=7, iters=16)
    u64, v64 = R.optical_flow(a, b, levels=levels, radius=7, iters=16)
    torch.cuda.synchronize()
    assert tuple(u.shape) == (H, W, 2) and tuple(valid.shape) == (H, W)
    both = _host(valid) & v64
    assert np.isfinite(_host(u)[_host(valid)]).all()
    # (parity is tests 1-3's; this one is about running at all: the median is blind to a pixel that rounding tips elsewhere)
    assert not both.any() or np.median(np.abs(_host(u) - u64)[both]) < 1e-2


def test_one_step_beyond_each_range_is_refused_without_a_launch():
    lib = _lib.load()
    img = torch.zeros(16, 16, device=DEV)
    ok = dict(levels=1, iters=1, radius=1)
    ops.optical_flow(img, img.clone(), **ok)
    for bad in (dict(levels=0), dict(levels=9), dict(levels=3), dict(iters=0), dict(iters=17), dict(radius=0), dict(radius=8),
                dict(min_eig=-1.0), dict(min_eig=float("nan")), dict(consistency=-1.0), dict(consistency=float("inf"))):  # fmt: skip
        with pytest.raises(ValueError):
            ops.optical_flow(img, img.clone(), **{**ok, **bad})
    for shape in ((15, 16), (16, 15), (16385, 16), (16, 16, 4), (16, 16, 2)):
        with pytest.raises(ValueError):
            ops.optical_flow(torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV))
    with pytest.raises(ValueError):
        ops.optical_flow(torch.zeros(16, 16, dtype=torch.uint8, device=DEV), torch.zeros(16, 16, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.optical_flow_pyramid(img, 3)
    # the library itself, with the addresses of real tensors: refused before any launch
    u, v, ws = torch.zeros(16, 16, 2, device=DEV), torch.zeros(16, 16, dtype=torch.uint8, device=DEV), torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    other = img.clone()

    def raw(H=16, W=16, levels=1, iters=1, radius=1):
        return lib.fg_optflow(H, W, 1, _lib.TARGET_F32, img.data_ptr(), other.data_ptr(), levels, iters, radius, 1e-5, 0, 0.0, None,
                              u.data_ptr(), v.data_ptr(), ws.data_ptr(), ws.numel(), None)  # fmt: skip

    for kw in (dict(H=15), dict(W=15), dict(H=16385), dict(W=16385), dict(levels=9), dict(levels=3), dict(radius=8), dict(iters=17)):
        assert raw(**kw) == -4, kw
    for kw in (dict(levels=0), dict(radius=0), dict(iters=0)):
        assert raw(**kw) == -1, kw
    torch.cuda.synchronize()
    assert not bool(u.any()) and not bool(v.any())


def test_the_call_does_not_synchronise():
    a, b, _ = R.pair("shift_small", 97, 131)
    a, b = _dev(a), _dev(b)
    ops.optical_flow(a, b)  # (the library is loaded, the allocator warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        u, valid = ops.optical_flow(a, b)
        since = flow.optical_flow_since(a, b)
        levels = ops.optical_flow_pyramid(a, 3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(valid.any()) and since.shape == u.shape and len(levels) == 3


# ---- 5 use


def test_the_disc_pair_through_the_consumers():
    a, b, truth, inside, outside = R.disc_pair()
    m = R.interior(*R.DISC_SHAPE)
    # the disc's motion on the CURRENT frame's grid: `since` sees the disc where it is in b
    H, W = R.DISC_SHAPE
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d1 = np.hypot(x - R.DISC_CENTRE[0] - R.DISC_SHIFT[0], y - R.DISC_CENTRE[1] - R.DISC_SHIFT[1])
    inside_now = d1 <= R.DISC_RADIUS - 8
    flows = flow.optical_flow_since(_dev(a), _dev(b))
    labels, valids = masks.flow_motion_labels(flows, threshold=1.0)
    moving = _host(labels[..., 0])
    assert moving[inside_now].all()
    assert not moving[outside & m].any()
    f = _host(flows)
    assert np.abs(f[inside_now] - np.array(R.DISC_SHIFT)).max() < 0.05
    assert np.isnan(f).any() and bool(valids.all())  # the occluded rim carries the "no measurement" mark
    loss = ops.flow_l1(torch.zeros(H, W, 2, device=DEV), flows)
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    fwd = _host(flow.optical_flow_forward(_dev(a), _dev(b)))
    assert np.abs(fwd[inside] - np.array(R.DISC_SHIFT)).max() < 0.05


# ---- the table of profiles/optical_flow_parity.md


def _report(path: str) -> None:
    ratio, e32 = P.read_records(path, "test_optical_flow_gpu.py")
    for test, F in (("pyramid", R.F_PYRAMID), ("step", R.F_STEP), ("call", R.F_CALL)):
        rows = {k: v for k, v in ratio.items() if k[0] == test}
        worst = max(rows.values(), default=0.0)
        print(f"\n{test}: worst ratio {worst:.3g}, F = {F}\n| cell | regime | E32 | ratio |\n|---|---|---|---|")
        for k in sorted(rows):
            print(f"| {' '.join(k[1:-1])} | {k[-1]} | {e32[k]:.3g} | {rows[k]:.3g} |")


if __name__ == "__main__":
    _report(sys.argv[1])
