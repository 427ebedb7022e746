"""The image loss's restatement (tests/loss_restatement.py) and its regime image, checked on the CPU: the float64 restatement
is autograd through ``harness.ssim`` in float64, the fp32 one is ``harness.ssim`` in fp32 to within the fp32 yardstick, every
regime is what it is named for, the sign ties are exact, and the per-element bound the GPU test applies (F x the fp32
restatement's own distance from float64, per regime and cotangent group, relative to the element's absolute accumulation)
catches each wrong restatement.  tests/parity_common.py has the protocol.

``harness.ssim`` builds its 11 x 11 window in fp32 (exp, sum and outer product rounded to float); the kernel holds the taps
normalised in double and rounded once.  The two windows differ by an fp32 ulp per tap, 1e-7 of the gradient: the comparison
with ``harness.ssim`` hands the restatement the harness's window, everything else here uses the kernel's."""
import functools

import pytest
import torch

import loss_restatement as L
import parity_common as P
from freegaussian_amd import harness

H0, W0 = L.SHAPES[0]


@functools.lru_cache(maxsize=None)
def _image(H=H0, W=W0, first=0):
    return L.regime_image(H, W, first)


@functools.lru_cache(maxsize=None)
def _grads(dtype, mutant=None, C=3, harness_window=False):
    pred, gt, _ = _image()
    w2d = harness._gauss_window() if harness_window else None
    return L.gradients(pred[..., :C].contiguous(), gt[..., :C].contiguous(), dtype, mutant, w2d=w2d)


def _harness(dtype, C, group):
    pred, gt, _ = _image()
    x = pred[..., :C].to(dtype).requires_grad_(True)
    y = gt[..., :C].to(dtype)
    v_l1, v_ssim = L.COTANGENTS[group]
    l1 = (y - x).abs().mean()
    ss = harness.ssim(y.permute(2, 0, 1)[None], x.permute(2, 0, 1)[None])
    (v_l1 * l1 + v_ssim * ss).backward()
    return l1.detach(), ss.detach(), x.grad


@pytest.mark.parametrize("C", [1, 3, 4])
def test_float64_restatement_is_autograd_through_the_torch_statement(C):
    fwd, res = _grads(torch.float64, None, C, True)
    for group in L.GROUPS:
        l1, ss, g = _harness(torch.float64, C, group)
        assert abs(float(fwd["l1"]) - float(l1)) <= 1e-12 * float(l1) and abs(float(fwd["ssim"]) - float(ss)) <= 1e-12
        d = P.distance(res[group][0], g, res[group][1])
        assert float(d.max()) <= 1e-12, (group, float(d.max()))


@pytest.mark.parametrize("C", [1, 3, 4])
def test_fp32_restatement_is_the_torch_statement_in_fp32(C):
    """Two plain fp32 statements of one formula (the sums of the windows in another order): the torch statement lies within
    4 x the restatement's own floored yardstick of float64, per regime, relative to A."""
    masks = P.masks_of_index(_image()[2], L.REGIMES)
    _, r64 = _grads(torch.float64, None, C, True)
    _, r32 = _grads(torch.float32, None, C, True)
    for group in L.GROUPS:
        e32 = P.yardstick(masks, P.distance(r32[group][0], *r64[group]), L.FLOOR)
        d = P.distance(_harness(torch.float32, C, group)[2], *r64[group])
        for name, (ratio, at) in P.worst_ratios(masks, d, e32).items():
            print(f"C={C} {group} {name}: harness fp32 at {ratio:.2f} x E32 ({e32[name]:.2e})")
            assert ratio <= 4.0, (group, name, ratio, at)


def test_census_every_regime_is_what_it_is_named_for():
    pred, gt, regime = _image()
    ys, xs = L.block_grid(H0, W0)
    assert len(ys) == 3 and len(xs) == 5 and min(b - a for a, b in zip(ys, ys[1:])) >= L.BLOCK
    assert min(b - a for a, b in zip(xs, xs[1:])) >= L.BLOCK
    assert set(regime.unique().tolist()) == set(range(len(L.REGIMES)))
    assert float(pred.min()) >= 0 and float(pred.max()) <= 1.001 and float(gt.min()) >= 0 and float(gt.max()) <= 1
    fwd = L.forward(pred, gt, torch.float64)
    mreg = L.map_regime(regime)
    px = lambda name: regime == L.REGIMES.index(name)  # noqa: E731
    # whole windows inside one block: there the moments are the block's own
    inside = torch.zeros_like(mreg, dtype=torch.bool)
    for i in range(len(ys) - 1):
        for j in range(len(xs) - 1):
            inside[ys[i] : ys[i + 1] - L.HALO, xs[j] : xs[j + 1] - L.HALO] = True
    for name in L.REGIMES:
        assert int((inside & (mreg == L.REGIMES.index(name))).sum()) >= 11 * 11, name
    var = lambda name, k: fwd["moments"][k][:, inside & (mreg == L.REGIMES.index(name))]  # noqa: E731
    for name in ("white_equal", "black_equal", "flat_offset"):  # flat: the windowed variances are far below C2
        assert float(var(name, "s1").abs().max()) < 1e-3 * L.C2 and float(var(name, "s2").abs().max()) < 1e-3 * L.C2, name
    assert bool((pred[px("white_equal")] == 1).all()) and bool((gt[px("white_equal")] == 1).all())
    assert bool((pred[px("black_equal")] == 0).all()) and bool((gt[px("black_equal")] == 0).all())
    off = (pred - gt)[px("flat_offset")]
    assert bool((off > 0.9e-3).all()) and bool((off < 1.1e-3).all())
    assert float(var("textured", "s1").min()) > 10 * L.C2 and float(var("clamped_ties", "s2").min()) > 10 * L.C2
    assert float(var("ramp", "s2").max()) < 0.02 and float(var("ramp", "s2").min()) > 1e-5  # smooth, not flat
    step = px("step")
    assert 0 < int((pred != gt)[step].sum()) <= 4 * (ys[1] - ys[0])  # one column of every channel differs
    assert float(var("step", "s2").max()) > 0.05 and float(var("step", "s2").min()) < 1e-3 * L.C2  # the edge, and flat beside it
    ties = px("clamped_ties")
    tied = (pred == gt)[ties]
    assert 0.6 < float(tied.float().mean()) < 0.9
    assert bool(((gt[ties] == 0) | (gt[ties] == 1)).all()) and bool((gt[ties][tied] == 0).any()) and bool((gt[ties][tied] == 1).any())
    # the white-equal block: the gradient is far below its accumulation (what the element distance is there for)
    _, r64 = _grads(torch.float64)
    g, a = r64["ssim"]
    own = torch.zeros_like(regime, dtype=torch.bool)  # pixels whose whole support (every window that holds them) is their block's
    for i in range(len(ys) - 1):
        for j in range(len(xs) - 1):
            own[ys[i] + L.HALO : ys[i + 1] - L.HALO, xs[j] + L.HALO : xs[j + 1] - L.HALO] = True
    w = px("white_equal") & own
    assert int(w.sum()) >= 6 * 6 and bool((g[w].abs() < 1e-3 * a[w]).all())


def test_sign_ties_are_exact():
    """No decision depends on rounding: sign(pred - gt) is the same in fp32 and float64 on every element, and the ties are
    exact zeros of fp32 inputs."""
    for (H, W), first in zip(L.SHAPES, (0, 1, 0, 5)):
        pred, gt, _ = _image(H, W, first)
        assert torch.equal(torch.sign(pred - gt).double(), torch.sign(pred.double() - gt.double()))
    pred, gt, _ = _image()
    assert int((pred == gt).sum()) > 3 * 4 * 29 * 26 // 2


def test_yardsticks_are_floored_and_finite():
    regime = _image()[2]
    masks, map_masks = P.masks_of_index(regime, L.REGIMES), P.masks_of_index(L.map_regime(regime), L.REGIMES)
    for C in (1, 3, 4):
        f32, r32 = _grads(torch.float32, None, C)
        f64, r64 = _grads(torch.float64, None, C)
        for group in L.GROUPS:
            assert bool(torch.isfinite(r64[group][0]).all()) and bool((r64[group][1] >= 0).all())
            e32 = P.yardstick(masks, P.distance(r32[group][0], *r64[group]), L.FLOOR)
            assert set(e32) == set(L.REGIMES)
            for name, e in e32.items():
                assert L.FLOOR <= e < 1e-2, (C, group, name, e)
        for k in L.MAPS:
            e32 = P.yardstick(map_masks, P.distance(f32["maps"][k], f64["maps"][k], f64["acc"][k]), L.FLOOR)
            for name, e in e32.items():
                assert L.FLOOR <= e < 1e-2, (C, k, name, e)


LIVE = ("textured", "ramp", "step", "clamped_ties")  # (on the flat blocks the SSIM gradient vanishes whatever the window)
TIES = ("white_equal", "black_equal", "clamped_ties")
SSIM_GROUPS = ("ssim", "both")
# (mutant, cotangent groups that drive it, regimes it concerns, further condition on the element)
MUTANT_CASES = [
    ("sigma_1p4", SSIM_GROUPS, LIVE, None),
    ("window_not_normalised", SSIM_GROUPS, LIVE, None),
    ("c2_not_squared", SSIM_GROUPS, LIVE, None),
    ("d_mu_without_variance_paths", SSIM_GROUPS, LIVE, None),
    ("full_conv_shifted", SSIM_GROUPS, LIVE, None),
    ("last_map_column_dropped", SSIM_GROUPS, ("textured",), "last_columns"),
    ("sign_of_zero_is_one", ("l1", "both"), TIES, "tied"),
    ("ssim_mean_over_hwc", SSIM_GROUPS, LIVE, None),
]


def mutant_cells(factor):
    """-> {(mutant, group, regime): (caught, elements, cap)}: an element of the mutant's float64 gradient is CAUGHT when the
    GPU test would flag it: at least 4 * factor * E32 of its accumulation from the true one.  ``cap``: the largest F at
    which three quarters of the concerned elements are still caught."""
    pred, gt, regime = _image()
    _, r32 = _grads(torch.float32)
    _, r64 = _grads(torch.float64)
    cond = dict(last_columns=(torch.arange(W0) >= W0 - L.WIN)[None, :, None].expand(H0, W0, 3),
                tied=(pred == gt)[..., :3])  # fmt: skip
    edge = int(((pred != gt).any(-1) & (regime == L.REGIMES.index("step"))).any(0).nonzero().min())
    cond["near_edge"] = ((torch.arange(W0) - edge).abs() <= 2)[None, :, None].expand(H0, W0, 3)
    out = {}
    for mutant, groups, regimes, extra in MUTANT_CASES:
        _, rm = _grads(torch.float64, mutant)
        for group in groups:
            e32 = P.yardstick(P.masks_of_index(regime, L.REGIMES), P.distance(r32[group][0], *r64[group]), L.FLOOR)
            d = P.distance(rm[group][0], *r64[group])
            for name in regimes:
                sel = (regime == L.REGIMES.index(name))[..., None].expand_as(d)
                if extra:
                    sel = sel & cond[extra]
                if name == "step":  # (two columns either side of the edge: further out the block is flat)
                    sel = sel & cond["near_edge"]
                ratios = d[sel] / e32[name]
                out[(mutant, group, name)] = (int((ratios >= 4 * factor).sum()), ratios.numel(), P.three_quarter_cap(ratios))
    return out


def test_every_mutant_is_listed():
    assert {c[0] for c in MUTANT_CASES} == set(L.MUTANTS)


def test_mutants_are_caught_by_the_element_bound():
    """On at least three quarters of the elements a mutant concerns, in each cotangent group that drives it, the mutant's
    float64 gradient is at least 4 * F * E32 of the element's accumulation from the true one (cancellation may hide it on
    single elements): the GPU bound F * E32 has teeth, and this caps F.  That is looser than "on the elements it concerns":
    three quarters of them, as in tests/test_raster_rows_host.py; of the ``step`` block only the two columns either side of its
    edge count, and the flat blocks count for the sign mutant alone (there the SSIM gradient vanishes whatever the window).
    The two mutants of the SSIM mean, the wrong C2 and the window that is not normalised move the scalar as well."""
    factor = 1.0 if L.F is None else L.F
    cells = mutant_cells(factor)
    for (mutant, group, name), (caught, n, cap) in cells.items():
        print(f"{mutant} {group} {name}: {caught}/{n} elements caught at F = {factor:g}; caps F at {cap:.1f}")
    cap = min(v[2] for v in cells.values())
    print(f"the cap on F: {cap:.1f}")
    failures = [f"{k}: {v[0]}/{v[1]}" for k, v in cells.items() if v[1] == 0 or 4 * v[0] < 3 * v[1]]
    assert not failures, "\n".join(failures)
    assert L.F is None or L.F <= cap
    pred, gt, _ = _image()
    f32, f64 = L.forward(pred[..., :3], gt[..., :3], torch.float32), L.forward(pred[..., :3], gt[..., :3], torch.float64)
    e32 = max(float(P.distance(f32["ssim"], f64["ssim"], f64["ssim_acc"])), L.FLOOR)
    for mutant in ("last_map_column_dropped", "ssim_mean_over_hwc", "c2_not_squared", "window_not_normalised"):
        fm = L.forward(pred[..., :3], gt[..., :3], torch.float64, mutant)
        ratio = float(P.distance(fm["ssim"], f64["ssim"], f64["ssim_acc"])) / e32
        print(f"{mutant}: the SSIM value is {ratio:.1f} x E32 ({e32:.2e}) away")
        assert ratio >= 4 * factor, (mutant, ratio)
    # where the true gradient is exactly zero (tied pixels, l1 group) the sign mutant's is not
    _, r64 = _grads(torch.float64)
    _, rm = _grads(torch.float64, "sign_of_zero_is_one")
    tied = (pred == gt)[..., :3]
    assert bool((r64["l1"][0][tied] == 0).all()) and bool((rm["l1"][0][tied] != 0).all())
