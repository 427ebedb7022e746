"""The per-Gaussian stage's restatement (tests/per_gaussian_restatement.py) and the regime scene, checked on the CPU: the
restatement is the pinned oracle's projection, every regime is what it is named for, no row sits near a branch boundary,
and the row-wise bound the GPU test applies (F x the fp32 restatement's own row distance from float64, per regime, cotangent
group and input tensor; tests/parity_common.py has the protocol) is tight enough to catch each autograd-level mutant of the
restatement."""
import functools

import pytest
import torch

import parity_common as P
import per_gaussian_restatement as R
from oracle import raster_oracle as O

SEED = 0
VISIBLE = R.VISIBLE_REGIMES


@functools.lru_cache(maxsize=None)
def _scene():
    return R.regime_scene(SEED)


@functools.lru_cache(maxsize=None)
def _grads(path_name, dtype, mutant=None):
    return R.gradients(_scene(), R.PATHS[path_name], dtype, mutant=mutant)


def test_path_table_has_every_value_at_least_twice():
    cols = dict(form=R.FORMS, sh_degree=(-1, 0, 1, 3), antialiased=(False, True), with_depth=(False, True), n_extra=(0, 2),
                note=(False, True))  # fmt: skip
    for col, values in cols.items():
        for v in values:
            assert sum(p[col] == v for p in R.PATHS.values()) >= 2, (col, v)
    sh = [p for p in R.PATHS.values() if p["sh_degree"] >= 0]
    assert sum(p["k_stored"] == (p["sh_degree"] + 1) ** 2 for p in sh) >= 2 and sum(p["k_stored"] == 16 for p in sh) >= 2
    for p in R.PATHS.values():
        assert 3 + p["with_depth"] + p["n_extra"] <= 8


def test_restatement_is_the_pinned_oracles_projection():
    """fp32: radii, means2d, depths, conics of the restatement equal ``O.rasterization``'s info on the regime scene, bit for
    bit (classic and antialiased; the record's opacity slot is the oracle's ``info["opacities"]``)."""
    sc = _scene()
    for aa in (False, True):
        inp = sc.inputs("plain", 3, 16, 0)
        outs = R.stage(inp, sc.viewmat, sc.K, form="plain", sh_degree=3, antialiased=aa)
        _, _, info = O.rasterization(inp["means"], inp["quats"], inp["scales"], inp["opacities"], inp["colors"], sc.viewmat[None],
                                     sc.K[None], sc.width, sc.height, sh_degree=3, packed=False,
                                     rasterize_mode="antialiased" if aa else "classic")  # fmt: skip
        for k in ("radii", "means2d", "depths", "conics"):
            assert torch.equal(outs[k], info[k][0]), k
        vis = outs["radii"] > 0
        assert torch.equal(outs["record"][:, 2][vis], info["opacities"][0][vis])
        assert torch.equal(outs["record"][:, :2], outs["means2d"]) and torch.equal(outs["record"][:, 3:6], outs["conics"])
        assert bool((outs["record"][:, 9:] == 0).all()) and bool((outs["record"][~vis] == 0).all())


def test_census_every_regime_is_what_it_is_named_for():
    sc = _scene()
    W, H = sc.width, sc.height
    limx, limy = O.FOV_CLAMP * 0.5 * W / float(sc.K[0, 0]), O.FOV_CLAMP * 0.5 * H / float(sc.K[1, 1])
    assert sc.viewmat[:3, :3].abs().min() > 0.05  # not axis-aligned
    assert sc.K[0, 0] != sc.K[1, 1] and sc.K[0, 2] != 0.5 * W and sc.K[1, 2] != 0.5 * H
    for name, n in R.COUNTS.items():
        assert len(sc.rows(name)) == n >= 8
    first = sc.labels[:64]  # regimes interleave within a workgroup
    assert len(set(first)) == len(R.COUNTS)
    for path_name in ("plain-sh3-aa-rows", "raw-sh3-aa-depth-extra", "delta-sh1-k16-aa-extra"):
        o32, _ = _grads(path_name, torch.float32)
        o64, _ = _grads(path_name, torch.float64)
        assert torch.equal(o32["radii"], o64["radii"]), path_name
        form = R.PATHS[path_name]["form"]
        inp = sc.inputs(form, 3, 16, 0, torch.float64)
        pc = inp["means"] @ sc.viewmat.double()[:3, :3].T + sc.viewmat.double()[:3, 3]
        ax, ay = (pc[:, 0] / pc[:, 2]).abs() / limx, (pc[:, 1] / pc[:, 2]).abs() / limy
        radii, comp = o64["radii"], o64["compensations"]
        for name in R.COUNTS:
            rows = sc.rows(name)
            assert bool((radii[rows] > 0).all() if name not in R.CULLED else (radii[rows] == 0).all()), (path_name, name)
            x, y = ax[rows], ay[rows]
            if name in ("clamp_x", "clamp_xy"):
                assert bool(((x > 1.05) & (x < 1.6)).all())
            if name in ("clamp_y", "clamp_xy"):
                assert bool(((y > 1.05) & (y < 1.6)).all())
            if name == "clamp_x":
                assert bool((y < 0.9).all())
            if name == "clamp_y":
                assert bool((x < 0.9).all())
            if name == "near_limit":
                m = torch.maximum(x, y)
                assert bool(((m >= 0.9) & (m <= 0.999)).all())
            if name in ("ordinary", "subpixel", "sh_clamped", "saturated"):
                assert bool(((x < 0.9) & (y < 0.9)).all())
            if name == "subpixel":
                assert bool(((comp[rows] > 1e-4) & (comp[rows] < 1e-2)).all()) and bool((radii[rows] == 2).all())
            if name == "behind":
                assert bool((pc[rows, 2] < 0).all())
            if name == "offscreen":
                assert bool((pc[rows, 2] > R.NEAR).all())
        qn = sc.raw["quats"].norm(dim=1)
        assert bool(((qn > 0.2) & (qn < 5.0)).all()) and float(qn.min()) < 0.5 and float(qn.max()) > 2.0
        sat = sc.rows("saturated")
        assert bool((sc.raw["opacity_logits"][sat].abs() == 12).all())
        assert len(set(torch.sign(sc.raw["opacity_logits"][sat]).tolist())) == 2
        assert bool((sc.raw["d_scales"][sat] > 0).any()) and bool((sc.raw["d_scales"][sat] < 0).any())
    # sh_clamped: one, two or three channels below -0.5 (before the offset), at every degree of the path table
    inp = sc.inputs("plain", 3, 16, 0, torch.float64)
    campos = torch.linalg.inv(sc.viewmat.double())[:3, 3]
    for deg in R.SH_DEGREES:
        below = (O.sh_eval(deg, inp["means"] - campos[None, :], inp["colors"]) < -0.5).sum(dim=1)
        assert sorted(set(below[sc.rows("sh_clamped")].tolist())) == [1, 2, 3]
        assert bool((below[sc.rows(*[k for k in R.COUNTS if k != "sh_clamped"])] == 0).all())


@pytest.mark.parametrize("form", R.FORMS)
def test_no_row_is_near_a_branch_boundary(form):
    """What lets the GPU test compare EVERY row: no decision of the stage is within 1e-3 of flipping."""
    m = R.margins(_scene(), form)
    for name, v in m.items():
        assert not bool(torch.isnan(v).any()), name
        assert float(v.min()) >= R.MARGIN, (form, name, float(v.min()), int(v.argmin()))
    assert bool(torch.isfinite(m["cull"][_scene().rows(*R.CULLED)]).all())


def _row_e32(x32, x64):
    return P.yardstick(P.live_row_masks(_scene().labels, x64), P.distance(x32, x64, x64.abs(), rows=True), R.FLOOR)


def test_yardstick_is_floored_and_finite():
    for path_name in R.PATHS:
        _, g32 = _grads(path_name, torch.float32)
        _, g64 = _grads(path_name, torch.float64)
        for group in g64:
            for tensor in g64[group]:
                for regime, e in _row_e32(g32[group][tensor], g64[group][tensor]).items():
                    assert R.FLOOR <= e < 1e-2, (path_name, group, tensor, regime, e)


def test_exact_zero_rows_stay_exactly_zero_in_fp32():
    """Rows whose float64 gradient is exactly zero (culled rows; quats / scales under means2d-only cotangents; ...) are
    exactly zero in the fp32 restatement too -- and some exist in every group."""
    sc = _scene()
    culled = sc.rows(*R.CULLED)
    for path_name in R.PATHS:
        _, g32 = _grads(path_name, torch.float32)
        _, g64 = _grads(path_name, torch.float64)
        for group in g64:
            for tensor in g64[group]:
                z = P.zero_rows(g64[group][tensor])
                if not (tensor == "extra" and group in ("extra", "all")):  # (a record slot's pass-through gradient)
                    assert bool(z[culled].all()), (path_name, group, tensor)
                assert bool((g32[group][tensor][z] == 0).all()), (path_name, group, tensor)
        for tensor in ("quats", "scales" if R.PATHS[path_name]["form"] == "plain" else "log_scales"):
            assert bool(P.zero_rows(g64["means2d"][tensor]).all())
            assert not bool(P.zero_rows(g64["conics_out"][tensor]).all())


# (mutant, path, cotangent groups that drive it, input tensors it reaches, regimes it concerns)
MUTANT_CASES = [
    ("clamp_derivative", "plain-sh3-aa-rows", ("conics_out", "conics_rec", "opacity"), ("means",),
     ("clamp_x", "clamp_y", "clamp_xy")),
    ("clamp_derivative", "raw-sh1-k4-rows", ("conics_out",), ("means",), ("clamp_x", "clamp_y", "clamp_xy")),
    ("compensation", "plain-sh3-aa-rows", ("opacity",), ("means", "quats", "scales"), VISIBLE),
    ("quat_projection", "plain-direct", ("conics_out", "conics_rec"), ("quats",), VISIBLE),
    ("quat_projection", "delta-sh3-depth-rows", ("conics_out",), ("quats", "d_quats"), VISIBLE),
    # the outer q/|q| of the raw form matters through the delta only (without one, the projection's own normalisation
    # already projects); on sub-pixel rows the blur is the whole conic and the rotation's gradient, a second-order matter
    # of the delta here, drowns: every other regime
    ("raw_quat_projection", "delta-sh3-depth-rows", ("conics_out",), ("quats",), tuple(k for k in VISIBLE if k != "subpixel")),
    ("sh_mask", "plain-sh3-depth-extra", ("colour",), ("colors", "means"), ("sh_clamped",)),
    ("sh_mask", "plain-sh0-k1-depth", ("colour",), ("colors",), ("sh_clamped",)),
    ("view_dir_projection", "plain-sh3-depth-extra", ("colour",), ("means",), VISIBLE),
    ("view_dir_projection", "plain-sh1-k4-aa-depth", ("colour",), ("means",), VISIBLE),
    ("depth_channel", "plain-sh3-depth-extra", ("depth_channel",), ("means",), VISIBLE),
]  # fmt: skip


def test_every_mutant_is_listed():
    assert {c[0] for c in MUTANT_CASES} == set(R.MUTANTS)


@pytest.mark.parametrize("mutant,path_name,groups,tensors,regimes", MUTANT_CASES, ids=[f"{c[0]}-{c[1]}" for c in MUTANT_CASES])
def test_mutants_are_caught_by_the_row_bound(mutant, path_name, groups, tensors, regimes):
    """On the rows of the regimes a mutant concerns, in the cotangent groups that drive it, EVERY row of the mutant's
    float64 gradient is at least 4 * F * E32 from the true one (or non-zero where the true one is exactly zero): the GPU
    bound F * E32 has teeth (and this caps F).  The mutant's forward is the restatement's."""
    sc = _scene()
    factor = 1.0 if R.F is None else R.F
    o64, g64 = _grads(path_name, torch.float64)
    _, g32 = _grads(path_name, torch.float32)
    om, gm = _grads(path_name, torch.float64, mutant)
    for k in o64:
        assert torch.equal(o64[k], om[k]), k
    for group in groups:
        for tensor in tensors:
            e32 = _row_e32(g32[group][tensor], g64[group][tensor])
            d = P.distance(gm[group][tensor], g64[group][tensor], g64[group][tensor].abs(), rows=True)
            for regime in regimes:
                rows = sc.rows(regime)
                # a row whose true gradient is exactly zero (all three channels clamped: no colour gradient at all) falls
                # to the exact-zero rule if the mutant's is not zero; if it is zero too the mutant does not reach the row
                zero = P.zero_rows(g64[group][tensor])[rows]
                assert int(zero.sum()) * 2 < len(rows), (group, tensor, regime)
                if mutant == "sh_mask":
                    assert not bool(P.zero_rows(gm[group][tensor])[rows][zero].any())
                dr = d[rows][~zero]
                assert bool(torch.isfinite(dr).all())
                print(f"{mutant} {path_name} {group} {tensor} {regime}: min row distance {float(dr.min()):.3e}, "
                      f"E32 {e32[regime]:.3e}, ratio {float(dr.min()) / e32[regime]:.0f} (needs {4 * factor:.0f})")  # fmt: skip
                assert float(dr.min()) >= 4 * factor * e32[regime], (group, tensor, regime)


def test_clamp_mutant_is_invisible_to_pooled_cotangents_and_touches_no_other_row():
    """Why the groups are driven one at a time: with cotangents on all outputs the means2d path dominates a clamped row's
    gradient and the clamp mutant's MEDIAN row error falls under what the conics group alone shows by a factor of 100;
    rows of the other regimes are not touched at all."""
    sc = _scene()
    _, g64 = _grads("plain-sh3-aa-rows", torch.float64)
    _, gm = _grads("plain-sh3-aa-rows", torch.float64, "clamp_derivative")
    clamped = sc.rows("clamp_x", "clamp_y", "clamp_xy")
    others = sc.rows(*[k for k in R.VISIBLE_REGIMES if not k.startswith("clamp")])
    d_all = P.distance(gm["all"]["means"], g64["all"]["means"], g64["all"]["means"].abs(), rows=True)
    d_con = P.distance(gm["conics_out"]["means"], g64["conics_out"]["means"], g64["conics_out"]["means"].abs(), rows=True)
    assert float(d_con[others].max()) == 0.0 and float(d_all[others].max()) == 0.0
    assert float(d_all[clamped].median()) * 100 < float(d_con[clamped].median())
