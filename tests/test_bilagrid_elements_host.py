"""The per-element restatement of the bilateral-grid slice (tests/bilagrid_restatement.py: restate, regime_case) checked on the
CPU: the float64 restatement is torch's float64 autograd of ``bilagrid.apply_to_render`` element by element at the scale of
each element's accumulation; every shape of the GPU test holds what its line there says (asserted from the integer maps
restated in Python, and from the library's workspace query, which answers without a GPU); the integer maps partition
every axis and the floor of the fp32 quotient is the integer cell at every cell boundary of every supported size; every
regime has elements; and the bound the GPU test applies (tests/parity_common.py has the protocol) catches each wrong
restatement."""
import functools

import numpy as np
import pytest
import torch

import bilagrid_restatement as R
import parity_common as P
from freegaussian_amd import _lib, bilagrid
from freegaussian_amd.bilagrid import BilateralGrid

IDS = ["%dx%d-%d-%d-%d-%s" % (s[0], s[1], s[2], s[3], s[4], s[7]) for s in R.SHAPES]
BY_SIZE = {s[:2]: s for s in R.SHAPES}

# float64 restatement against torch's float64 autograd, per element at the scale of A.  Torch forms the level coordinate
# through [-1, 1] (luma * 2 - 1, then (z + 1) / 2 * (GL-1)): a few roundings of a coordinate of up to 15, 4 * 15 * 2^-52 =
# 1.3e-14, against a weight that is as small as 1e-3 on the pixels placed near a node: 1.3e-11 of such an element's
# accumulation.  Measured over the ten shapes: at most 2.1e-12 (v_grid of 5 x 300 with 16 levels; at most 4e-15 where GL <= 3);
# bound 2e-11.  (The 3e-7 of the helper's docstring is apply_to_render's fp32 ``linspace``: here the default dtype is float64
# while it runs.  The luma weights are the same fp32 values on both sides.)
TORCH_BOUND = 2e-11


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_float64_restatement_is_torch_autograd_per_element(monkeypatch, shape):
    monkeypatch.delenv("FG_FUSED_BILAGRID", raising=False)
    H, W, GX, GY, GL, num, cam, _ = shape
    c = R.regime_case(*shape)
    m = BilateralGrid(num=num, grid_X=GX, grid_Y=GY, grid_W=GL)
    with torch.no_grad():
        m.grids.copy_(torch.from_numpy(np.array(c["grids"])))
    m = m.double()  # (the luma weights: the fp32 values as doubles, as in the restatement)
    rgb = torch.from_numpy(np.array(c["rgb"])).double().requires_grad_(True)
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # apply_to_render's pixel grid is a linspace in the default dtype
    try:
        out = bilagrid.apply_to_render(m, rgb.unsqueeze(0), cam, H, W).squeeze(0)
    finally:
        torch.set_default_dtype(before)
    (out * torch.from_numpy(np.array(c["v_out"])).double()).sum().backward()
    got = {"out": out.detach().numpy(), "v_rgb": rgb.grad.numpy(), "v_grid": m.grids.grad[cam].numpy()}
    r64 = c["r64"]
    for name in R.ARRAYS:
        acc = r64[name + "_acc"]
        # a node that only a pixel ON a node could reach: torch may hold the pixel a rounding below the node and give the
        # next node a weight of 1e-16; the restatement's weight there is exactly 0 (A = 0): compare those at the scale of u
        reached = acc > 0
        d = P.distance(got[name][reached], r64[name][reached], acc[reached])
        print(f"{c['tag']} {name}: float64 restatement against torch, worst element {d.max():.2e} of its accumulation")
        assert float(d.max()) <= TORCH_BOUND, (name, float(d.max()))
        assert float(np.abs(got[name][~reached]).max(initial=0.0)) <= TORCH_BOUND * float(np.abs(c["v_out"]).max() * W * H)
        assert bool((r64[name][~reached] == 0).all())
    for i in range(num):
        assert i == cam or not bool(m.grids.grad[i].any())


def test_census_every_shape_holds_what_the_gpu_test_says():
    lib = _lib.load()
    seg = {s[:2]: R.segments(s[1], s[2]) for s in R.SHAPES}
    lay = {s[:2]: R.gather_layout(s[0], s[1], s[2], s[3]) for s in R.SHAPES}
    for s in R.SHAPES:  # the chunk count, against the library's workspace query
        H, W, GX, GY, GL = s[:5]
        chunks = -(-int(lay[s[:2]]["npx"].max()) // R.CHUNK)
        assert int(lay[s[:2]]["chunk"].max()) + 1 == chunks
        assert lib.fg_bilagrid_bwd_workspace_bytes(H, W, GX, GY, GL) == chunks * GL * 48 * (GX - 1) * (GY - 1) * 4, s
        assert len(seg[s[:2]]) == -(-W // R.SEG) and all(n * GL * 48 <= 49152 for _, _, _, n in seg[s[:2]])
    assert seg[3, 523] == [(0, 256, 0, 4), (256, 512, 2, 5), (512, 523, 5, 2)]
    assert seg[5, 257] == [(0, 256, 0, 9), (256, 257, 7, 2)]
    px = R.regime_case(*BY_SIZE[5, 257])["masks"]["out"]
    assert np.flatnonzero(px["on_x_node"][0]).tolist() == list(range(0, 256, 32)) and np.flatnonzero(px["on_y_node"][:, 0]).tolist() == [0, 2]
    assert px["last_col"][:, 256].all() and px["segment_start"][:, 256].all()
    assert len(seg[4, 769]) == 4 and [s[2] for s in seg[4, 769]] == [0, 0, 1, 1]
    assert lay[4, 769]["nx"].tolist() == [384, 385] and lay[4, 769]["ny"].tolist() == [4] and int(lay[4, 769]["chunk"].max()) == 1
    assert lay[700, 3]["nx"].tolist() == [3] and lay[700, 3]["npx"].tolist() == [[2100]] and int(lay[700, 3]["chunk"].max()) == 2
    assert 2100 % R.CHUNK not in (0, 2100)  # three chunks, the third partial
    for size in ((4, 769), (700, 3)):
        nodes = R.regime_case(*BY_SIZE[size])["masks"]["v_grid"]
        assert int(nodes["multi_chunk"].sum()) >= 8
    assert max(n for _, _, _, n in seg[7, 130]) * 16 * 48 == 49152 and len(seg[7, 130]) == 1
    assert lib.fg_bilagrid_bwd_workspace_bytes(7, 130, 64, 64, 16) == 16 * 48 * 63 * 63 * 4  # 12 MB
    big = R.regime_case(*BY_SIZE[7, 130])
    assert int(big["masks"]["v_grid"]["unreached"].sum()) > 64 * 16 * (64 - 2 * 7) and int(big["masks"]["v_grid"]["sparse"].sum()) >= 2
    assert int((lay[7, 130]["npx"] == 0).sum()) > 0  # cells without a pixel: their workgroups write no partial block
    assert seg[5, 300] == [(0, 256, 0, 55), (256, 300, 53, 11)]
    tiny = R.regime_case(*BY_SIZE[2, 2])["masks"]["out"]
    assert bool((tiny["on_x_node"] | tiny["last_col"]).all()) and bool((tiny["on_y_node"] | tiny["last_row"]).all())
    assert (49 - 1) % (5 - 1) == 0 and (9 - 1) % (3 - 1) == 0
    both = R.regime_case(*BY_SIZE[9, 49])["masks"]["out"]
    assert int(both["on_x_node"][0].sum()) == 4 and int(both["on_y_node"][:, 0].sum()) == 2 and int((both["on_x_node"] & both["on_y_node"]).sum()) == 8
    assert len(seg[24, 600]) == 3 and seg[24, 600][1][2] > 0
    # the coherent input: (cell, chunk, wave)s of the gather that hold pixels and have both a touched and an untouched level
    c = R.regime_case(*BY_SIZE[24, 600])
    GL = 8
    fz = R.guidance(c["rgb"], GL)
    z0 = np.minimum(np.floor(np.clip(fz, 0, GL - 1)).astype(int), GL - 2)
    L = lay[24, 600]
    group = (L["cell"] * (int(L["chunk"].max()) + 1) + L["chunk"]) * 4 + L["wave"]
    mixed, levels = 0, []
    for g in np.unique(group):
        touched = np.zeros(GL, bool)
        touched[z0[group == g]] = True
        touched[z0[group == g] + 1] = True
        mixed += bool(touched.any() and not touched.all())
        levels.append(int(touched.sum()))
    print(f"coherent 24 x 600: {mixed} of {len(levels)} waves with pixels skip a level; they touch {min(levels)} .. {max(levels)} of {GL} levels")
    assert mixed == len(levels) >= 30 and max(levels) <= 3
    assert np.ptp(c["rgb"].mean(axis=(0, 1))) > 0.05  # the channels differ
    noise = R.regime_case(*BY_SIZE[3, 523])
    assert len(np.unique(z0)) > 3 and R.clear_of_knife_edges(c["rgb"], GL) and R.clear_of_knife_edges(noise["rgb"], 3)
    assert int(c["masks"]["out"]["coherent"].sum()) == 24 * 600 and "coherent" not in noise["masks"]["out"]


def test_every_regime_has_elements_and_every_element_a_regime():
    count = {}
    for s in R.SHAPES:
        c = R.regime_case(*s)
        for kind, names in (("out", R.PIXEL_REGIMES), ("v_grid", R.NODE_REGIMES)):
            masks = c["masks"][kind]
            assert set(masks) <= set(names) and bool(np.any(list(masks.values()), axis=0).all()), s
            for k, m in masks.items():
                count[kind, k] = max(count.get((kind, k), 0), int(m.sum()))
        px = c["masks"]["out"]
        assert int(px.get("near_node", np.zeros(s[:2], bool))[c["placed"]].sum()) == int(c["placed"].sum())  # placed on purpose, all labelled
        if "segment_start" in px:
            assert np.flatnonzero(px["segment_start"][0]).tolist() == list(range(256, s[1], 256))
        nodes = c["masks"]["v_grid"]
        if "unreached" in nodes:
            assert bool((c["r64"]["v_grid_acc"][:, nodes["unreached"]] == 0).all()) and bool((c["r64"]["v_grid"][:, nodes["unreached"]] == 0).all())
            assert bool((c["r32"]["v_grid"][:, nodes["unreached"]] == 0).all())
        assert all(bool((c["r64"][a + "_acc"] >= 0).all()) and bool(np.isfinite(c["r64"][a]).all()) for a in R.ARRAYS)
        for a in R.ARRAYS:
            for e in c["e32"][a].values():
                assert R.FLOOR <= e < 1e-2, (s, a, e)
    print({k: v for k, v in count.items()})
    for kind, names in (("out", R.PIXEL_REGIMES), ("v_grid", R.NODE_REGIMES)):
        for k in names:
            assert count.get((kind, k), 0) >= 2, (kind, k)


@pytest.mark.parametrize("S,n", [(2, 2), (3, 2), (7, 64), (523, 7), (257, 9), (769, 3), (130, 64), (16384, 64), (16384, 2), (1920, 16)])
def test_integer_maps_partition_an_axis(S, n):
    """Each pixel lies in exactly one cell's [first_px, end_px), and cell_of names that cell."""
    cells = np.arange(n - 1)
    first, end = R.first_px(cells, S, n), R.end_px(cells, S, n)
    assert first[0] == 0 and end[-1] == S and bool((end[:-1] == first[1:]).all()) and bool((end >= first).all())
    owner = np.repeat(cells, end - first)
    assert owner.shape == (S,) and bool((owner == R.cell_of(np.arange(S), S, n)).all())


def test_floor_of_the_fp32_quotient_is_the_integer_cell():
    """What cell_frac of csrc/bilagrid.hip rests on: floor(float32(p (n-1)) / float32(S-1)) is the integer quotient
    p (n-1) / (S-1), at both pixels around every cell boundary (the first pixel of cell c and the one before it, c = 1 .. n-1:
    the last is the last pixel, on node n-1), for every S in 2 .. 16384 and n in 2 .. 64.  Were it false for one (S, n, p), the
    slice would index one LDS node past what its segment loaded."""
    S = np.arange(2, 16385, dtype=np.int64)[None, :]
    mismatches = checked = 0
    for n in range(2, 65):
        c = np.arange(1, n, dtype=np.int64)[:, None]
        first = R.first_px(c, S, n)
        for p in (first, first - 1):
            ok = (p >= 0) & (p <= S - 1)
            assert bool(ok.all())
            f = (p * (n - 1)).astype(np.float32) / (S - 1).astype(np.float32)
            assert f.dtype == np.float32
            mismatches += int((np.floor(f).astype(np.int64) != p * (n - 1) // (S - 1)).sum())
            checked += p.size
    print(f"{checked} (S, n, p) checked, {mismatches} mismatches")
    assert checked > 6e7 and mismatches == 0


# ---------------------------------------------------------------------------------------------------------------------
# teeth

CLAMPED = ("black", "white", "below_range", "above_range")
# (mutant, shapes (by size), arrays, the elements it concerns)
#   "all": every element that a pixel reaches            "interior": pixels under the interior regime (not grey, in range)
#   "clamped": black, white and out-of-range pixels      "changed": the sums that lose a term (their accumulation changes)
#   "shifted": pixels of a segment with cx_lo > 0        "stale": the sums that receive a stale sum other than zero
MUTANT_CASES = [
    ("align_corners_false", [(37, 53), (9, 49)], R.ARRAYS, "all"),
    ("luma_weights_permuted", [(37, 53), (24, 600)], R.ARRAYS, "interior"),
    ("slope_not_zeroed_outside_range", [(37, 53), (3, 523), (7, 130)], ("v_rgb",), "clamped"),
    ("slope_without_GL_minus_1", [(37, 53), (3, 523), (7, 130)], ("v_rgb",), "interior"),
    ("last_column_dropped_from_the_gather", [(37, 53), (5, 257), (4, 769), (7, 130)], ("v_grid",), "changed"),
    ("last_chunk_pixel_dropped", [(4, 769), (700, 3)], ("v_grid",), "changed"),
    ("second_chunk_dropped", [(4, 769), (700, 3)], ("v_grid",), "changed"),
    ("neighbour_row_ty", [(37, 53), (24, 600), (700, 3)], ("v_grid",), "all"),
    ("x_node_shifted_in_later_segments", [(3, 523), (5, 257), (5, 300), (24, 600)], ("out", "v_rgb"), "shifted"),
    ("skipped_level_keeps_previous_sums", [(24, 600)], ("v_grid",), "stale"),
]


def _smallest_e32(c, name):
    """Per element: the smallest E32 among the regimes it carries (the GPU test checks it under each)."""
    like = c["r64"][name]
    e = np.full(like.shape, np.inf)
    for regime, mask in c["masks"][name].items():
        full = np.broadcast_to(mask[..., None] if like.shape[:2] == mask.shape else mask[None], like.shape)
        e = np.where(full, np.minimum(e, c["e32"][name][regime]), e)
    return e


@functools.lru_cache(maxsize=None)
def mutant_cells(factor):
    """-> {(mutant, shape tag, array): (caught, elements, cap)}: an element of the mutant's float64 result is CAUGHT when
    the GPU test would flag it: at least 4 * factor * E32 of its accumulation from the true one, E32 the smallest of its
    regimes'.  ``cap``: the largest F at which three quarters of the concerned elements are still caught."""
    out = {}
    for mutant, sizes, arrays, concerns in MUTANT_CASES:
        for size in sizes:
            shape = BY_SIZE[size]
            H, W, GX = shape[0], shape[1], shape[2]
            c = R.regime_case(*shape)
            r64 = c["r64"]
            rm = R.restate(c["grids"][c["cam"]], c["rgb"], c["v_out"], np.float64, mutant)
            px = c["masks"]["out"]
            for name in arrays:
                sel = r64[name + "_acc"] > 0
                if concerns == "changed":
                    sel = sel & (rm[name + "_acc"] != r64[name + "_acc"])
                elif concerns == "stale":
                    sel = sel & rm["got_stale"]
                elif concerns == "interior" and name != "v_grid":
                    sel = sel & px["interior"][..., None]
                elif concerns == "clamped":
                    sel = sel & np.any([px[k] for k in CLAMPED], axis=0)[..., None]
                elif concerns == "shifted":
                    cols = np.zeros(W, bool)
                    for x0, x1, lo, _ in R.segments(W, GX):
                        cols[x0:x1] = lo > 0
                    sel = sel & cols[None, :, None]
                ratios = (P.distance(rm[name], r64[name], r64[name + "_acc"]) / _smallest_e32(c, name))[sel]
                out[(mutant, c["tag"], name)] = (int((ratios >= 4 * factor).sum()), ratios.size, P.three_quarter_cap(ratios))
    return out


def test_every_mutant_is_listed():
    assert [c[0] for c in MUTANT_CASES] == list(R.MUTANTS)


def test_mutants_are_caught_by_the_element_bound():
    """On at least three quarters of the elements a mutant concerns, in every shape and array listed for it, the mutant's
    float64 result is at least 4 * F * E32 of the element's accumulation from the true one (cancellation, or a weight near
    zero, may hide it on single elements): the GPU bound F * E32 has teeth, and this caps F."""
    factor = 1.0 if R.F is None else R.F
    cells = mutant_cells(factor)
    for (mutant, tag, name), (caught, n, cap) in cells.items():
        print(f"{mutant} | {tag} | {name}: {caught}/{n} elements caught at F = {factor:g}; caps F at {cap:.3g}")
    cap = min(v[2] for v in cells.values())
    print(f"the cap on F: {cap:.3g}")
    failures = [f"{k}: {v[0]}/{v[1]}" for k, v in cells.items() if v[1] < 2 or 4 * v[0] < 3 * v[1]]
    assert not failures, "\n".join(failures)
    assert R.F is None or R.F <= cap
