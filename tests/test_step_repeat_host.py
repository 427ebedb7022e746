"""CPU: the count ``k`` of float-atomic addends per splat (tests/step_repeat_common.py) and the bound it carries.

    the census of the training step's scene (the flaky test's log-scales, and the repaired test's) and of the three small
        raster scenes: which of k = 1, k = 2, k >= 3 occur
    ``addend_count`` + ``groups_from_jobs`` against a count by explicit loops on a hand-built job list
    ``2 (k - 1) 2^-24 A`` against the fp32 partial sums of the restatement added in EVERY order, k = 3 and 4

Nothing of the package's native code runs here."""
import itertools

import pytest
import torch

import raster_restatement as R
import step_repeat_common as C


@pytest.fixture(scope="module")
def scenes():
    return {name: C.raster_scene(name) for name in C.RASTER_SCENES}


def _default_groups(name, scene):
    nt = C.n_tiles_of(scene)
    if C.RASTER_SCENES[name][4] == "classic":
        return C.groups_classic(nt)
    return torch.tensor([[15, 0, 0, 0]] * nt, dtype=torch.int64)  # list shares: one addend per (splat, tile)


def test_the_old_step_had_a_row_with_three_addends_and_the_new_one_has_none():
    """One 16 x 16 tile is ONE workgroup of FOUR wavefronts (classic launch, one pixel per lane below 3000 tiles), each
    adding for its own four pixel rows: "one job per splat" never meant one addend.  At the flaky test's log-scales
    (mean -3.8) rows with three addends exist -- a handful of rows whose sum depends on the order, which is what "two
    outcomes" looks like; at the repaired test's (-5.2) no row has more than two."""
    assert C.launch_of(C.W_STEP, C.H_STEP) == "classic" and C.classic_ppt_bwd(1) == 1
    old = C.scene_addends(C.step_scene_host(C.OLD_SCALE_MEAN), C.groups_classic(1))
    new = C.scene_addends(C.step_scene_host(C.SCALE_MEAN), C.groups_classic(1))
    print("k census, step scene on the CPU: log-scale mean -3.8", C.census(old), " -5.2", C.census(new))
    c_old, c_new = C.census(old), C.census(new)
    assert c_old["1"] > 0 and c_old["2"] > 0 and c_old[">=3"] > 0
    assert c_new["1"] > 0 and c_new["2"] > 0 and c_new[">=3"] == 0 and c_new["max"] == 2


@pytest.mark.parametrize("name", list(C.RASTER_SCENES))
def test_every_class_is_populated_in_the_small_scenes(name, scenes):
    sc = scenes[name]
    assert C.launch_of(sc.width, sc.height) == C.RASTER_SCENES[name][4]
    assert 200 <= sc.means2d.shape[0] <= 5000
    last = C.host_last_ids(sc)
    assert torch.equal(last, R.composite(sc, 3, torch.float64)["last_ids"])  # (the chunked walk is the restatement's)
    c = C.census(C.scene_addends(sc, _default_groups(name, sc), last))
    print(f"k census, {name}: {c}")
    assert min(c["1"], c["2"], c[">=3"]) >= 20, c


def test_job_lists_start_at_200_tiles():
    assert C.n_tiles_of(C.raster_scene("job_lists")) == C.MIXED_MIN_TILES
    assert C.launch_of(320, 160) == "jobs" and C.launch_of(16 * 199, 16) == "classic" and C.launch_of(304, 160) == "classic"


# ---- the count against explicit loops ---------------------------------------------------------------------------------------
def _tiny():
    g = torch.Generator().manual_seed(11)
    n = 14
    xy = torch.stack([torch.rand(n, generator=g) * 32, torch.rand(n, generator=g) * 16], -1)
    s = 0.5 + 3.5 * torch.rand(n, generator=g, dtype=torch.float64)
    return R.with_lists(xy, R.conic_of(s, s, torch.zeros(n, dtype=torch.float64)).float(), 0.1 + 0.3 * torch.rand(n, generator=g),
                        1.0 + torch.rand(n, generator=g), (torch.ceil(3.5 * s) + 1).to(torch.int32), torch.rand(n, 8, generator=g),
                        ["tiny"] * n, 32, 16)  # fmt: skip


def _job_list(cap, n_tiles, per_xcd):
    jobs = torch.zeros(8 + 8 * cap + n_tiles, dtype=torch.int32)
    for xcd, entries in per_xcd.items():
        jobs[xcd] = len(entries)
        jobs[8 + xcd * cap : 8 + xcd * cap + len(entries)] = torch.tensor(entries, dtype=torch.int32)
    return jobs


ROWS = {s: list(range(4 * s, 4 * s + 4)) for s in range(4)}


def test_the_count_equals_explicit_loops_on_a_hand_built_job_list():
    sc = _tiny()
    n, last = sc.means2d.shape[0], C.host_last_ids(sc)
    gid, tile, hits = C.strip_hits(sc.means2d, sc.conics, sc.opacities, sc.offsets, sc.flatten_ids, last, 32, 16)
    args = (n, sc.means2d, sc.conics, sc.opacities, sc.offsets, sc.flatten_ids, last, 32, 16)
    # pixel strips: tile 0 as two two-strip jobs (strip 4, 5: rows {0-3, 8-11} and {4-7, 12-15}), on XCDs 0 and 3; tile 1 as
    # one single-strip job each, spread over three XCDs
    strips = _job_list(4, 2, {0: [0 << 3 | 5], 3: [0 << 3 | 6, 1 << 3 | 1], 5: [1 << 3 | 4, 1 << 3 | 2], 7: [1 << 3 | 3]})
    G = C.groups_from_jobs(strips, 2, False, sc.offsets)
    assert G.tolist() == [[5, 10, 0, 0], [1, 8, 2, 4]]
    want = C.addend_count_brute(*args, {0: [ROWS[0] + ROWS[2], ROWS[1] + ROWS[3]], 1: [ROWS[0], ROWS[3], ROWS[1], ROWS[2]]})
    got = C.addend_count(n, gid, tile, hits, G)
    assert torch.equal(got, want) and int(want.max()) >= 3, (got, want)
    # a whole-tile job and a classic workgroup of four wavefronts
    G = C.groups_from_jobs(_job_list(4, 2, {1: [0 << 3 | 0], 2: [1 << 3 | 0]}), 2, False, sc.offsets)
    assert G.tolist() == [[15, 0, 0, 0]] * 2
    whole = C.addend_count_brute(*args, {0: [list(range(16))], 1: [list(range(16))]})
    assert torch.equal(C.addend_count(n, gid, tile, hits, G), whole) and int(whole.max()) <= 2
    classic = C.addend_count_brute(*args, {t: [ROWS[0], ROWS[1], ROWS[2], ROWS[3]] for t in (0, 1)})
    assert torch.equal(C.addend_count(n, gid, tile, hits, C.groups_classic(2)), classic)
    assert bool((classic >= whole).all()) and int(classic.sum()) > int(whole.sum())
    # list shares: tile 0 in three parts (rotated), tile 1 whole: one addend per (splat, tile) either way
    shares = _job_list(4, 2, {0: [0 << 12 | 2 << 6 | 2, 1 << 12 | 0 << 6 | 0], 4: [0 << 12 | 0 << 6 | 2], 6: [0 << 12 | 1 << 6 | 2]})
    assert torch.equal(C.addend_count(n, gid, tile, hits, C.groups_from_jobs(shares, 2, True, sc.offsets)), whole)
    # a list that leaves a part out, or a tile with a list and no job, is refused
    with pytest.raises(AssertionError):
        C.groups_from_jobs(_job_list(4, 2, {0: [0 << 12 | 2 << 6 | 2, 1 << 12], 4: [0 << 12 | 0 << 6 | 2]}), 2, True, sc.offsets)
    with pytest.raises(AssertionError):
        C.groups_from_jobs(_job_list(4, 2, {1: [0 << 3 | 0]}), 2, False, sc.offsets)


# ---- the bound -----------------------------------------------------------------------------------------------------------
def _wave_partials(sc):
    """([waves, N, 16] fp32 partial sums of the restatement, one per (tile, 4-row strip); A [N,16] float64).  The backward is
    linear in each pixel's cotangent, so a wavefront's addend is the backward of the cotangent image masked to its rows."""
    vr = C.raster_cotangent(sc)
    va = torch.zeros(sc.height, sc.width, dtype=torch.float64)
    alpha64 = R.composite(sc, 3, torch.float64)["alpha"]
    alpha32 = R.composite(sc, 3, torch.float32)["alpha"]
    _, accum = R.backward(sc, 3, vr, va, alpha64, torch.float64)
    tw = (sc.width + 15) // 16
    parts = []
    for t in range(C.n_tiles_of(sc)):
        ty, tx = divmod(t, tw)
        for s in range(4):
            mask = torch.zeros(sc.height, sc.width, 1, dtype=torch.float64)
            mask[ty * 16 + 4 * s : ty * 16 + 4 * s + 4, tx * 16 : tx * 16 + 16] = 1.0
            g, _ = R.backward(sc, 3, vr * mask, va, alpha32, torch.float32)
            p = torch.zeros(sc.means2d.shape[0], 16)
            p[:, 0:2], p[:, 2:3], p[:, 3:6], p[:, 6:8], p[:, 8:11] = g["means2d"], g["opacities"], g["conics"], g["absgrad"], g["features"]
            parts.append(p)
    return torch.stack(parts), C.accum_slots(accum)


@pytest.mark.parametrize("name", ["one_tile", "two_tiles"])
def test_no_order_of_the_partial_sums_exceeds_the_bound(name, scenes):
    sc = scenes[name]
    n, nt = sc.means2d.shape[0], C.n_tiles_of(sc)
    gid, tile, hits = C.strip_hits(sc.means2d, sc.conics, sc.opacities, sc.offsets, sc.flatten_ids, C.host_last_ids(sc),
                                   sc.width, sc.height)  # fmt: skip
    k = C.addend_count(n, gid, tile, hits, C.groups_classic(nt))
    present = torch.zeros(n, nt * 4, dtype=torch.bool)  # (row, wavefront): the wavefront adds into the row
    for s in range(4):
        on = (hits >> s) & 1 == 1
        present[gid[on], tile[on] * 4 + s] = True
    assert torch.equal(present.sum(1), k)
    partials, A = _wave_partials(sc)
    assert not bool((partials[~present.t()] != 0).any())  # nothing arrives from a wavefront the count leaves out
    bound = C.order_bound(k, A)
    changed = {3: 0, 4: 0}
    for kk in (3, 4):
        rows = (k == kk).nonzero().flatten().tolist()
        assert len(rows) >= 5, (name, kk, len(rows))
        for r in rows:
            p = partials[present[r].nonzero().flatten(), r]  # [kk, 16] fp32
            sums = []
            for order in itertools.permutations(range(kk)):
                acc = torch.zeros(16)
                for j in order:
                    acc = acc + p[j]
                sums.append(acc)
            sums = torch.stack(sums).double()
            spread = sums.max(0).values - sums.min(0).values
            assert bool((spread <= bound[r]).all()), (name, r, kk, spread.tolist(), bound[r].tolist())
            changed[kk] += int(bool((spread > 0).any()))
    print(f"{name}: rows whose sum depends on the order: k = 3: {changed[3]}, k = 4: {changed[4]}")
    assert changed[3] > 0 and changed[4] > 0
    # k <= 2: every order gives the same bits
    for r in (k == 2).nonzero().flatten().tolist()[:40]:
        a, b = partials[present[r].nonzero().flatten(), r]
        assert torch.equal((torch.zeros(16) + a) + b, (torch.zeros(16) + b) + a)


# ---- the two checkers have teeth -------------------------------------------------------------------------------------------
def _ulp_up(t, index):
    t = t.clone()
    flat = t.view(-1).view(torch.int32)
    flat[index] += 1
    return t


def test_one_ulp_in_one_of_eight_runs_fails_the_bit_contract():
    g = torch.Generator().manual_seed(0)
    base = dict(a=torch.randn(50, 3, generator=g), b=torch.randn(7, generator=g))
    runs = [dict(base) for _ in range(C.REPEATS)]
    assert C.bit_failures("t", runs) == []
    runs[5] = dict(a=_ulp_up(base["a"], 77), b=base["b"])
    fails = C.bit_failures("t", runs)
    assert len(fails) == 1 and "run 5" in fails[0] and "1 elements of a" in fails[0]


def test_the_order_contract_fails_under_both_mutations(scenes):
    sc = scenes["one_tile"]
    k = C.scene_addends(sc, C.groups_classic(1))
    _, A = _wave_partials(sc)
    bound = C.order_bound(k, A)
    g = torch.randn(sc.means2d.shape[0], 16, generator=torch.Generator().manual_seed(1)) * A.float()
    runs = [g.clone() for _ in range(C.REPEATS)]
    assert C.order_failures("t", runs, k, bound) == []
    # inside the bound: half of it on a k >= 3 row passes
    r3 = int((k >= 3).nonzero()[0])
    inside = [x.clone() for x in runs]
    inside[3][r3, 4] += float(0.5 * bound[r3, 4])
    assert float(bound[r3, 4]) > 0 and C.order_failures("t", inside, k, bound) == []
    # 4 (k - 1) 2^-24 A on one slot of a k >= 3 row: twice the bound
    outside = [x.clone() for x in runs]
    outside[3][r3, 4] += float(2.0 * bound[r3, 4])
    fails = C.order_failures("t", outside, k, bound)
    assert len(fails) == 1 and "k >= 3" in fails[0] and f"first row {r3} " in fails[0]
    # one ulp on a k <= 2 row
    r2 = int(((k == 2) & (g[:, 8] != 0)).nonzero()[0])
    ulp = [x.clone() for x in runs]
    ulp[6] = _ulp_up(ulp[6], r2 * 16 + 8)
    fails = C.order_failures("t", ulp, k, bound)
    assert len(fails) == 1 and "k <= 2" in fails[0] and f"first row {r2} " in fails[0]
