"""GPU checks of the clustering (``ops.dbscan`` / ``fg_dbscan``): labels, core flags and K EQUAL to the brute-force
restatement of the definition (tests/dbscan_restatement.py) wherever a CPU can afford one; at 200 000 rows an exact check
on the device through ``ops.knn``, whose squared distances are the same arithmetic; and the hand-off of a clustered mask to
the stage-2 model.  Nothing here has a tolerance except the last test, which uses the bar of the control tests."""
import copy

import numpy as np
import pytest
import torch

import helpers
import test_se3_apply_gpu as S
from dbscan_restatement import (labels_from_lists, neighbour_lists, permute_lists, renumber_by_lowest_core_row,
                                shared_border_case)
from freegaussian_amd import masks, ops
from freegaussian_amd.scenes import room_scene

pytestmark = pytest.mark.gpu


def _uniform(n, seed=0):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * 10


def _clustered(n, seed=0):
    x = _uniform(n, seed)
    x[: (4 * n) // 5] *= 0.2  # 80 % of the points scaled by 0.2 about the origin (as in test_knn_gpu.py)
    return x


_lists = {}


def _lists_of(name, make, eps):
    """The neighbour lists of a named set: the brute force over all pairs runs once per (set, eps)."""
    if name not in _lists:
        x = make().contiguous()
        _lists[name] = (x, *neighbour_lists(x.numpy(), eps)[:2])
    return _lists[name]


def _assert_equal(x, eps, min_samples, lists=None, tag=""):
    indptr, indices = lists if lists is not None else neighbour_lists(x.numpy(), eps)[:2]
    want_labels, want_core, want_k = labels_from_lists(indptr, indices, min_samples)
    labels, core, k = ops.dbscan(x.cuda(), eps, min_samples)
    n = x.shape[0]
    assert labels.shape == (n,) and labels.dtype == torch.int32 and labels.is_cuda
    assert core.shape == (n,) and core.dtype == torch.bool and core.is_cuda and isinstance(k, int)
    border = int(((want_labels >= 0) & ~want_core).sum())
    bad = int((labels.cpu().numpy() != want_labels).sum())
    print(f"{tag} n={n} eps={eps} min_samples={min_samples}: K {k} (want {want_k}), {int(want_core.sum())} core, {border} border, "
          f"{int((want_labels < 0).sum())} noise rows; {bad} labels differ")  # fmt: skip
    assert torch.equal(core.cpu(), torch.from_numpy(want_core))
    assert torch.equal(labels.cpu(), torch.from_numpy(want_labels))
    assert k == want_k
    return labels, core, k


def test_tiny_and_odd_sizes():
    one = torch.tensor([[0.3, -1.0, 2.0]])
    labels, core, k = _assert_equal(one, 0.5, 1)
    assert labels.tolist() == [0] and core.tolist() == [True] and k == 1
    labels, core, k = _assert_equal(one, 0.5, 2)
    assert labels.tolist() == [-1] and core.tolist() == [False] and k == 0
    for n, seed in ((63, 1), (257, 2)):
        for min_samples in (1, 3):
            _assert_equal(torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * 2, 0.3, min_samples)


def test_identical_points_and_one_ball():
    labels, core, k = _assert_equal(torch.full((1500, 3), 0.37), 0.5, 4)
    assert k == 1 and bool(core.all()) and not bool(labels.any())
    # 4096 points inside one eps-ball: every row neighbours every row
    ball = torch.rand(4096, 3, generator=torch.Generator().manual_seed(3)) * 0.25 + 7.0
    labels, core, k = _assert_equal(ball, 0.5, 16)
    assert k == 1 and bool(core.all())
    assert _assert_equal(ball, 0.5, 4097)[2] == 0  # one more than there are rows: nothing is core


def test_chains_over_many_cells_and_workgroups():
    eps = 0.5
    t = torch.arange(4096, dtype=torch.float32)[:, None] * (0.9 * eps)
    chain = torch.cat([t, torch.full_like(t, 1.5), torch.full_like(t, -2.0)], dim=1)
    lists = neighbour_lists(chain.numpy(), eps)[:2]
    labels, core, k = _assert_equal(chain, eps, 2, lists, "chain")
    assert k == 1 and bool(core.all())
    _assert_equal(chain, eps, 3, lists, "chain")  # the two end rows are border rows
    perm = torch.randperm(4096, generator=torch.Generator().manual_seed(4))
    labels, core, k = _assert_equal(chain[perm], eps, 2, permute_lists(*lists, perm.numpy()), "chain, random row order")
    assert k == 1
    # two chains 1.1 eps apart stay two clusters, in either row order
    two = torch.cat([chain[:2048], chain[:2048] + torch.tensor([0.0, 1.1 * eps, 0.0])])
    labels, core, k = _assert_equal(two, eps, 2, tag="two chains")
    assert k == 2 and labels[:2048].unique().tolist() == [0] and labels[2048:].unique().tolist() == [1]
    assert _assert_equal(two[perm], eps, 2, tag="two chains, random row order")[2] == 2


def test_pairs_at_exactly_eps_and_the_shared_border_row():
    pairs = torch.zeros(64, 3)
    pairs[:, 1] = torch.arange(64).div(2, rounding_mode="floor") * 3.0  # 32 pairs, 3 apart
    pairs[1::2, 0] = 0.5
    labels, core, k = _assert_equal(pairs, 0.5, 2)
    assert k == 32 and bool(core.all())  # 0.5 - 0 == eps in fp32: d2 == eps2 is a neighbour
    x, eps, min_samples, lone = shared_border_case()
    labels, core, k = _assert_equal(torch.from_numpy(x), eps, min_samples)
    assert k == 2 and not bool(core[lone]) and int(labels[lone]) == 0


def test_eps_against_the_extent_outliers_and_non_finite_rows():
    g = torch.Generator().manual_seed(5)
    x = torch.rand(3000, 3, generator=g) * 4 - 2
    assert _assert_equal(x, 100.0, 4, tag="eps above the extent")[2] == 1
    # eps below extent / 1024: the cells are wider than eps; two outliers at 1e6, three rows that are not numbers
    y = torch.rand(3000, 3, generator=g) * 2000
    y[:600] = y[600:1200] + (torch.rand(600, 3, generator=g) - 0.5) * 0.5  # 600 rows with a close companion
    y[7] = torch.tensor([1e6, 1e6, 1e6])
    y[1999] = torch.tensor([-1e6, 3.0, 1e6])
    y[11, 0] = float("nan")
    y[1200, 2] = float("inf")
    y[2999] = torch.tensor([float("-inf"), float("nan"), 0.0])
    for min_samples in (1, 2):
        labels, core, k = _assert_equal(y, 0.6, min_samples, tag="eps below extent / 1024")
        for bad in (11, 1200, 2999):
            assert int(labels[bad]) == -1 and not bool(core[bad])  # (not even at min_samples 1: such a row is no neighbour of itself)
    assert k > 100


@pytest.mark.parametrize("min_samples", [1, 2, 4, 16])
def test_uniform_20k_equals_the_restatement(min_samples):
    x, indptr, indices = _lists_of("uniform", lambda: _uniform(20_000), 0.5)
    _assert_equal(x, 0.5, min_samples, (indptr, indices), "uniform")


def test_clustered_20k_equals_the_restatement():
    x, indptr, indices = _lists_of("clustered", lambda: _clustered(20_000), 0.3)
    for min_samples in (2, 8):
        _assert_equal(x, 0.3, min_samples, (indptr, indices), "clustered")


def test_two_runs_and_a_row_permutation():
    x, indptr, indices = _lists_of("uniform", lambda: _uniform(20_000), 0.5)
    xd = x.cuda()
    a = ops.dbscan(xd, 0.5, 4)
    b = ops.dbscan(xd, 0.5, 4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    perm = torch.randperm(20_000, generator=torch.Generator().manual_seed(6))
    p = ops.dbscan(xd[perm.cuda()], 0.5, 4)
    assert p[2] == a[2] and torch.equal(p[1].cpu(), a[1].cpu()[perm])
    # the core rows: the permuted partition, its clusters renumbered by lowest (core) row
    want = renumber_by_lowest_core_row(a[0].cpu().numpy()[perm.numpy()], p[1].cpu().numpy())
    got = np.where(p[1].cpu().numpy(), p[0].cpu().numpy(), -1)
    assert np.array_equal(got, want)
    # every row, the border rows by the rule (the lowest NEW number among their core neighbours): the permuted lists
    want_labels, want_core, want_k = labels_from_lists(*permute_lists(indptr, indices, perm.numpy()), 4)
    assert torch.equal(p[0].cpu(), torch.from_numpy(want_labels)) and p[2] == want_k


def test_200k_rows_exactly_through_knn_on_the_device():
    """min_samples 4: a row is core iff its THIRD other neighbour is within eps, and a non-core row has at most two other
    neighbours, so the 8 nearest of ``ops.knn`` (squared distances in the arithmetic of the definition) hold all of them."""
    n, eps, min_samples = 200_000, 0.15, 4
    x = _uniform(n, seed=7).cuda()
    labels, core, k = ops.dbscan(x, eps, min_samples)
    d2, idx = ops.knn(x, 8, squared=True)
    e = torch.tensor(eps, dtype=torch.float32, device=x.device)
    near = d2 <= e * e
    idx = idx.long()
    assert torch.equal(core, near[:, min_samples - 2])
    print(f"200k: K {k}, {int(core.sum())} core, {int(((labels >= 0) & ~core).sum())} border, {int((labels < 0).sum())} noise rows")
    assert bool(core.any()) and bool((~core).any()) and bool(((labels >= 0) & ~core).any()) and bool((labels < 0).any())
    core_near = near & core[idx]
    lab = labels.long()
    # a non-core row: the minimum label over its core neighbours, -1 without one
    big = torch.iinfo(torch.int64).max
    low = torch.where(core_near, lab[idx], torch.full_like(idx, big)).min(dim=1).values
    want = torch.where(low == big, torch.full_like(low, -1), low)
    assert torch.equal(lab[~core], want[~core])
    # a core row: labelled, and its core neighbours share the label
    assert bool((lab[core] >= 0).all())
    assert bool((~core_near | (lab[idx] == lab[:, None]))[core].all())
    # K distinct labels 0..K-1, numbered by ascending lowest core row
    assert k == int(lab[lab >= 0].unique().numel()) and int(lab.max()) == k - 1
    rows = torch.arange(n, device=x.device)
    first = torch.full((k,), n, dtype=torch.int64, device=x.device).scatter_reduce(0, lab[core], rows[core], "amin")
    assert bool((first[1:] > first[:-1]).all()) and bool((first < n).all())


def _room_control_model(gaussian_mask, means):
    from freegaussian_amd.model import FreeGaussianControlModel, FreeGaussianModel, FreeGaussianModelConfig

    _, cam = S._model_and_camera(n=8)  # (its camera: 64 x 64, looking at the origin from z = -3)
    torch.manual_seed(0)
    base = FreeGaussianModel(FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000), seed_points=means,
                             init_scales=-3.0)  # fmt: skip
    with torch.no_grad():
        for p in base.deform.parameters():
            p.mul_(0.3)
    init_cam = type(cam)(cam.camera_to_worlds, cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, times=torch.tensor([[0.0]]))
    cm = FreeGaussianControlModel(gaussian_mask, init_cam, config=FreeGaussianModelConfig(background_color="black"),
                                  seed_points=means.clone())  # fmt: skip
    cm.load_state_dict(base.state_dict(), strict=False)
    cam.metadata["cameras0"] = init_cam
    return cm.train(), cam  # (training mode, as the control tests run it)


def test_clustered_mask_drives_the_control_model(monkeypatch):
    means = room_scene(2000, 64, 64)[0].means.detach().float().contiguous()
    # two separated blobs: everything within 0.7 of row 0 and of the row farthest from it
    a = means[0]
    b = means[(means - a).norm(dim=1).argmax()]
    in_a, in_b = (means - a).norm(dim=1) <= 0.7, (means - b).norm(dim=1) <= 0.7
    assert int(in_a.sum()) >= 4 and int(in_b.sum()) >= 4 and float((a - b).norm()) > 3.0
    dynamic = (in_a | in_b).cuda()
    # eps 0.75: each blob's centre neighbours the whole blob, the blobs are more than 1.6 apart
    mask = masks.cluster_gaussian_masks(means.cuda(), dynamic, 0.75, min_samples=2)
    assert mask.shape == (2000, 2) and mask.dtype == torch.bool and mask.is_cuda
    assert torch.equal(mask[:, 0].cpu(), in_a) and torch.equal(mask[:, 1].cpu(), in_b)  # row 0 is in the first cluster
    assert ops.control_plan(mask).n == int(dynamic.sum())
    cm, cam = _room_control_model(mask.cpu(), means)
    images = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("FG_FUSED_CONTROL", knob)
        images[knob] = copy.deepcopy(cm).cuda().get_outputs(cam)["rgb"].detach().cpu()
        assert bool(torch.isfinite(images[knob]).all()) and float(images[knob].max()) > 0.05
    bar = S._bar(images["1"], images["0"])
    print(f"control model on a clustered mask, fused against unset: {bar:.2e}")
    assert bar <= helpers.REL_TOL
