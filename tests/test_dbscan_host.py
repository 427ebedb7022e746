"""CPU checks around the GPU DBSCAN (``ops.dbscan`` / ``fg_dbscan``): the restatement of its definition against
scikit-learn, the constructed shared-border case, the argument errors of the op, and the two host functions of ``masks``
that turn flow maps and labels into a stage-2 mask (with ``ops.dbscan`` replaced by the restatement)."""
import numpy as np
import pytest
import torch

from dbscan_restatement import dbscan as restated
from dbscan_restatement import labels_from_lists, neighbour_lists, permute_lists, shared_border_case
from freegaussian_amd import _lib, masks, ops

GAP = 1e-5  # no pair distance within this relative distance of eps: fp32 and float64 then agree on every neighbour
# (the seeds below are sets that meet it; at 1500 rows and eps 1.1 about a million pairs lie near eps and seeds 3 and 6,
# with gaps of 5.0e-6 and 2.9e-7, do not)


@pytest.mark.parametrize("seed, n, eps", [(0, 200, 0.5), (1, 700, 0.7), (2, 1100, 0.9), (7, 1500, 1.1), (4, 1500, 0.5),
                                          (5, 400, 1.1)])  # fmt: skip
def test_restatement_is_sklearn_away_from_the_rounding_edge(seed, n, eps):
    cluster = pytest.importorskip("sklearn.cluster")
    x = (torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * 10).numpy()
    indptr, indices, gap = neighbour_lists(x, eps, want_gap=True)
    print(f"seed {seed} n {n} eps {eps}: gap {gap:.3e}")
    assert gap > GAP  # the condition under which the two must agree
    for min_samples in (1, 2, 4, 8):
        labels, core, k = labels_from_lists(indptr, indices, min_samples)
        ref = cluster.DBSCAN(eps=eps, min_samples=min_samples, algorithm="brute").fit(x.astype(np.float64))
        want_core = np.zeros(n, dtype=bool)
        want_core[ref.core_sample_indices_] = True
        border = int(((labels >= 0) & ~core).sum())
        print(f"  min_samples {min_samples}: K {k}, {int(core.sum())} core, {border} border rows")
        assert np.array_equal(core, want_core)
        assert np.array_equal(labels, ref.labels_.astype(np.int32))
        assert k == int(ref.labels_.max()) + 1


def test_shared_border_row_takes_the_lowest_numbered_cluster():
    x, eps, min_samples, lone = shared_border_case()
    indptr, indices, _ = neighbour_lists(x, eps)
    labels, core, k = labels_from_lists(indptr, indices, min_samples)
    near = indices[indptr[lone] : indptr[lone + 1]]
    assert not core[lone] and core[:lone].all() and k == 2
    assert set(labels[near[near != lone]].tolist()) == {0, 1}  # core neighbours in both clusters
    assert np.array_equal(labels[:9], np.zeros(9)) and np.array_equal(labels[9:18], np.ones(9))  # the far grid holds the lowest rows
    assert labels[lone] == 0


def test_restatement_edge_rules():
    # a pair at exactly eps is a pair of neighbours; a non-finite row neighbours nobody, itself included
    x = np.array([[0, 0, 0], [0.5, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [0.25, 0, 0]], dtype=np.float32)
    labels, core, k, _ = restated(x, 0.5, 3)
    assert core.tolist() == [True, True, False, False, True] and labels.tolist() == [0, 0, -1, -1, 0] and k == 1
    labels, core, k, _ = restated(x, 0.5, 1)
    assert core.tolist() == [True, True, False, False, True] and labels.tolist() == [0, 0, -1, -1, 0] and k == 1
    # the permuted lists are the lists of the permuted points
    y = (torch.rand(300, 3, generator=torch.Generator().manual_seed(9)) * 4).numpy()
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(10)).numpy()
    a = labels_from_lists(*permute_lists(*neighbour_lists(y, 0.5)[:2], perm), 4)
    b = restated(y[perm], 0.5, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_dbscan_argument_errors(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    x = torch.zeros(5, 3)
    for shape in ((5, 2), (5, 4), (15,), (1, 5, 3), (0, 3)):
        with pytest.raises(ValueError):
            ops.dbscan(torch.zeros(shape), 0.5)
    for eps in (0.0, -1.0, float("nan"), float("inf"), None, "0.5", True, 1e-30, 1e30):
        with pytest.raises(ValueError):
            ops.dbscan(x, eps)
    for min_samples in (0, -1, 65536, 2.0, None, True):
        with pytest.raises(ValueError):
            ops.dbscan(x, 0.5, min_samples)
    with pytest.raises(ValueError):
        ops.dbscan(x.double(), 0.5)
    with pytest.raises(_lib.FgRasterError):  # in order but on the CPU: there is no CPU path
        ops.dbscan(x, 0.5, 4)


def test_flow_motion_labels():
    flow = torch.zeros(4, 5, 2)
    flow[0, 0] = torch.tensor([3.0, 4.0])  # |flow| = 5
    flow[0, 1] = torch.tensor([0.6, 0.8])  # |flow| = 1: not above a threshold of 1
    flow[1, 2] = torch.tensor([float("nan"), 9.0])
    flow[2, 3] = torch.tensor([float("inf"), 0.0])
    flow[3, 4] = torch.tensor([0.0, -2.0])
    labels, valids = masks.flow_motion_labels(flow, 1.0)
    assert labels.shape == (4, 5, 2) and labels.dtype == torch.bool and valids.tolist() == [True, True]
    want = torch.zeros(4, 5, dtype=torch.bool)
    want[0, 0] = want[3, 4] = True
    assert torch.equal(labels[..., 0], want) and torch.equal(labels[..., 1], ~want)
    assert masks.flow_motion_labels(flow, 0)[0][..., 0].sum() == 3  # the NaN and the inf pixel never move
    for bad in (torch.zeros(4, 5), torch.zeros(4, 5, 3)):
        with pytest.raises(ValueError):
            masks.flow_motion_labels(bad, 1.0)
    for bad in (-1.0, float("nan"), None):
        with pytest.raises(ValueError):
            masks.flow_motion_labels(flow, bad)


def _blobs():
    """40 rows: blobs of 5, 9, 5 and 2 dynamic points (in that row order, 10 apart) among static rows, one dynamic loner."""
    g = torch.Generator().manual_seed(3)
    means = torch.rand(40, 3, generator=g) * 0.1 + 100.0  # the static rows: a dense clump that must never be clustered
    dynamic = torch.zeros(40, dtype=torch.bool)
    rows = {"a": range(2, 7), "b": range(10, 19), "c": range(20, 25), "d": range(30, 32), "loner": range(35, 36)}
    for i, (name, r) in enumerate(rows.items()):
        r = list(r)
        means[r] = torch.rand(len(r), 3, generator=g) * 0.1 + 10.0 * i
        dynamic[r] = True
    return means, dynamic, {k: list(v) for k, v in rows.items()}


def test_cluster_gaussian_masks_columns(monkeypatch):
    calls = []

    def on_the_cpu(x, eps, min_samples=4):
        calls.append((tuple(x.shape), eps, min_samples))
        labels, core, k, _ = restated(x.numpy(), eps, min_samples)
        return torch.from_numpy(labels), torch.from_numpy(core), k

    monkeypatch.setattr(ops, "dbscan", on_the_cpu)
    means, dynamic, rows = _blobs()

    def column(names):
        m = torch.zeros(40, len(names), dtype=torch.bool)
        for c, name in enumerate(names):
            m[rows[name], c] = True
        return m

    # min_samples 2: four clusters in row order, the loner is noise, static rows are never looked at
    m = masks.cluster_gaussian_masks(means, dynamic, 0.5, min_samples=2)
    assert calls[-1] == ((22, 3), 0.5, 2)
    assert m.dtype == torch.bool and torch.equal(m, column(["a", "b", "c", "d"]))
    assert torch.equal(masks.cluster_gaussian_masks(means, dynamic[:, None], 0.5, min_samples=2), m)
    # min_samples 1: the loner is a cluster of its own; min_cluster_size drops it and the pair
    assert masks.cluster_gaussian_masks(means, dynamic, 0.5, min_samples=1).shape == (40, 5)
    m = masks.cluster_gaussian_masks(means, dynamic, 0.5, min_samples=1, min_cluster_size=3)
    assert torch.equal(m, column(["a", "b", "c"]))
    # max_clusters: the largest; a tie (a and c, 5 rows each) goes to the lower number; columns stay in cluster order
    assert torch.equal(masks.cluster_gaussian_masks(means, dynamic, 0.5, 2, max_clusters=1), column(["b"]))
    assert torch.equal(masks.cluster_gaussian_masks(means, dynamic, 0.5, 2, max_clusters=2), column(["a", "b"]))
    assert torch.equal(masks.cluster_gaussian_masks(means, dynamic, 0.5, 2, max_clusters=3), column(["a", "b", "c"]))
    assert torch.equal(masks.cluster_gaussian_masks(means, dynamic, 0.5, 2, max_clusters=9), column(["a", "b", "c", "d"]))
    assert torch.equal(masks.cluster_gaussian_masks(means, dynamic, 0.5, 2, 3, max_clusters=1), column(["b"]))
    assert bool(m.any(dim=0).all()) and not bool(m[~dynamic].any())
    # the two refusals, and the malformed calls
    with pytest.raises(ValueError, match="no dynamic"):
        masks.cluster_gaussian_masks(means, torch.zeros(40, dtype=torch.bool), 0.5)
    with pytest.raises(ValueError, match="no cluster survives"):
        masks.cluster_gaussian_masks(means, dynamic, 0.5, min_samples=2, min_cluster_size=10)
    with pytest.raises(ValueError, match="no cluster survives"):
        masks.cluster_gaussian_masks(means, dynamic, 0.5, min_samples=12)  # everything is noise
    for bad in (dynamic[:39], dynamic.float(), dynamic[:, None].expand(40, 2)):
        with pytest.raises(ValueError):
            masks.cluster_gaussian_masks(means, bad, 0.5)
    for kw in ({"min_cluster_size": 0}, {"max_clusters": 0}, {"max_clusters": 1.5}):
        with pytest.raises(ValueError):
            masks.cluster_gaussian_masks(means, dynamic, 0.5, **kw)


def test_entry_points_are_declared_bound_and_limited():
    assert {"fg_dbscan", "fg_dbscan_workspace_bytes"} <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.fg_dbscan_workspace_bytes(0) == 0 and lib.fg_dbscan_workspace_bytes(_lib.DBSCAN_MAX_ROWS + 1) == 0
    a, b = lib.fg_dbscan_workspace_bytes(1000), lib.fg_dbscan_workspace_bytes(_lib.DBSCAN_MAX_ROWS)
    assert 0 < a < b and a % 256 == 0
    # a workspace of no bytes keeps an otherwise valid call on the host
    assert lib.fg_dbscan(1000, 4096, 0.5, 4, 4096, 4096, 4096, 4096, 0, None) == -3
    for n, eps, ms in ((0, 0.5, 4), (_lib.DBSCAN_MAX_ROWS + 1, 0.5, 4), (10, 0.0, 4), (10, float("nan"), 4),
                       (10, float("inf"), 4), (10, 0.5, 0), (10, 0.5, 65536)):  # fmt: skip
        assert lib.fg_dbscan(n, 4096, eps, ms, 4096, 4096, 4096, 4096, 1 << 40, None) == -1
    assert lib.fg_dbscan(10, 4096, 1e-30, 4, 4096, 4096, 4096, 4096, 1 << 40, None) == -4
