"""CPU checks of the neighbour search's host side: the C ABI's argument validation, the brute-force restatement the GPU
tests compare against, and the CPU paths of ``utils.knn_mean_distance``."""
import builtins
import warnings

import pytest
import torch

from freegaussian_amd import _lib, utils
from knn_restatement import knn_restatement


def test_workspace_query_and_argument_validation_without_gpu():
    lib = _lib.load()
    sizes = [int(lib.fg_knn_workspace_bytes(n)) for n in (0, 10, 1000, 100_000, 1_000_000, 5_000_000)]
    assert sizes == sorted(sizes) and len(set(sizes[1:])) == len(sizes) - 1
    for n, b in zip((10, 1000, 100_000, 1_000_000, 5_000_000), sizes[1:]):
        assert b >= n * 8  # the keys and the values alone
    assert lib.fg_knn(0, None, 3, None, None, None, 0, None) == 0  # nothing to do
    big = 1 << 40  # (no buffer is touched: every call below is rejected before a launch)
    bad = -1
    assert lib.fg_knn(100, None, 0, None, None, None, big, None) == bad  # k < 1
    assert lib.fg_knn(100, None, _lib.KNN_MAX_K + 1, None, None, None, big, None) == bad  # k > FG_KNN_MAX_K
    assert lib.fg_knn(3, None, 3, None, None, None, big, None) == bad  # n <= k
    assert lib.fg_knn(2, None, 3, None, None, None, big, None) == bad
    assert lib.fg_knn(1 << 31, None, 3, None, None, None, big, None) == bad  # n >= 2^31
    assert lib.fg_knn(-5, None, 3, None, None, None, big, None) == bad
    # a workspace that is too small: rejected although every pointer is set
    buf = torch.zeros(4096, dtype=torch.float32)
    p = buf.data_ptr()
    need = int(lib.fg_knn_workspace_bytes(100))
    assert lib.fg_knn(100, p, 3, p, p, p, need - 1, None) == bad
    assert lib.fg_knn(100, None, 3, None, None, None, need, None) == bad  # buffers missing
    assert _lib.KNN_MAX_K == 8


def test_restatement_against_float64():
    g = torch.Generator().manual_seed(3)
    n, k = 3000, 8
    x = torch.rand(n, 3, generator=g) * 10
    d2, idx = knn_restatement(x, k)
    d64 = torch.cdist(x.double(), x.double())
    d64.fill_diagonal_(float("inf"))
    want_d, want_i = d64.topk(k, dim=1, largest=False)
    assert torch.allclose(d2.double().sqrt(), want_d, rtol=1e-6, atol=0)
    # indices wherever float64 tells the neighbour apart from the ones before and after it
    wide = d64.topk(k + 1, dim=1, largest=False).values
    gap_after = (wide[:, 1:] - wide[:, :-1]) > 1e-5 * wide[:, 1:]
    gap_before = torch.cat([torch.ones(n, 1, dtype=torch.bool), gap_after[:, :-1]], dim=1)
    clear = gap_after & gap_before
    assert clear.float().mean() > 0.99
    assert torch.equal(idx.long()[clear], want_i[clear])
    # ascending, self excluded, ties by row number
    assert bool((d2[:, 1:] >= d2[:, :-1]).all()) and bool((idx.long() != torch.arange(n)[:, None]).all())
    y = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0], [-1.0, 0, 0], [0.0, 0, 0]])
    d2, idx = knn_restatement(y, 3)
    assert idx.tolist() == [[2, 4, 1], [0, 2, 4], [0, 4, 1], [0, 2, 4], [0, 2, 1]]
    assert d2.tolist() == [[0, 0, 1], [1, 1, 1], [0, 0, 1], [1, 1, 1], [0, 0, 1]]


def test_cpu_input_takes_the_tree_query_unchanged():
    """A CPU tensor: the reference's own query (sklearn, k + 1 neighbours, the point dropped), value for value."""
    nn = pytest.importorskip("sklearn.neighbors")
    g = torch.Generator().manual_seed(5)
    x = torch.rand(4000, 3, generator=g) * 4 - 2
    got = utils.knn_mean_distance(x, 3)
    d, _ = nn.NearestNeighbors(n_neighbors=4, algorithm="auto", metric="euclidean").fit(x.numpy()).kneighbors(x.numpy())
    want = torch.from_numpy(d[:, 1:].astype("float32")).mean(dim=-1, keepdim=True)
    assert got.device.type == "cpu" and got.shape == (4000, 1) and torch.equal(got, want)
    assert torch.equal(utils.knn_mean_distance(x[:1]), torch.ones(1, 1))
    assert utils.knn_mean_distance(x[:0]).shape == (0, 1)


@pytest.fixture
def no_sklearn(monkeypatch):
    real = builtins.__import__

    def blocked(name, *a, **kw):
        if name.split(".")[0] == "sklearn":
            raise ImportError("sklearn blocked by the test")
        return real(name, *a, **kw)

    monkeypatch.setattr(builtins, "__import__", blocked)


def test_bounded_fallback_without_sklearn(no_sklearn, monkeypatch):
    g = torch.Generator().manual_seed(7)
    n = 5000
    x = torch.rand(n, 3, generator=g) * 10
    shapes = []
    real_cdist = torch.cdist

    def spy(a, b, *args, **kw):
        shapes.append((a.shape[0], b.shape[0]))
        return real_cdist(a, b, *args, **kw)

    monkeypatch.setattr(torch, "cdist", spy)
    monkeypatch.setattr(utils, "KNN_FALLBACK_CHUNK_BYTES", 1 << 20)  # 1 MiB: 52 rows of 5000 floats
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no warning at this size
        got = utils.knn_mean_distance(x, 3)
    assert shapes and sum(r for r, _ in shapes) == n
    assert all(r * c * 4 <= 1 << 20 and c == n for r, c in shapes) and max(r for r, _ in shapes) == 52
    d2, _ = knn_restatement(x, 3)
    want = d2.sqrt().mean(dim=1, keepdim=True)
    assert torch.allclose(got, want, rtol=1e-6, atol=0)
    # the default budget: the 2048 rows it always used while they fit, 16 rows at 1M points, never above the budget
    monkeypatch.undo()
    assert utils.knn_fallback_rows(5000) == 2048 and utils.knn_fallback_rows(1_000_000) == 16
    for m in (1, 100, 8191, 8193, 10**6, 10**8):
        assert utils.knn_fallback_rows(m) >= 1
        assert utils.knn_fallback_rows(m) * m * 4 <= max(utils.KNN_FALLBACK_CHUNK_BYTES, 4 * m)


def test_fallback_warns_above_100k_points(no_sklearn, monkeypatch):
    monkeypatch.setattr(torch, "cdist", lambda a, b, *args, **kw: torch.zeros(a.shape[0], b.shape[0]))  # (not the point here)
    x = torch.zeros(100_001, 3)
    with pytest.warns(RuntimeWarning, match="scikit-learn"):
        utils.knn_mean_distance(x, 3)
