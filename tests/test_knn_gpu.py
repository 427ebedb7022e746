"""GPU checks of the neighbour search (``ops.knn`` / ``fg_knn``): bit for bit against the brute-force restatement where
a CPU can afford one, against a float64 brute force ON THE DEVICE for sampled and worst-case queries where it cannot, and
the wiring into ``knn_mean_distance`` and the model constructor.

rtol 1e-6 of the distance comparisons: the fp32 chain subtract, square, two adds, square root and the three-term mean
carries at most 6.5 roundings of 2^-24 (all terms are non-negative), about 3.9e-7."""
import pytest
import torch

from freegaussian_amd import ops, utils
from freegaussian_amd.model import FreeGaussianModel, FreeGaussianModelConfig
from freegaussian_amd.scenes import room_scene
from knn_restatement import knn_restatement

pytestmark = pytest.mark.gpu

RTOL = 1e-6


def _uniform(n, seed=0):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * 10


def _clustered(n, seed=0):
    x = _uniform(n, seed)
    x[: (4 * n) // 5] *= 0.2  # 80 % of the points scaled by 0.2 about the origin
    return x


def _room(n):
    return room_scene(n, 320, 180)[0].means.detach().float().contiguous()


def _sheet(n, seed=0):
    return _uniform(n, seed) * torch.tensor([1.0, 1.0, 1e-4])  # z extent 1e-3


SETS_50K = {"uniform": lambda: _uniform(50_000), "clustered": lambda: _clustered(50_000), "room": lambda: _room(50_000),
            "sheet": lambda: _sheet(50_000)}  # fmt: skip
_restated = {}


def _set_50k(name):
    if name not in _restated:
        x = SETS_50K[name]()
        _restated[name] = (x, *knn_restatement(x, 8))  # (the k best of 8 are its first k columns)
    return _restated[name]


def _assert_exact(x, k, want=None):
    d2, idx = ops.knn(x.cuda(), k, squared=True)
    assert d2.shape == (x.shape[0], k) and d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.is_cuda and idx.is_cuda
    want_d2, want_idx = want if want is not None else knn_restatement(x, k)
    bad = int((idx.cpu() != want_idx[:, :k]).any(dim=1).sum())
    print(f"n={x.shape[0]} k={k}: {bad} rows differ in idx")
    assert torch.equal(idx.cpu(), want_idx[:, :k])
    assert torch.equal(d2.cpu(), want_d2[:, :k])
    return d2, idx


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("name", list(SETS_50K))
def test_bit_exact_at_50k(name, k):
    x, want_d2, want_idx = _set_50k(name)
    _assert_exact(x, k, (want_d2, want_idx))


def test_degenerate_inputs_exact():
    g = torch.Generator().manual_seed(11)
    same = torch.full((1500, 3), 0.37)
    for k in (1, 3, 8):
        d2, _ = _assert_exact(same, k)
        assert float(d2.abs().max()) == 0.0
    base = torch.rand(1000, 3, generator=g) * 6 - 3
    rep = base.repeat(4, 1)[torch.randperm(4000, generator=g)]
    d2, _ = _assert_exact(rep, 3)
    assert float(d2.abs().max()) == 0.0  # three other copies of every point
    _assert_exact(rep, 8)
    t = torch.rand(4096, 1, generator=g)
    for line in (t * torch.tensor([[1.0, 0.0, 0.0]]) + 2.0,  # along an axis: two axes of zero extent
                 t * torch.tensor([[3.0, -2.0, 0.5]]) + torch.tensor([[1.0, 5.0, -4.0]]),
                 torch.linspace(0, 1, 4096)[:, None] * torch.tensor([[1.0, 1.0, 1.0]])):  # evenly spaced: ties everywhere
        for k in (1, 3, 8):
            _assert_exact(line, k)
    for k in range(1, 9):  # N = k + 1
        _assert_exact(torch.rand(k + 1, 3, generator=g), k)
    _assert_exact(torch.rand(300, 3, generator=g) * torch.tensor([1.0, 0.0, 1.0]), 5)  # a plane of zero thickness


def test_fewer_points_than_neighbours_and_bad_input():
    g = torch.Generator().manual_seed(12)
    x = torch.rand(5, 3, generator=g)
    assert torch.equal(utils.knn_mean_distance(x[:1].cuda()).cpu(), torch.ones(1, 1))
    two = utils.knn_mean_distance(x[:2].cuda())
    assert two.is_cuda and torch.allclose(two.cpu(), (x[0] - x[1]).norm().reshape(1, 1).expand(2, 1))
    d, idx = ops.knn(x[:3].cuda(), 8)
    assert d.shape == (3, 2) and idx.shape == (3, 2)
    d, idx = ops.knn(x[:1].cuda(), 3)
    assert d.shape == (1, 0) and idx.shape == (1, 0) and d.is_cuda
    assert ops.knn(x[:0].cuda(), 3)[0].shape == (0, 0)
    for bad in (float("nan"), float("inf"), -float("inf")):
        y = x.clone()
        y[3, 1] = bad
        with pytest.raises(ValueError):
            ops.knn(y.cuda(), 3)
        with pytest.raises(ValueError):
            utils.knn_mean_distance(y.cuda())
    for k in (0, 9, -1):
        with pytest.raises(ValueError):
            ops.knn(x.cuda(), k)
    for shape in ((5, 2), (5, 4), (15,), (1, 5, 3)):
        with pytest.raises(ValueError):
            ops.knn(torch.zeros(shape).cuda(), 3)


def _check_queries_float64(x_dev, d, queries, label):
    """Rows ``queries`` of the returned distances d [N,k] against a float64 brute force over all N, on the device."""
    k = d.shape[1]
    x64 = x_dev.double()
    worst = 0.0
    for i in range(0, queries.numel(), 256):
        q = queries[i : i + 256]
        dd = ((x64[q][:, None, :] - x64[None, :, :]) ** 2).sum(-1)
        dd[torch.arange(q.numel(), device=q.device), q] = float("inf")
        want = dd.topk(k, dim=1, largest=False).values.sqrt()
        got = d[q].double()
        err = ((got - want).abs() / want.clamp_min(1e-300)).masked_fill(want == got, 0.0)
        worst = max(worst, float(err.max()))
    print(f"{label}: {queries.numel()} queries, worst relative distance error {worst:.3e}")
    assert worst <= RTOL, f"{label}: {worst}"


def _sample_and_worst(d, seed):
    n = d.shape[0]
    sample = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:4096].to(d.device)
    worst = d[:, -1].topk(64).indices  # the longest searches: the ring growth's worst case
    return torch.cat([sample, worst])


def test_outliers_do_not_break_the_grid():
    n = 200_000
    x = _uniform(n, seed=21)
    out = torch.randperm(n, generator=torch.Generator().manual_seed(22))[: n // 100]
    x[out] = (x[out] - 5.0) * 1000.0  # 1 % of the points at 1000 x the extent
    xd = x.cuda()
    d, idx = ops.knn(xd, 3)
    assert bool(torch.isfinite(d).all()) and bool((idx >= 0).all()) and bool((idx < n).all())
    _check_queries_float64(xd, d, torch.cat([_sample_and_worst(d, 23), out.to(d.device)]).unique(), "outliers")


@pytest.mark.parametrize("name", ["uniform", "clustered"])
def test_one_million_points_sampled_against_float64_on_the_device(name):
    n = 1_000_000
    xd = (_uniform(n, seed=31) if name == "uniform" else _clustered(n, seed=32)).cuda()
    d, idx = ops.knn(xd, 3)
    assert bool(torch.isfinite(d).all()) and bool((d[:, 1:] >= d[:, :-1]).all())
    assert bool((idx.long() != torch.arange(n, device=idx.device)[:, None]).all())
    _check_queries_float64(xd, d, _sample_and_worst(d, 33), f"1M {name}")
    d8, _ = ops.knn(xd, 8)
    assert torch.equal(d8[:, :3], d)
    _check_queries_float64(xd, d8, _sample_and_worst(d8, 34)[::8], f"1M {name} k=8")


@pytest.mark.parametrize("name", list(SETS_50K))
def test_knn_mean_distance_on_the_device(name):
    x = _set_50k(name)[0]
    got = utils.knn_mean_distance(x.cuda())
    want = utils.knn_mean_distance(x)
    assert got.is_cuda and got.shape == (x.shape[0], 1) and want.device.type == "cpu"
    err = float(((got.cpu() - want).abs() / want).max())
    print(f"{name}: knn_mean_distance device vs host, worst relative difference {err:.3e}")
    assert torch.allclose(got.cpu(), want, rtol=RTOL, atol=0)


def test_model_constructor_on_the_device():
    cfg = FreeGaussianModelConfig()
    torch.manual_seed(5)
    host = FreeGaussianModel(cfg, num_points=20_000)
    torch.manual_seed(5)
    dev = FreeGaussianModel(cfg, num_points=20_000, device="cuda")
    assert all(p.is_cuda for p in dev.parameters()) and not any(p.is_cuda for p in host.parameters())
    assert torch.equal(dev.gauss_params["means"].detach().cpu(), host.gauss_params["means"].detach())
    assert torch.allclose(dev.gauss_params["scales"].detach().cpu(), host.gauss_params["scales"].detach(), atol=1e-5)
    for name in ("quats", "features_dc", "features_rest", "opacities"):
        assert torch.equal(dev.gauss_params[name].detach().cpu(), host.gauss_params[name].detach())
    seeded = FreeGaussianModel(cfg, seed_points=host.gauss_params["means"].detach().cuda())
    assert {p.device for p in seeded.parameters()} == {dev.gauss_params["means"].device}
    assert torch.equal(seeded.gauss_params["scales"].detach(), dev.gauss_params["scales"].detach())
    fixed = FreeGaussianModel(cfg, num_points=64, init_scales=-4.0, device="cuda")
    assert all(p.is_cuda for p in fixed.parameters()) and float(fixed.gauss_params["scales"].max()) == -4.0


def test_two_calls_give_the_same_bits():
    x = _clustered(300_000, seed=41).cuda()
    a = ops.knn(x, 3, squared=True)
    b = ops.knn(x, 3, squared=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = ops.knn(x, 8)
    e = ops.knn(x, 8)
    assert torch.equal(c[0], e[0]) and torch.equal(c[1], e[1])
