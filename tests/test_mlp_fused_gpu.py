"""GPU: the fused fp32 MLP forward (``ops.mlp_forward`` / ``fg_mlp_fwd``) against the reference's recorded outputs, a
float64 run of the same module on the CPU, and itself (row independence and repeatability, bit for bit).

The kernel is called directly, so the sizes are free of the dispatch threshold; only the dispatch tests go through the
modules.  Every output buffer starts as NaN: a row nobody wrote cannot pass.  The float64 runs are made once per
(module, time form) for the largest size; rows are independent, so a smaller size is a prefix of it.

Measured margins (MI355X; helpers records them, profiles/mlp_forward.md has the table): see that file."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from freegaussian_amd import deform as D
from freegaussian_amd import ops
from freegaussian_amd.utils import transform_points
from helpers import REL_TOL, close_except_knife_edge, rel_err
from mlp_common import NAN

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
from make_golden import fill_params  # noqa: E402  (pure helper)

DEV = "cuda"
M = ops.MLP_ROW_TILE
SIZES = [1, M - 1, M, M + 1, 2 * M + 3, 1000, 33_000]
N_MAX = max(SIZES)


def _gold(k):
    return torch.from_numpy(np.load(os.path.join(GOLD, "g_mlp.npz"))[k])


def _deform(weights="fill", **kw):
    torch.manual_seed(0)
    m = D.FreeGaussianDeformableModel(**kw)
    if weights == "fill":
        fill_params(m)
    return m.requires_grad_(False)


def _control(weights="fill"):
    torch.manual_seed(0)
    m = D.FreeGaussianControllableModel()
    if weights == "fill":
        fill_params(m)
    return m.requires_grad_(False)


def _heads(m):
    if isinstance(m, D.FreeGaussianControllableModel):
        return (m.d_xyz, m.d_rot, m.d_scale)
    return (m.branch_w, m.branch_v, m.gaussian_rotation, m.gaussian_scaling)


def _aux(m, other):
    """What the module's own fused path hands the kernel as `aux` (torch, tiny)."""
    with torch.no_grad():
        if isinstance(m, D.FreeGaussianControllableModel):
            return D.positional_encoding(other, m.multires)
        a = D.positional_encoding(other, m.t_multires)
        return m.timenet(a) if m.is_blender else a


def _nan(n, *shape):
    return torch.full((n, *shape), NAN, device=DEV)


def _fused(m_dev, x, other, outs=None):
    """ops.mlp_forward on the module `m_dev` (already on the device) into NaN-filled buffers."""
    control = isinstance(m_dev, D.FreeGaussianControllableModel)
    n = x.shape[0]
    if outs is None:
        outs = [_nan(n, 3), _nan(n, 4), _nan(n, 3)] if control else [_nan(n, 4, 4), _nan(n, 4), _nan(n, 3), _nan(n, 3)]
    return ops.mlp_forward(x.to(DEV), _aux(m_dev, other.to(DEV)), m_dev.linear, _heads(m_dev),
                           mode="plain" if control else "se3", outs=outs)  # fmt: skip


def _float64(m, x, other):
    """The same module in float64 on the CPU; for the deformation net with the transformed points appended."""
    m64 = copy.deepcopy(m).cpu().double()
    with torch.no_grad():
        out = m64(x.cpu().double(), other.cpu().double())
        if isinstance(m, D.FreeGaussianDeformableModel):
            out = (*out, transform_points(out[0], x.cpu().double()))
    return out


def _inputs(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g) * 2 - 1
    t = torch.rand(n, 1, generator=g)
    return x, t


# ---- 1. the reference's own outputs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,kw", [("deform", {}), ("deform_blender", {"is_blender": True})])
def test_deform_matches_the_reference_outputs(tag, kw):
    m = _deform(**kw).to(DEV)
    x = _gold("x")
    for ti, tt in enumerate((0.0, 0.5, 1.0)):
        for t in (torch.full((16, 1), tt), torch.full((1, 1), tt).expand(16, -1)):  # per-row and broadcast
            d_xyz, rot, scale, pts = _fused(m, x, t)
            assert rel_err(d_xyz, _gold(f"{tag}.t{ti}.d_xyz")) < REL_TOL
            assert rel_err(rot, _gold(f"{tag}.t{ti}.rot")) < REL_TOL
            assert rel_err(scale, _gold(f"{tag}.t{ti}.scale")) < REL_TOL
            assert rel_err(pts, transform_points(_gold(f"{tag}.t{ti}.d_xyz"), x)) < REL_TOL


def test_control_matches_the_reference_outputs():
    m = _control().to(DEV)
    d_xyz, rot, scale = _fused(m, _gold("x"), _gold("control.value"))
    assert rel_err(d_xyz, _gold("control.d_xyz")) < REL_TOL
    assert rel_err(rot, _gold("control.rot")) < REL_TOL
    assert rel_err(scale, _gold("control.scale")) < REL_TOL


# ---- 2. float64 arbiter across tile edges ---------------------------------------------------------------------------
_REF = {}


def _arbiter(weights, form):
    """(module on the device, x, t, float64 outputs) for N_MAX rows; `form`: "rows" = a time per row, "one" = one time
    for all (the stride-0 tensor the model passes)."""
    key = (weights, form)
    if key not in _REF:
        m = _deform(weights)
        x, t = _inputs(N_MAX)
        if form == "one":
            t = torch.full((1, 1), 0.37).expand(N_MAX, -1)
        _REF[key] = (m.to(DEV), x, t, _float64(m, x, t))
    return _REF[key]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", ["rows", "one"])
@pytest.mark.parametrize("weights", ["fill", "default"])
def test_float64_arbiter_across_tile_edges(weights, form, n):
    m, x, t, want = _arbiter(weights, form)
    got = _fused(m, x[:n], t[:n])
    assert form == "rows" or n == 1 or t[:n].stride(0) == 0
    for name, g, w in zip(("d_xyz", "d_rot", "d_scale", "pts"), got, want):
        assert bool(torch.isfinite(g).all()), name
        err = rel_err(g, w[:n])
        print(f"mlp_fused {weights} {form} n={n} {name}: rel_err {err:.3e}")
        assert err < REL_TOL, name


@pytest.mark.parametrize("kind", ["deform_blender", "control"])
def test_float64_arbiter_other_networks(kind):
    """The 30-wide time net input (A = 30) and the control net (A = 63, plain heads), default init and fill_params."""
    n = 2 * M + 3
    for weights in ("fill", "default"):
        m = _control(weights) if kind == "control" else _deform(weights, is_blender=True)
        x, t = _inputs(n, seed=2)
        other = (torch.randn(n, 3, generator=torch.Generator().manual_seed(4)) * 0.1) if kind == "control" else t
        want = _float64(m, x, other)
        got = _fused(m.to(DEV), x, other)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert rel_err(g, w) < REL_TOL


# ---- 3. row independence, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["fill", "default"])
def test_rows_are_independent_and_runs_repeat_bitwise(weights):
    """Each output element is one fixed fmaf chain over its own row: a row's result cannot depend on the tile it lands in,
    its place in the tile, the rows beside it or the pad rows of the last tile."""
    m = _deform(weights).to(DEV)
    n = 2 * M + 3
    x, t = _inputs(n, seed=5)
    a = _fused(m, x, t)
    b = _fused(m, x, t)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(6))
    c = _fused(m, x[perm], t[perm])
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v)
        assert torch.equal(u[perm.to(DEV)], w)
    # ... nor on how many rows follow it
    d = _fused(m, x[: M + 1], t[: M + 1])
    for u, w in zip(a, d):
        assert torch.equal(u[: M + 1], w)


# ---- 4. structure ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zeroed", ["input_columns", "hidden_columns"])
def test_skip_layer_halves_against_float64(zeroed):
    """Layer 5 multiplies [inp, h]: with its input columns zeroed the re-injected row is irrelevant, with its hidden
    columns zeroed nothing but the re-injected row reaches the layers behind it."""
    m = _deform("default")
    in_ch = m.input_ch
    with torch.no_grad():
        if zeroed == "input_columns":
            m.linear[5].weight[:, :in_ch] = 0.0
        else:
            m.linear[5].weight[:, in_ch:] = 0.0
    n = M + 5
    x, t = _inputs(n, seed=7)
    want = _float64(m, x, t)
    got = _fused(m.to(DEV), x, t)
    for g, w in zip(got, want):
        assert rel_err(g, w) < REL_TOL


def test_relu_at_zero_and_below():
    """Pre-activations that are exactly 0 (zero weights, zero bias) and negative for every row (zero weights, bias -1) in a
    middle layer; the columns behind them must see exact zeros."""
    m = _deform("default")
    with torch.no_grad():
        m.linear[3].weight[:64] = 0.0
        m.linear[3].bias[:64] = 0.0
        m.linear[3].weight[64:128] = 0.0
        m.linear[3].bias[64:128] = -1.0
        m.linear[0].weight[::2] = -m.linear[0].weight[::2].abs()  # many negative pre-activations in the first layer too
    n = M + 5
    x, t = _inputs(n, seed=8)
    want = _float64(m, x, t)
    got = _fused(m.to(DEV), x, t)
    for g, w in zip(got, want):
        assert bool(torch.isfinite(g).all()) and rel_err(g, w) < REL_TOL
    # the dead columns carry nothing: whatever layer 4 holds for them changes no output bit
    m2 = copy.deepcopy(m)
    with torch.no_grad():
        m2.linear[4].weight[:, :128] = 7.0
    for g, g2 in zip(got, _fused(m2.to(DEV), x, t)):
        assert torch.equal(g, g2)


def test_null_outputs_are_left_alone_and_bottom_row_is_exact():
    m = _deform("fill").to(DEV)
    n = 2 * M + 3
    x, t = _inputs(n, seed=9)
    full = _fused(m, x, t)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], device=DEV).expand(n, 4)
    assert torch.equal(full[0][:, 3], bottom)
    # all four arrays carved out of one NaN arena with guard bands: a store outside what was asked for shows up
    widths, gap = (16, 4, 3, 3), 64
    for skip in (0, 3):  # no d_xyz but pts; d_xyz but no pts
        arena = torch.full((gap + sum(n * w + gap for w in widths),), NAN, device=DEV)
        views, spans, at = [], [], gap
        for w in widths:
            views.append(arena[at : at + n * w].view((n, 4, 4) if w == 16 else (n, w)))
            spans.append((at, at + n * w))
            at += n * w + gap
        outs = [False if i == skip else v for i, v in enumerate(views)]
        got = ops.mlp_forward(x.to(DEV), _aux(m, t.to(DEV)), m.linear, _heads(m), mode="se3", outs=outs)
        written = torch.zeros_like(arena, dtype=torch.bool)
        for i, (a, b) in enumerate(spans):
            if i != skip:
                written[a:b] = True
        assert got[skip] is None
        assert bool(torch.isnan(arena[~written]).all()) and bool(torch.isfinite(arena[written]).all())
        for i in range(4):
            if i != skip:
                assert torch.equal(got[i], full[i])


# ---- 5. dispatch ----------------------------------------------------------------------------------------------------
@pytest.fixture
def recorder(monkeypatch):
    calls = []
    real = ops.mlp_forward

    def spy(*a, **k):
        calls.append((a, k))
        return real(*a, **k)

    monkeypatch.setattr(ops, "mlp_forward", spy)
    return calls


def test_module_dispatch(recorder, monkeypatch):
    monkeypatch.setenv("FG_FUSED_MLP", "1")
    torch.manual_seed(0)
    m = D.FreeGaussianDeformableModel().to(DEV)
    n = max(33_000, D.FUSED_MIN_ROWS)
    x, _ = _inputs(n, seed=10)
    x = x.to(DEV)
    t = torch.full((1, 1), 0.3, device=DEV).expand(n, -1)
    with torch.no_grad():
        fused = m(x, t)
    assert len(recorder) == 1 and len(fused) == 3 and fused[0].shape == (n, 4, 4)
    assert recorder[0][0][1].shape == (1, 21)  # the broadcast time: encoded on one row
    plain = m(x, t)  # grad mode on, parameters want gradients: the torch path, untouched
    assert len(recorder) == 1 and plain[0].requires_grad
    for a, b in zip(fused, plain):
        assert rel_err(a, b) < REL_TOL
    with torch.no_grad():
        small = m(x[: D.FUSED_MIN_ROWS - 1], t[: D.FUSED_MIN_ROWS - 1])  # below the threshold
        assert len(recorder) == 1 and small[0].shape[0] == D.FUSED_MIN_ROWS - 1
        monkeypatch.setenv("FG_FUSED_MLP", "0")
        off = m(x, t)
    assert len(recorder) == 1
    for a, b in zip(off, plain):
        assert rel_err(a, b) < 1e-6  # (the same torch ops with and without a tape)
    # parameters that want no gradient: the fused path with grad mode on as well
    monkeypatch.setenv("FG_FUSED_MLP", "1")
    m.requires_grad_(False)
    m(x, t)
    assert len(recorder) == 2
    # a shape of `other` the kernel is not built for: the torch ops, not an error
    assert not D.fused_applies(m, x, torch.zeros(n, 3, device=DEV)) and not D.fused_applies(m, x, t[: n - 1])
    # the variable unset: what deform.FUSED_DEFAULT says
    monkeypatch.delenv("FG_FUSED_MLP")
    assert D.fused_applies(m, x, t) == (D.FUSED_DEFAULT != "0")
    monkeypatch.setenv("FG_FUSED_MLP", "1")
    c = D.FreeGaussianControllableModel().to(DEV)
    with torch.no_grad():
        got = c(x, torch.zeros(n, 3, device=DEV))
    assert len(recorder) == 3 and [tuple(g.shape) for g in got] == [(n, 3), (n, 4), (n, 3)]


def test_render_is_the_same_with_the_knob_on_and_off(recorder, monkeypatch):
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    n, W, H = 33_000, 64, 48
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-3.8)
    with torch.no_grad():
        model.gauss_params["scales"].normal_(-3.8, 0.3)
        model.gauss_params["features_rest"].normal_(0, 0.1)
        for q in model.deform.parameters():
            q.mul_(0.3)
    model.step = 4000
    model = model.to(DEV).eval()
    w2c = look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3))
    c2w = torch.linalg.inv(w2c)
    c2w[:3, 1:3] *= -1
    cam = Camera(c2w[None, :3], 56.0, 60.0, W / 2, H / 2, W, H, times=torch.tensor([[0.4]]))
    monkeypatch.setenv("FG_FUSED_MLP", "1")
    on = model.get_outputs_for_camera(cam)
    assert len(recorder) == 1 and recorder[0][1]["outs"][0] is False  # no [N,4,4] transforms: the points directly
    monkeypatch.setenv("FG_FUSED_MLP", "0")
    off = model.get_outputs_for_camera(cam)
    assert len(recorder) == 1
    assert on["rgb"].shape == (H, W, 3) and float(off["rgb"].std()) > 1e-3
    assert close_except_knife_edge(on["rgb"], off["rgb"], REL_TOL)


# ---- 6. graph capture -----------------------------------------------------------------------------------------------
def test_capture_and_replay_equal_the_eager_call():
    m = _deform("fill").to(DEV)
    n = 2 * M + 3
    x, t = _inputs(n, seed=11)
    x, aux = x.to(DEV), _aux(m, t.to(DEV))
    eager = ops.mlp_forward(x, aux, m.linear, _heads(m))
    torch.cuda.synchronize()
    outs = [_nan(n, 4, 4), _nan(n, 4), _nan(n, 3), _nan(n, 3)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.mlp_forward(x, aux, m.linear, _heads(m), outs=outs)
    for _ in range(2):
        for o in outs:
            o.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, eager):
            assert torch.equal(o, e)
