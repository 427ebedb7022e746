"""GPU: the opt-in split-bf16 mode of the fused MLP calls (``precision="bf16x3"`` / ``FG_MLP_BF16X3``; the contract is in
include/fgraster.h) against float64 at the project's one bar (``helpers.REL_TOL`` = 1e-4 of each array's largest magnitude),
against itself (repeatability, row independence, graph replay: bit for bit), on guarded buffers, and through the modules
and the model with ``FG_FUSED_MLP_PRECISION=bf16x3``.

Rows come from tests/mlp_split_common.py: 1024 rows clear of the ReLU's kink by 1e-4 of the layer's largest pre-activation
out of 4096 candidates (the split moves a pre-activation by about 5e-6 of that; a row nearer to zero may take the other
branch, and its gradient is then another one).  One float64 reference per network, computed once and never changed; rows
are independent, so a smaller size is a prefix of it.  Every output buffer starts as NaN.

Every test here that passes ``precision=`` fails without the feature (``TypeError``).  Measured: profiles/mlp_split_bf16.md."""
import copy
import ctypes

import pytest
import torch

from freegaussian_amd import _lib
from freegaussian_amd import deform as D
from freegaussian_amd import ops
from helpers import REL_TOL, rel_err
from mlp_common import GUARD, NAN, arena, train_step
from mlp_split_common import ROWS, case
from mlp_train_common import head_rows, heads_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
M = ops.MLP_ROW_TILE
SPLIT = "bf16x3"
NETS = [("deform", "default"), ("deform", "half_dead"), ("control", "default"), ("control", "half_dead"),
        ("blender", "default"), ("blender", "half_dead")]  # fmt: skip

_DEV = {}


def _on_device(kind, weights="default"):
    """(case, the case's module on the device, x, aux, g_heads on the device): made once, never changed."""
    key = (kind, weights)
    if key not in _DEV:
        c = case(kind, weights)
        _DEV[key] = (c, copy.deepcopy(c["m"]).to(DEV), c["x"].to(DEV), c["aux"].to(DEV), c["g_heads"].to(DEV))
    return _DEV[key]


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _mode(m):
    return "plain" if isinstance(m, D.FreeGaussianControllableModel) or not hasattr(m, "is_blender") else "se3"


def _forward(m_dev, x, aux, precision=SPLIT, outs=None):
    n, mode = x.shape[0], _mode(m_dev)
    if outs is None:
        outs = [_nan(n, r) for r in head_rows(m_dev)] if mode == "plain" else [_nan(n, 4, 4), _nan(n, 4), _nan(n, 3), _nan(n, 3)]
    return ops.mlp_forward(x, aux, m_dev.linear, heads_of(m_dev), mode=mode, outs=outs, precision=precision)


def _train_fwd(m_dev, x, aux, precision=_lib.MLP_BF16X3, bufs=None, ws=None):
    """``fg_mlp_train_fwd`` itself: (raw heads, enc, H) into NaN-filled buffers (or the ones given)."""
    n, A = x.shape[0], aux.shape[1]
    d, _, rows, keep = ops._mlp_desc("test", x, aux, m_dev.linear, heads_of(m_dev), _lib.MLP_PLAIN)
    d.precision = precision
    raw, enc, H = bufs or (_nan(n, sum(rows)), _nan(n, _lib.mlp_enc_width(A)), _nan(8, n, 256))
    if ws is None:
        ws = torch.empty(int(_lib.load().fg_mlp_train_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
    ops._call("fg_mlp_train_fwd", n, ctypes.addressof(d), raw.data_ptr(), enc.data_ptr(), H.data_ptr(), ws.data_ptr(),
              ws.numel() * ws.element_size(), ops._stream())  # fmt: skip
    return raw, enc, H


def _bwd(m_dev, A, H, g_heads, inputs, precision=_lib.MLP_BF16X3, bufs=None, ws=None):
    """``fg_mlp_bwd_inputs`` (``inputs``) or ``fg_mlp_bwd`` itself: (G, g_enc or None)."""
    n = H.shape[1]
    d, _, _, keep = ops._mlp_desc("test", None, A, m_dev.linear, heads_of(m_dev), _lib.MLP_PLAIN)
    d.precision = precision
    G, ge = bufs or (_nan(8, n, 256), _nan(n, _lib.mlp_enc_width(A)) if inputs else None)
    lib = _lib.load()
    if ws is None:
        need = lib.fg_mlp_bwd_inputs_workspace_bytes(n) if inputs else lib.fg_mlp_train_workspace_bytes(n)
        ws = torch.empty(int(need), dtype=torch.uint8, device=DEV)
    nbytes = ws.numel() * ws.element_size()
    if inputs:
        ops._call("fg_mlp_bwd_inputs", n, ctypes.addressof(d), g_heads.data_ptr(), H.data_ptr(), G.data_ptr(), ge.data_ptr(),
                  ws.data_ptr(), nbytes, ops._stream())  # fmt: skip
    else:
        ops._call("fg_mlp_bwd", n, ctypes.addressof(d), g_heads.data_ptr(), H.data_ptr(), G.data_ptr(), ws.data_ptr(), nbytes, ops._stream())
    return G, ge


def _check(tag, errs):
    print(f"mlp_split {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= REL_TOL, (tag, k, v)


# ---- 1. the forward against float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,weights", NETS)
def test_forward_against_float64(kind, weights):
    c, m, x, aux, _ = _on_device(kind, weights)
    names = ("d_xyz", "d_rot", "d_scale") if kind == "control" else ("d_xyz", "d_rot", "d_scale", "pts")
    for n in (1, M - 1, M + 1, 200, ROWS):
        got = _forward(m, x[:n].contiguous(), aux[:n].contiguous())
        assert all(bool(torch.isfinite(g).all()) for g in got)
        _check(f"forward {kind} {weights} n={n}", {k: rel_err(g, w[:n]) for k, g, w in zip(names, got, c["ref"]["outs"])})
    # the mode is taken: not the fp32 call's bits
    split, exact = _forward(m, x[:200].contiguous(), aux[:200].contiguous()), _forward(m, x[:200].contiguous(), aux[:200].contiguous(), "fp32")
    assert not any(torch.equal(a, b) for a, b in zip(split, exact))
    _check(f"forward {kind} {weights} n=200 fp32", {k: rel_err(g, w[:200]) for k, g, w in zip(names, exact, c["ref"]["outs"])})


# ---- 2. the training forward and the backwards against float64 -------------------------------------------------------------
@pytest.mark.parametrize("kind,weights", [("deform", "default"), ("deform", "half_dead"), ("control", "default"), ("blender", "default")])
def test_training_arrays_against_float64(kind, weights):
    """``heads``, ``enc``, ``acts`` of ``fg_mlp_train_fwd`` and ``g_pre``, ``g_enc`` of both backward calls, as the calls store them."""
    c, m, x, aux, gh = _on_device(kind, weights)
    ref, A, in_ch = c["ref"], aux.shape[1], 63 + aux.shape[1]
    raw, enc, H = _train_fwd(m, x, aux)
    G, ge = _bwd(m, A, H, gh, inputs=True)
    G2, _ = _bwd(m, A, H, gh, inputs=False)
    assert torch.equal(G, G2)  # the same chain with and without the input-row products
    assert torch.equal(raw, torch.cat(ops.mlp_forward(x, aux, m.linear, heads_of(m), mode="plain", precision=SPLIT), dim=1))
    assert bool((ge[:, in_ch:] == 0).all()) and bool((enc[:, in_ch:] == 0).all())
    # enc is the fp32 call's, bit for bit (the encoding is not part of the mode); H is not
    _, enc32, H32 = _train_fwd(m, x, aux, _lib.MLP_FP32)
    assert torch.equal(enc, enc32) and not torch.equal(H, H32)
    _check(f"train arrays {kind} {weights}", {"heads": rel_err(raw, ref["raw"]), "enc": rel_err(enc[:, :in_ch], ref["enc"]),
                                              "acts": rel_err(H, ref["H"]), "g_pre": rel_err(G, ref["G"]),
                                              "g_enc": rel_err(ge[:, :in_ch], ref["g_enc"])})  # fmt: skip
    for l in range(8):  # layer by layer too: the largest layer must not hide the smallest
        assert rel_err(H[l], ref["H"][l]) <= REL_TOL and rel_err(G[l], ref["G"][l]) <= REL_TOL, l


FORMS = {"library_products": {}, "fused_param_grads": {"fused_param_grads": True}, "input_grads": {"input_grads": True},
         "chunked_1": {"input_grads": True, "fused_param_grads": True, "chunked_backward": 1}}  # fmt: skip


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind,weights", [("deform", "default"), ("deform", "half_dead"), ("control", "default"), ("blender", "default")])
def test_mlp_train_against_float64(kind, weights, form):
    """``ops.mlp_train(..., precision="bf16x3")`` in every form of its backward: heads, every parameter gradient and, where
    asked for, the gradients of ``x`` and ``aux``."""
    c, m, x, aux, gh = _on_device(kind, weights)
    ref = c["ref"]
    raw, grads, g_x, g_aux = train_step(m, x, aux, gh, precision=SPLIT, **FORMS[form])
    trunk_and_heads = {k: v for k, v in ref["grads"].items() if v is not None and not k.startswith("timenet")}
    assert set(grads) == set(trunk_and_heads) and len(grads) == 2 * (8 + len(head_rows(m)))
    errs = {"heads": rel_err(raw, ref["raw"])}
    errs.update({k: rel_err(grads[k], w) for k, w in trunk_and_heads.items()})
    if FORMS[form].get("input_grads"):
        errs["g_x"], errs["g_aux"] = rel_err(g_x, ref["g_x"]), rel_err(g_aux, ref["g_aux"])
    else:
        assert g_x is None and g_aux is None
    _check(f"mlp_train {kind} {weights} {form}", errs)


@pytest.mark.parametrize("kind", ["deform", "blender"])
def test_chunked_backward_equals_the_two_calls(kind):
    """``fg_mlp_train_bwd`` under the mode for chunks of one slab and of all of them: ``g_enc`` and every parameter gradient
    bit for bit what ``fg_mlp_bwd_inputs`` + ``fg_mlp_param_grads`` give (``g_pre`` lives in the call's workspace: the
    gradients formed from it are its witness), and not the fp32 chain's."""
    c, m, x, aux, gh = _on_device(kind)
    A, rows = aux.shape[1], head_rows(m)
    _, enc, H = _train_fwd(m, x, aux)
    G, ge = _bwd(m, A, H, gh, inputs=True)
    want = [t for group in ops.mlp_param_grads(enc, H, G, gh, A, rows) for t in group]
    slabs = -(-ROWS // ops.mlp_wgrad_slab_rows(ROWS))
    assert slabs >= 2
    for chunk_slabs in (1, slabs):
        *grads4, ge_c = ops.mlp_train_backward(enc, H, gh, m.linear, heads_of(m), A, rows, want_g_enc=True, chunk_slabs=chunk_slabs,
                                               precision=SPLIT)  # fmt: skip
        assert torch.equal(ge_c, ge), chunk_slabs
        for i, (a, b) in enumerate(zip([t for group in grads4 for t in group], want)):
            assert torch.equal(a, b), (chunk_slabs, i)
    *_, ge32 = ops.mlp_train_backward(enc, H, gh, m.linear, heads_of(m), A, rows, want_g_enc=True, chunk_slabs=1)
    assert not torch.equal(ge32, ge)


# ---- 3. bitwise repeat and row independence --------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["default", "half_dead"])
def test_rows_are_independent_and_runs_repeat_bitwise(weights):
    """An output element's three-term sums run over its own row in a fixed order: neither the tile a row lands in, its place
    there, the rows beside it nor the pad rows of the last tile can show.  Forward (SE(3) epilogue included) and backward."""
    _, m, x, aux, gh = _on_device("deform", weights)
    n = 200
    x, aux, gh = x[:n].contiguous(), aux[:n].contiguous(), gh[:n].contiguous()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(6)).to(DEV)

    def run(x, aux, gh):
        raw, enc, H = _train_fwd(m, x, aux)
        G, ge = _bwd(m, aux.shape[1], H, gh, inputs=True)
        return [*_forward(m, x, aux), raw, enc, H.transpose(0, 1), G.transpose(0, 1), ge]  # (rows first)

    a, b = run(x, aux, gh), run(x, aux, gh)
    p = run(x[perm].contiguous(), aux[perm].contiguous(), gh[perm].contiguous())
    d = run(x[: M + 1].contiguous(), aux[: M + 1].contiguous(), gh[: M + 1].contiguous())
    for i, (u, v, w, z) in enumerate(zip(a, b, p, d)):
        assert bool(torch.isfinite(u).all()) and torch.equal(u, v), i
        assert torch.equal(u[perm], w), i
        assert torch.equal(u[: M + 1], z), i


# ---- 4. edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["A1", "A64"])
def test_narrowest_and_widest_input_row(kind):
    """aux widths 1 (the input row's last k-step is mostly padding) and 64 (no padding at all), four plain heads."""
    c, m, x, aux, gh = _on_device(kind)
    ref, A = c["ref"], aux.shape[1]
    n = 200
    got = _forward(m, x[:n].contiguous(), aux[:n].contiguous())
    raw, enc, H = _train_fwd(m, x, aux)
    G, ge = _bwd(m, A, H, gh, inputs=True)
    assert torch.equal(torch.cat(got, dim=1), raw[:n])
    _check(f"edges {kind}", {"heads": rel_err(raw, ref["raw"]), "acts": rel_err(H, ref["H"]), "g_pre": rel_err(G, ref["G"]),
                             "g_enc": rel_err(ge[:, : 63 + A], ref["g_enc"])})  # fmt: skip
    assert bool((ge[:, 63 + A :] == 0).all())


def test_one_row_aux():
    """One ``aux`` row for all (stride 0): the rows' results are those of the row repeated."""
    _, m, x, aux, _ = _on_device("deform")
    n = 2 * M + 3
    x = x[:n].contiguous()
    one = aux[5:6].contiguous()
    want = _forward(m, x, one.expand(n, -1).contiguous())
    for form in (one, one.expand(n, -1)):
        for g, w in zip(_forward(m, x, form), want):
            assert torch.equal(g, w)


def test_null_outputs_guard_bands_and_the_bottom_row():
    _, m, x, aux, gh = _on_device("deform")
    n = 200
    x, aux, gh = x[:n].contiguous(), aux[:n].contiguous(), gh[:n].contiguous()
    full = _forward(m, x, aux)
    assert torch.equal(full[0][:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0], device=DEV).expand(n, 4))
    lib = _lib.load()
    shapes = ((n, 4, 4), (n, 4), (n, 3), (n, 3))
    for skip in (0, 3, None):  # no d_xyz but pts; d_xyz but no pts; all four
        arenas = [arena(*s) for s in shapes]
        ws_flat, ws = arena(int(lib.fg_mlp_workspace_bytes(n)) // 4)
        d, _, _, keep = ops._mlp_desc("test", x, aux, m.linear, heads_of(m), _lib.MLP_SE3)
        d.precision = _lib.MLP_BF16X3
        for i, (_, view) in enumerate(arenas):
            d.out[i] = None if i == skip else view.data_ptr()
        ops._call("fg_mlp_fwd", n, ctypes.addressof(d), ws.data_ptr(), ws.numel() * 4, ops._stream())
        torch.cuda.synchronize()
        for i, (flat, view) in enumerate(arenas):
            if i == skip:
                assert bool(torch.isnan(flat).all())  # not asked for: not touched
            else:
                assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all()) and torch.equal(view, full[i])
        assert bool(torch.isnan(ws_flat[:GUARD]).all()) and bool(torch.isnan(ws_flat[-GUARD:]).all())
    # the training calls: every array between NaN bands, the workspaces too; inputs unchanged; the unguarded run's bits
    A = aux.shape[1]
    raw, enc, H = _train_fwd(m, x, aux)
    G, ge = _bwd(m, A, H, gh, inputs=True)
    fwd = [arena(*t.shape) for t in (raw, enc, H)]
    ws_flat, ws = arena(int(lib.fg_mlp_train_workspace_bytes(n)) // 4)
    _train_fwd(m, x, aux, bufs=[v for _, v in fwd], ws=ws)
    for ins in (True, False):
        bwd = [arena(*G.shape), arena(*ge.shape)]
        hin = [arena(*H.shape), arena(*gh.shape)]
        hin[0][1].copy_(H), hin[1][1].copy_(gh)
        before = [flat.clone() for flat, _ in hin]
        need = lib.fg_mlp_bwd_inputs_workspace_bytes(n) if ins else lib.fg_mlp_train_workspace_bytes(n)
        wsb_flat, wsb = arena(int(need) // 4)
        _bwd(m, A, hin[0][1], hin[1][1], inputs=ins, bufs=(bwd[0][1], bwd[1][1] if ins else None), ws=wsb)
        torch.cuda.synchronize()
        for flat in [f for f, _ in fwd] + [bwd[0][0], ws_flat, wsb_flat] + ([bwd[1][0]] if ins else []):
            assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())
        for (flat, _), was in zip(hin, before):
            assert torch.equal(flat.view(torch.int32), was.view(torch.int32))
        assert torch.equal(bwd[0][1], G) and (torch.equal(bwd[1][1], ge) if ins else bool(torch.isnan(bwd[1][0]).all()))
    for (_, view), t in zip(fwd, (raw, enc, H)):
        assert torch.equal(view, t)


# ---- 5. graph capture ------------------------------------------------------------------------------------------------------
def test_capture_and_replay_equal_the_eager_call():
    _, m, x, aux, _ = _on_device("deform")
    n = 2 * M + 3
    x, aux = x[:n].contiguous(), aux[:n].contiguous()
    eager = _forward(m, x, aux)
    torch.cuda.synchronize()
    outs = [_nan(n, 4, 4), _nan(n, 4), _nan(n, 3), _nan(n, 3)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.mlp_forward(x, aux, m.linear, heads_of(m), outs=outs, precision=SPLIT)
    for _ in range(2):
        for o in outs:
            o.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, eager):
            assert torch.equal(o, e)


# ---- 6. through the modules and the model ----------------------------------------------------------------------------------
@pytest.fixture
def recorder(monkeypatch):
    calls = {"forward": [], "train": []}
    real_forward, real_train = ops.mlp_forward, ops.mlp_train

    def forward(*a, **k):
        calls["forward"].append((a, k))
        return real_forward(*a, **k)

    def train(*a, **k):
        calls["train"].append((a, k))
        return real_train(*a, **k)

    monkeypatch.setattr(ops, "mlp_forward", forward)
    monkeypatch.setattr(ops, "mlp_train", train)
    return calls


@pytest.mark.parametrize("kind", ["deform", "control"])
def test_module_dispatch(kind, recorder, monkeypatch):
    """The knob reaches ``ops`` where a fused path takes the call, as ``precision="bf16x3"``; unset, no ``precision`` is passed
    (``ops``' default, "fp32") and the outputs are the explicit fp32 call's bits."""
    monkeypatch.setenv("FG_FUSED_MLP", "1")
    monkeypatch.delenv("FG_FUSED_MLP_PRECISION", raising=False)
    torch.manual_seed(0)
    m = (D.FreeGaussianControllableModel() if kind == "control" else D.FreeGaussianDeformableModel()).to(DEV)
    n = max(33_000, D.FUSED_MIN_ROWS)
    g = torch.Generator().manual_seed(10)
    x = (torch.rand(n, 3, generator=g) * 2 - 1).to(DEV)
    other = (torch.randn(n, 3, generator=g) * 0.1 if kind == "control" else torch.rand(n, 1, generator=g)).to(DEV)
    with torch.no_grad():
        unset = m(x, other)
        monkeypatch.setenv("FG_FUSED_MLP_PRECISION", "fp32")
        named = m(x, other)
        monkeypatch.setenv("FG_FUSED_MLP_PRECISION", SPLIT)
        split = m(x, other)
    kws = [k for _, k in recorder["forward"]]
    assert [k.get("precision", "fp32") for k in kws] == ["fp32", "fp32", SPLIT] and "precision" not in kws[0]
    for a, b, c in zip(unset, named, split):
        assert torch.equal(a, b) and not torch.equal(a, c) and rel_err(c, a) <= REL_TOL
    # the taped call under FG_FUSED_MLP_TRAIN=2
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "2")
    outs = m(x, other)
    assert len(recorder["train"]) == 1 and recorder["train"][0][1] == {"input_grads": True, "precision": SPLIT}
    monkeypatch.delenv("FG_FUSED_MLP_PRECISION")
    outs32 = m(x, other)
    assert recorder["train"][1][1] == {"input_grads": True}
    for a, b in zip(outs, outs32):
        assert a.requires_grad and not torch.equal(a, b) and rel_err(a, b) <= REL_TOL
    # a typo is an error where a fused path takes the call, and only there
    monkeypatch.setenv("FG_FUSED_MLP_PRECISION", "bf16")
    with pytest.raises(ValueError, match="FG_FUSED_MLP_PRECISION"):
        m(x, other)
    assert m(x[:100], other[:100])[0].shape[0] == 100  # below the threshold: the torch ops, the knob is not read


def _clear_of_the_kink_on_device(net, x, aux, margin):
    """``mlp_inputs_common.rows_clear_of_the_kink_aux`` -- the same rule, in float64 -- on the device (one ``aux`` row for all)."""
    lin = copy.deepcopy(net.linear).double()
    with torch.no_grad():
        inp = torch.cat([D.positional_encoding(x.double(), 10), aux.double().expand(x.shape[0], -1)], dim=-1)
        ok, h = torch.ones(x.shape[0], dtype=torch.bool, device=x.device), inp
        for i, layer in enumerate(lin):
            z = layer(h)
            ok &= (z.abs() > margin * z.abs().max()).all(dim=1)
            h = torch.cat([inp, torch.relu(z)], dim=-1) if i == net.skip_at else torch.relu(z)
    return ok


def test_model_training_step_with_the_knob_set_and_unset(recorder, monkeypatch):
    """The default (blender) model, one training step with the knob set and one with it unset: every parameter gradient
    within the bar.  An image of ONE 16 x 16 tile gives every splat one job in the render's backward (one float atomic per
    (splat, job): two runs of it agree bit for bit only where no splat gets more than two addends), so the step is
    repeatable and the difference between the two steps is the mode's alone (tests/test_mlp_chunked_gpu.py).

    The Gaussians are drawn clear of the ReLU's kink like every other row a gradient is compared on here (the rule and the
    margin of tests/mlp_split_common.py, for the model's own net at the camera's time, 3 candidates a row).  Without that
    the step is not comparable at any bar: measured with unfiltered points (MI355X), a handful of the 33 024 rows take the
    other branch of one unit -- a flip in layer 6, one in layer 1 -- and the gradients of exactly those layers and the ones
    below differ by 2e-4 (layer 6), 1e-2 (layer 1) and 1e-3 (layer 0) while every other one stays below 5e-5."""
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat
    from mlp_split_common import MARGIN

    torch.manual_seed(0)
    n, W, H = D.FUSED_MIN_ROWS, 16, 16
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    pool = (torch.rand(3 * n, 3) - 0.5) * 2.0
    model = FreeGaussianModel(cfg, seed_points=pool[:n], init_scales=-3.8, is_blender=True)
    with torch.no_grad():
        model.gauss_params["scales"].normal_(-3.8, 0.3)
        model.gauss_params["features_rest"].normal_(0, 0.1)
        for q in model.deform.parameters():
            q.mul_(0.3)
    model = model.to(DEV).train()
    with torch.no_grad():
        net = model.deform
        aux = net.timenet(D.positional_encoding(torch.tensor([[0.4]], device=DEV), net.t_multires))
        ok = _clear_of_the_kink_on_device(net, pool.to(DEV), aux, MARGIN)
        assert int(ok.sum()) >= n, int(ok.sum())
        model.gauss_params["means"].copy_(pool.to(DEV)[ok][:n])
    model.step = 4000  # behind warm_up: the deformation net runs
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1
    cam = Camera(c2w[None, :3], 56.0, 60.0, W / 2, H / 2, W, H, times=torch.tensor([[0.4]]))
    gt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(12)).to(DEV)
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "2")
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD", "1")
    grads, losses = {}, {}
    for knob in (SPLIT, None):
        monkeypatch.setenv("FG_FUSED_MLP_PRECISION", knob) if knob else monkeypatch.delenv("FG_FUSED_MLP_PRECISION")
        model.zero_grad(set_to_none=True)
        out = model.get_outputs(copy.deepcopy(cam))
        loss = model.get_loss_dict(out, {"image": gt})["main_loss"]
        loss.backward()
        losses[knob] = loss.detach().clone()
        grads[knob] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    assert [k.get("precision", "fp32") for _, k in recorder["train"]] == [SPLIT, "fp32"]
    on, off = grads[SPLIT], grads[None]
    assert set(on) == set(off) and len([k for k in on if k.startswith("deform.")]) == 28
    errs = {k: rel_err(on[k], off[k]) for k in on}
    errs["loss"] = rel_err(losses[SPLIT], losses[None])
    _check("model step, knob set against unset", errs)
    assert any(not torch.equal(on[k], off[k]) for k in on)
