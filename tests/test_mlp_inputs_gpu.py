"""GPU: the fused MLP backward with input-row gradients (``fg_mlp_bwd_inputs``, ``ops.mlp_train(..., input_grads=True)``,
``FG_FUSED_MLP_TRAIN=2``) against a float64 run of the same network on the CPU whose input row wants a gradient
(tests/mlp_inputs_common.py), against ``fg_mlp_bwd`` (``g_pre``, bit for bit) and against itself (row independence,
repeatability, graph replay).

The float64 run is made once per (network, weights) for the largest size, on rows clear of the ReLU's kink; rows are
independent, so a smaller size is a prefix of it.

Measured margins (MI355X; helpers records them): profiles/mlp_train_inputs.md."""
import copy
import ctypes

import pytest
import torch

from freegaussian_amd import _lib
from freegaussian_amd import deform as D
from freegaussian_amd import ops
from helpers import REL_TOL, rel_err
from mlp_common import GUARD, NAN, arena, named_grads_or_zeros
from mlp_inputs_common import (BLENDER_TIME, aux_width, blender_clear_points, clear_inputs, float64_with_input_row, inputs,
                               make_net, module_float64, rows_clear_of_the_kink_aux, timenet_margin)  # fmt: skip
from mlp_train_common import cotangents, head_rows, heads_of, loss_of, rows_clear_of_the_kink

pytestmark = pytest.mark.gpu

DEV = "cuda"
M = ops.MLP_ROW_TILE
SIZES = [1, M - 1, M, M + 1, 2 * M + 1]
N_MAX = max(SIZES)
N_DISPATCH = 33_000
# aux widths 21 and 63 (the modules), and 1, 30, 64: enc widths 88, 128, 64, 96, 128 -- the narrowest row, a pad tail, the
# blender width, all four waves' blocks live
KINDS = ["deform", "control", "A1", "A30", "A64"]
CASES = [(k, w) for k in KINDS for w in ("default", "half_dead")]


@pytest.fixture
def spy(monkeypatch):
    """Calls of ops.mlp_train (positional and keyword arguments), and (inp, H, G, g_heads, rows) of every backward."""
    seen = {"train": [], "bwd": []}
    real_train, real_grads = ops.mlp_train, D.mlp_param_grads
    monkeypatch.setattr(ops, "mlp_train", lambda *a, **k: seen["train"].append((a, k)) or real_train(*a, **k))
    monkeypatch.setattr(D, "mlp_param_grads", lambda *a: seen["bwd"].append(a) or real_grads(*a))
    return seen


def _g_heads(m, n, seed=3):
    return torch.randn(n, sum(head_rows(m)), generator=torch.Generator().manual_seed(seed))


# ---- the C entry points on guarded buffers ------------------------------------------------------------------------------
def _entry_points(m_dev, x, aux, g_heads, plain_too=False):
    """fg_mlp_train_fwd and fg_mlp_bwd_inputs into NaN-filled buffers with a NaN guard band on either side of each: (enc, H,
    G, g_enc[, G of fg_mlp_bwd]); the bands must come back untouched and everything between them finite."""
    x, aux, g_heads = x.to(DEV).contiguous(), aux.to(DEV).contiguous(), g_heads.to(DEV).contiguous()
    d, n, rows, keep = ops._mlp_desc("test", x, aux, m_dev.linear, heads_of(m_dev), _lib.MLP_PLAIN)
    enc_w = _lib.mlp_enc_width(d.aux_width)
    arenas = [arena(n, sum(rows)), arena(n, enc_w), arena(8, n, 256), arena(8, n, 256), arena(n, enc_w), arena(8, n, 256)]
    (_, heads), (_, enc), (_, H), (_, G), (_, g_enc), (_, G_plain) = arenas
    lib = _lib.load()
    ws_flat, ws = arena(int(lib.fg_mlp_bwd_inputs_workspace_bytes(n)) // 4)
    st = ops._stream()
    ops._call("fg_mlp_train_fwd", n, ctypes.addressof(d), heads.data_ptr(), enc.data_ptr(), H.data_ptr(), ws.data_ptr(),
              int(lib.fg_mlp_train_workspace_bytes(n)), st)  # fmt: skip
    assert bool(torch.isnan(G).all()) and bool(torch.isnan(g_enc).all())  # (the forward does not know of them)
    ops._call("fg_mlp_bwd_inputs", n, ctypes.addressof(d), g_heads.data_ptr(), H.data_ptr(), G.data_ptr(), g_enc.data_ptr(),
              ws.data_ptr(), ws.numel() * 4, st)  # fmt: skip
    if plain_too:
        ops._call("fg_mlp_bwd", n, ctypes.addressof(d), g_heads.data_ptr(), H.data_ptr(), G_plain.data_ptr(), ws.data_ptr(),
                  int(lib.fg_mlp_train_workspace_bytes(n)), st)  # fmt: skip
    torch.cuda.synchronize()
    for flat, view in arenas[: 6 if plain_too else 5]:
        assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())
        assert bool(torch.isfinite(view).all())
    assert bool(torch.isnan(ws_flat[:GUARD]).all()) and bool(torch.isnan(ws_flat[-GUARD:]).all())
    return (enc, H, G, g_enc, G_plain) if plain_too else (enc, H, G, g_enc)


# ---- 1 / 2. g_enc against float64; g_pre is fg_mlp_bwd's, bit for bit ---------------------------------------------------
_REF = {}


def _arbiter(kind, weights):
    key = (kind, weights)
    if key not in _REF:
        m = make_net(kind, weights)
        x, aux = clear_inputs(m, N_MAX)
        g_heads = _g_heads(m, N_MAX)
        _REF[key] = dict(m=copy.deepcopy(m).to(DEV), x=x, aux=aux, g_heads=g_heads, ref=float64_with_input_row(m, x, aux, g_heads))
    return _REF[key]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind,weights", CASES)
def test_input_row_gradient_against_float64(kind, weights, n):
    a = _arbiter(kind, weights)
    m, ref = a["m"], a["ref"]
    if weights == "half_dead":
        assert 0.3 < float((ref["G"] == 0).double().mean()) < 0.7
    enc, H, G, g_enc, G_plain = _entry_points(m, a["x"][:n], a["aux"][:n], a["g_heads"][:n], plain_too=True)
    in_ch = 63 + aux_width(m)
    assert g_enc.shape == (n, _lib.mlp_enc_width(aux_width(m))) and ref["g_enc"].shape == (N_MAX, in_ch)
    errs = dict(enc=rel_err(enc[:, :in_ch], ref["enc"][:n]), g_enc=rel_err(g_enc[:, :in_ch], ref["g_enc"][:n]),
                G=max(rel_err(G[l], ref["G"][l, :n]) for l in range(8)))  # fmt: skip
    print(f"mlp_bwd_inputs {kind} {weights} n={n}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert float(ref["g_enc"][:n].abs().max()) > 0
    assert all(v < REL_TOL for v in errs.values()), errs
    # the pad columns: exact zeros
    assert bool((g_enc[:, in_ch:] == 0).all()) and bool((enc[:, in_ch:] == 0).all())
    # 2. the same chains as fg_mlp_bwd
    assert torch.equal(G, G_plain)


# ---- 3. guarded buffers: the last tile's rows beyond N ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["deform", "A64"])
def test_nothing_is_written_beyond_the_last_row(kind):
    """N = 65: one row in the second tile.  Every array is an arena of exactly N rows between NaN bands (`_entry_points`
    checks them): a store for one of the tile's other 63 rows would land in a band, or in the next layer's rows of
    ``g_pre``, which then would not equal ``fg_mlp_bwd``'s."""
    m = make_net(kind).to(DEV)
    n = M + 1
    x, aux = inputs(m, n, seed=5)
    g_heads = _g_heads(m, n, seed=6)
    enc, H, G, g_enc, G_plain = _entry_points(m, x, aux, g_heads, plain_too=True)
    assert torch.equal(G, G_plain)
    # the last row alone, as a call of its own: the same bits (nothing of the tile's other rows reaches it)
    one = _entry_points(m, x[n - 1 :], aux[n - 1 :], g_heads[n - 1 :])
    assert torch.equal(one[3], g_enc[n - 1 :]) and torch.equal(one[2], G[:, n - 1 :])


# ---- 4. rows independent, runs repeat -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["deform", "control", "A1"])
def test_rows_are_independent_and_runs_repeat(kind):
    m = make_net(kind).to(DEV)
    n = N_MAX
    x, aux = inputs(m, n, seed=7)
    g_heads = _g_heads(m, n, seed=8)
    a = _entry_points(m, x, aux, g_heads)
    b = _entry_points(m, x, aux, g_heads)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(9))
    c = _entry_points(m, x[perm], aux[perm], g_heads[perm])
    prefixes = {k: _entry_points(m, x[:k], aux[:k], g_heads[:k]) for k in (1, M - 1, M, M + 1)}
    for i, (u, v, w) in enumerate(zip(a, b, c)):
        rows_first = u if u.dim() == 2 else u.transpose(0, 1)  # [n, ...]
        assert torch.equal(u, v)
        assert torch.equal(rows_first[perm.to(DEV)], w if w.dim() == 2 else w.transpose(0, 1))
        for k, p in prefixes.items():
            assert torch.equal(rows_first[:k], p[i] if p[i].dim() == 2 else p[i].transpose(0, 1)), (i, k)


# ---- 5. ops.mlp_train(..., input_grads=True) ----------------------------------------------------------------------------
def _train_step(m_dev, x, aux, g_heads, **kw):
    """One taped ops.mlp_train + backward from the head cotangents: (raw, x.grad, aux.grad, parameter gradients)."""
    m_dev.zero_grad(set_to_none=True)
    x, aux = x.detach().to(DEV).requires_grad_(True), aux.detach().to(DEV).requires_grad_(True)
    raw = ops.mlp_train(x, aux, m_dev.linear, heads_of(m_dev), **kw)
    raw.backward(g_heads.to(DEV))
    return raw.detach(), x.grad, aux.grad, named_grads_or_zeros(m_dev)


def _check_param_grads(m_dev, grads, ref):
    want = {k: v for k, v in ref["grads"].items() if v is not None}
    assert set(want) <= set(grads) and len(want) == 2 * (8 + len(head_rows(m_dev)))
    return max(rel_err(grads[k], want[k]) for k in want)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["deform", "control", "A30"])
def test_ops_input_gradients_per_row_aux(kind, n, spy):
    a = _arbiter(kind, "default")
    m = a["m"]
    x, aux, g_heads = a["x"][:n], a["aux"][:n], a["g_heads"][:n]
    ref = a["ref"] if n == N_MAX else float64_with_input_row(m, x, aux, g_heads)  # (parameter gradients are sums over the rows)
    raw, g_x, g_aux, grads = _train_step(m, x, aux, g_heads, input_grads=True)
    assert g_x.shape == (n, 3) and g_aux.shape == (n, aux_width(m)) and len(spy["bwd"]) == 1
    errs = dict(raw=rel_err(raw, ref["raw"]), g_x=rel_err(g_x, ref["g_x"]), g_aux=rel_err(g_aux, ref["g_aux"]),
                params=_check_param_grads(m, grads, ref))  # fmt: skip
    print(f"mlp_train input_grads {kind} n={n}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < REL_TOL for v in errs.values()), errs
    # only x, only aux: the same gradient, bit for bit, and None for the other
    m.zero_grad(set_to_none=True)
    xd, ad = x.to(DEV).requires_grad_(True), aux.to(DEV)
    ops.mlp_train(xd, ad, m.linear, heads_of(m), input_grads=True).backward(g_heads.to(DEV))
    assert torch.equal(xd.grad, g_x) and ad.grad is None
    xd, ad = x.to(DEV), aux.to(DEV).requires_grad_(True)
    ops.mlp_train(xd, ad, m.linear, heads_of(m), input_grads=True).backward(g_heads.to(DEV))
    assert torch.equal(ad.grad, g_aux) and xd.grad is None


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["deform", "A30"])
def test_ops_input_gradients_one_row_aux(kind, n):
    m = make_net(kind)
    x, aux = inputs(m, n + n // 2 + 64, seed=11)
    one = aux[:1].contiguous()
    ok = rows_clear_of_the_kink_aux(m, x, one)
    assert int(ok.sum()) >= n
    x, g_heads = x[ok][:n].contiguous(), _g_heads(m, n, seed=12)
    ref = float64_with_input_row(m, x, one, g_heads)
    m_dev = copy.deepcopy(m).to(DEV)
    raw, g_x, g_aux, grads = _train_step(m_dev, x, one, g_heads, input_grads=True)
    assert g_aux.shape == one.shape == ref["g_aux"].shape
    errs = dict(raw=rel_err(raw, ref["raw"]), g_x=rel_err(g_x, ref["g_x"]), g_aux=rel_err(g_aux, ref["g_aux"]),
                params=_check_param_grads(m_dev, grads, ref))  # fmt: skip
    print(f"mlp_train input_grads, one aux row, {kind} n={n}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < REL_TOL for v in errs.values()), errs
    # the same row expanded (row stride 0, as the model passes its time): the leaf's gradient is the [1, A] sum again
    leaf = one.to(DEV).requires_grad_(True)
    ops.mlp_train(x.to(DEV), leaf.expand(n, -1), m_dev.linear, heads_of(m_dev), input_grads=True).backward(g_heads.to(DEV))
    assert torch.equal(leaf.grad, g_aux)


def test_ops_without_the_keyword_gives_the_inputs_no_gradient(spy):
    a = _arbiter("deform", "default")
    m, n = a["m"], M + 1
    raw, g_x, g_aux, grads = _train_step(m, a["x"][:n], a["aux"][:n], a["g_heads"][:n])
    assert g_x is None and g_aux is None
    raw2, g_x2, g_aux2, grads2 = _train_step(m, a["x"][:n], a["aux"][:n], a["g_heads"][:n], input_grads=False)
    assert g_x2 is None and g_aux2 is None and torch.equal(raw, raw2)
    # with the keyword and inputs that want nothing: fg_mlp_bwd as before -- the same G, the same parameter gradients
    m.zero_grad(set_to_none=True)
    ops.mlp_train(a["x"][:n].to(DEV), a["aux"][:n].to(DEV), m.linear, heads_of(m), input_grads=True).backward(a["g_heads"][:n].to(DEV))
    assert len(spy["bwd"]) == 3 and torch.equal(spy["bwd"][0][2], spy["bwd"][2][2])
    assert all(torch.equal(grads[k], v) for k, v in named_grads_or_zeros(m).items())
    # and with inputs that do: the parameter gradients are the same bits (g_pre is fg_mlp_bwd's)
    _, _, _, grads3 = _train_step(m, a["x"][:n], a["aux"][:n], a["g_heads"][:n], input_grads=True)
    assert torch.equal(spy["bwd"][3][2], spy["bwd"][0][2]) and all(torch.equal(grads[k], v) for k, v in grads3.items())


# ---- 6. through the module's dispatch -----------------------------------------------------------------------------------
def test_blender_net_through_the_module(spy, monkeypatch):
    torch.manual_seed(0)
    m = D.FreeGaussianDeformableModel(is_blender=True)
    n = N_DISPATCH
    assert n >= D.FUSED_MIN_ROWS and timenet_margin(m) >= 1e-4
    x = blender_clear_points(m, n)
    t = torch.full((1, 1), BLENDER_TIME)
    cots = cotangents(m, n)
    want_outs, want = module_float64(m, x, t.expand(n, -1), cots)
    m_dev = copy.deepcopy(m).to(DEV)
    xd, td, cd = x.to(DEV), t.to(DEV).expand(n, -1), [c.to(DEV) for c in cots]
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "2")
    outs = m_dev(xd, td)
    loss_of(outs, cd).backward()
    assert len(spy["train"]) == 1 and len(spy["bwd"]) == 1
    args, kw = spy["train"][0]
    assert args[1].shape == (1, 30) and args[1].requires_grad and kw == {"input_grads": True}  # the one time: timenet on one row
    grads = named_grads_or_zeros(m_dev)
    assert set(grads) == set(want) and len(grads) == 24 + 4 and sum(k.startswith("timenet.") for k in grads) == 4
    errs = {f"out{i}": rel_err(o, w) for i, (o, w) in enumerate(zip(outs, want_outs))}
    errs.update({k: rel_err(grads[k], want[k]) for k in sorted(want)})
    print("mlp_train blender module: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in want:
        assert float(want[k].abs().max()) > 0, k
    assert all(v < REL_TOL for v in errs.values()), errs
    # "1" leaves the blender net to the torch ops
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "1")
    plain = m_dev(xd, td)
    assert len(spy["train"]) == 1
    for a, b in zip(outs, plain):
        assert rel_err(a, b) < REL_TOL


def test_inputs_that_want_gradients_through_the_module(spy, monkeypatch):
    m = make_net("deform")
    n = N_DISPATCH
    g = torch.Generator().manual_seed(14)
    x, t = torch.rand(n + n // 2 + 64, 3, generator=g) * 2 - 1, torch.rand(n + n // 2 + 64, 1, generator=g)
    ok = rows_clear_of_the_kink(m, x, t)
    assert int(ok.sum()) >= n
    x, t, cots = x[ok][:n].contiguous(), t[ok][:n].contiguous(), cotangents(m, n)
    m64 = copy.deepcopy(m).double()
    x64, t64 = x.double().requires_grad_(True), t.double().requires_grad_(True)
    loss_of(m64(x64, t64), cots).backward()
    m_dev = copy.deepcopy(m).to(DEV)
    xd, td = x.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "2")
    loss_of(m_dev(xd, td), [c.to(DEV) for c in cots]).backward()
    assert len(spy["train"]) == 1 and spy["train"][0][1] == {"input_grads": True}
    errs = dict(g_x=rel_err(xd.grad, x64.grad), g_t=rel_err(td.grad, t64.grad))
    errs["params"] = max(rel_err(p.grad, dict(m64.named_parameters())[k].grad) for k, p in m_dev.named_parameters())
    print("mlp_train module, x and t want gradients: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < REL_TOL for v in errs.values()), errs
    # "1" refuses inputs that want a gradient; "2" takes what "1" takes, as "1" does (no keyword's worth of work: fg_mlp_bwd)
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "1")
    m_dev(xd, td)
    assert len(spy["train"]) == 1
    m_dev(xd.detach(), td.detach())
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "2")
    m_dev(xd.detach(), td.detach())
    assert len(spy["train"]) == 3


# ---- 7. graph capture ---------------------------------------------------------------------------------------------------
def test_capture_and_replay_equal_the_eager_call(spy):
    a = _arbiter("A30", "default")
    m, n = a["m"], N_MAX
    x, g_heads = a["x"].to(DEV).requires_grad_(True), a["g_heads"].to(DEV)
    aux = a["aux"][:1].to(DEV).requires_grad_(True)  # (one row for all: the column sum is part of the captured step)

    def step():
        m.zero_grad(set_to_none=True)
        x.grad = aux.grad = None
        raw = ops.mlp_train(x, aux, m.linear, heads_of(m), input_grads=True)
        raw.backward(g_heads)
        return raw.detach()

    raw_e = step().clone()
    eager = dict(g_x=x.grad.clone(), g_aux=aux.grad.clone(), G=spy["bwd"][0][2].clone(), params=named_grads_or_zeros(m))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_s = step()
    G_s, params = spy["bwd"][1][2], dict(m.named_parameters())
    for _ in range(3):
        for buf in (raw_s, G_s, x.grad, aux.grad, *(p.grad for p in params.values())):
            buf.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(raw_s, raw_e) and torch.equal(G_s, eager["G"])
        assert torch.equal(x.grad, eager["g_x"]) and torch.equal(aux.grad, eager["g_aux"])
        for k, p in params.items():
            assert rel_err(p.grad, eager["params"][k]) < REL_TOL, k


# ---- 8. the default model's training step -------------------------------------------------------------------------------
def test_default_model_training_step_with_the_knob_at_2_and_unset(spy, monkeypatch):
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat
    from freegaussian_amd.utils import positional_encoding

    torch.manual_seed(0)
    n, W, H = N_DISPATCH, 64, 48
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-3.8)  # (is_blender: the default)
    assert model.deform.is_blender
    with torch.no_grad():
        model.gauss_params["scales"].normal_(-3.8, 0.3)
        model.gauss_params["features_rest"].normal_(0, 0.1)
        for q in model.deform.parameters():
            q.mul_(0.3)
        # Gaussians within fp32 rounding of a ReLU's kink are moved, as tests/test_mlp_train_gpu.py moves them; the time must
        # leave timenet's own ReLU clear as well
        time = 0.4
        assert timenet_margin(model.deform, time) >= 1e-4
        aux = copy.deepcopy(model.deform.timenet).double()(positional_encoding(torch.tensor([[time]], dtype=torch.float64), 6))
        means = model.gauss_params["means"]
        bad = ~rows_clear_of_the_kink_aux(model.deform, means, aux)
        pool = (torch.rand(n // 2, 3) - 0.5) * 2.0
        pool = pool[rows_clear_of_the_kink_aux(model.deform, pool, aux)]
        assert 0 < int(bad.sum()) <= pool.shape[0]
        means[bad] = pool[: int(bad.sum())]
    model.step = 4000
    model = model.to(DEV).train()
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1
    cam = Camera(c2w[None, :3], 56.0, 60.0, W / 2, H / 2, W, H, times=torch.tensor([[time]]))
    gt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(12)).to(DEV)
    grads, losses = {}, {}
    for knob in ("2", None):
        monkeypatch.setenv("FG_FUSED_MLP_TRAIN", knob) if knob else monkeypatch.delenv("FG_FUSED_MLP_TRAIN")
        model.zero_grad(set_to_none=True)
        out = model.get_outputs(copy.deepcopy(cam))
        loss = model.get_loss_dict(out, {"image": gt})["main_loss"]
        loss.backward()
        losses[knob] = loss.detach()
        grads[knob] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        assert len(spy["train"]) == 1  # the taped forward of the knob-on step, and no other
    on, off = grads["2"], grads[None]
    assert set(on) == set(off)
    deform = [k for k in on if k.startswith("deform.")]
    gauss = [k for k in on if k.startswith("gauss_params.")]
    assert len(deform) == 24 + 4 and len(gauss) >= 5
    errs = {k: rel_err(on[k], off[k]) for k in deform + gauss}
    errs["loss"] = rel_err(losses["2"], losses[None])
    print("mlp_train default model step: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in deform + gauss:
        assert float(off[k].abs().max()) > 0, k
    assert all(v < REL_TOL for v in errs.values()), errs
