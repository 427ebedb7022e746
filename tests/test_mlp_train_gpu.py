"""GPU: the fused fp32 MLP training path (``ops.mlp_train`` / ``fg_mlp_train_fwd`` / ``fg_mlp_bwd``) against a float64 run
of the same network on the CPU (tests/mlp_train_common.py: the module's own torch ops, layer by layer), against the
inference kernel (raw heads, bit for bit) and against itself (row independence, repeatability, graph replay).

The float64 run is made once per (network, weights) for the largest size, on rows clear of the ReLU's kink
(``rows_clear_of_the_kink``); rows are independent, so a smaller size is a prefix of it, and the parameter gradients of a
prefix are ``deform.mlp_param_grads`` of the prefix in float64 (tests/test_mlp_train_host.py holds that to autograd).
``H`` and ``G`` of a run are what ``ops.mlp_train``'s backward hands ``deform.mlp_param_grads``: a spy keeps them.

Measured margins (MI355X; helpers records them): profiles/mlp_train.md."""
import copy
import ctypes

import pytest
import torch

from freegaussian_amd import _lib
from freegaussian_amd import deform as D
from freegaussian_amd import ops
from helpers import REL_TOL, rel_err
from mlp_common import GUARD, NAN, arena, named_grads_or_zeros
from mlp_train_common import (assembled, aux_of, cotangents, half_dead_, head_rows, heads_of, loss_of, manual_float64,
                              outputs_from_raw, rows_clear_of_the_kink)  # fmt: skip

pytestmark = pytest.mark.gpu

DEV = "cuda"
M = ops.MLP_ROW_TILE
CHUNK = D._TallLinear.CHUNK
SIZES = [1, M - 1, M, M + 1, 2 * M + 1, CHUNK + 65, 33_000]
N_MAX = max(SIZES)


def _net(kind, weights="default"):
    torch.manual_seed(0)
    m = D.FreeGaussianControllableModel() if kind == "control" else D.FreeGaussianDeformableModel()
    return half_dead_(m) if weights == "half_dead" else m


def _inputs(kind, n, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g) * 2 - 1
    return x, (torch.randn(n, 3, generator=g) * 0.1 if kind == "control" else torch.rand(n, 1, generator=g))


def _clear_inputs(m, kind, n, seed=1):
    """n rows of `_inputs` that are clear of the ReLU's kink for the network `m`."""
    x, other = _inputs(kind, n + n // 2 + 64, seed)
    ok = rows_clear_of_the_kink(m, x, other)
    assert int(ok.sum()) >= n
    return x[ok][:n].contiguous(), other[ok][:n].contiguous()


@pytest.fixture
def spy(monkeypatch):
    """Calls of ops.mlp_train, and (inp, H, G, g_heads) of every backward."""
    seen = {"train": [], "bwd": []}
    real_train, real_grads = ops.mlp_train, D.mlp_param_grads
    monkeypatch.setattr(ops, "mlp_train", lambda *a, **k: seen["train"].append(a) or real_train(*a, **k))
    monkeypatch.setattr(D, "mlp_param_grads", lambda *a: seen["bwd"].append(a) or real_grads(*a))
    return seen


def _fused_step(m_dev, x, other, cots):
    """One taped ops.mlp_train + the module's head arithmetic + backward: (raw heads, outputs, parameter gradients)."""
    m_dev.zero_grad(set_to_none=True)
    raw = ops.mlp_train(x.to(DEV), aux_of(m_dev, other.to(DEV)), m_dev.linear, heads_of(m_dev))
    outs = outputs_from_raw(m_dev, raw)
    loss_of(outs, [None if c is None else c.to(DEV) for c in cots]).backward()
    return raw.detach(), [o.detach() for o in outs], named_grads_or_zeros(m_dev)


# ---- 1. float64 arbiter ----------------------------------------------------------------------------------------------
_REF = {}


def _arbiter(kind, weights):
    key = (kind, weights)
    if key not in _REF:
        m = _net(kind, weights)
        x, other = _clear_inputs(m, kind, N_MAX)
        cots = cotangents(m, N_MAX)
        _REF[key] = dict(m=copy.deepcopy(m).to(DEV), x=x, other=other, cots=cots, ref=manual_float64(m, x, other, cots))
    return _REF[key]


def _check_against_float64(tag, m_dev, seen_bwd, outs, grads, ref, n):
    inp, H, G, g_heads, rows = seen_bwd
    assert H.shape == G.shape == (8, n, 256) and list(rows) == head_rows(m_dev)
    want = assembled(m_dev, D.mlp_param_grads(ref["inp"][:n], ref["H"][:, :n], ref["G"][:, :n], ref["g_heads"][:n], rows))
    assert set(want) == set(grads) and len(want) == 2 * (8 + len(rows))
    pairs = [("inp", inp, ref["inp"][:n]), ("g_heads", g_heads, ref["g_heads"][:n])]
    pairs += [(f"out{i}", o, w[:n]) for i, (o, w) in enumerate(zip(outs, ref["outs"]))]
    pairs += [(f"H[{l}]", H[l], ref["H"][l, :n]) for l in range(8)] + [(f"G[{l}]", G[l], ref["G"][l, :n]) for l in range(8)]
    pairs += [(k, grads[k], want[k]) for k in sorted(want)]
    worst = {}
    for name, got, w in pairs:
        assert bool(torch.isfinite(got).all()), name
        err = rel_err(got, w)
        group = name.split("[")[0] if "[" in name else ("param grads" if name in want else name)
        worst[group] = max(worst.get(group, 0.0), err)
        assert err < REL_TOL, (name, err)
    print(f"mlp_train {tag} n={n}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind,weights", [("deform", "default"), ("deform", "half_dead"), ("control", "default"),
                                          ("control", "half_dead")])  # fmt: skip
def test_activations_and_gradients_against_float64(kind, weights, n, spy, monkeypatch):
    a = _arbiter(kind, weights)
    m, ref = a["m"], a["ref"]
    x, other, cots = a["x"][:n], a["other"][:n], [c[:n] for c in a["cots"]]
    if weights == "half_dead":
        assert 0.3 < float((ref["H"] <= 0).double().mean()) < 0.7
    if n >= D.FUSED_MIN_ROWS:  # through the module's dispatch
        monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "1")
        m.zero_grad(set_to_none=True)
        outs = m(x.to(DEV), other.to(DEV))
        loss_of(outs, [c.to(DEV) for c in cots]).backward()
        outs, grads = [o.detach() for o in outs], named_grads_or_zeros(m)
    else:
        _, outs, grads = _fused_step(m, x, other, cots)
    assert len(spy["train"]) == 1 and len(spy["bwd"]) == 1
    _check_against_float64(f"{kind} {weights}", m, spy["bwd"][0], outs, grads, ref, n)


# ---- 2. the raw heads are the inference kernel's, bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("kind", ["deform", "control"])
def test_raw_heads_equal_the_inference_kernel_bitwise(kind):
    m = _net(kind).to(DEV)
    for n in (1, M + 1, CHUNK + 65):
        x, other = _inputs(kind, n, seed=2)
        x, aux = x.to(DEV), aux_of(m, other.to(DEV))
        raw = ops.mlp_train(x, aux, m.linear, heads_of(m))
        plain = ops.mlp_forward(x, aux, m.linear, heads_of(m), mode="plain")
        assert raw.requires_grad and raw.shape == (n, sum(head_rows(m)))
        assert torch.equal(raw.detach(), torch.cat(plain, dim=-1))
    # one aux row for all (the stride-0 time the model passes)
    one = aux_of(m, other.to(DEV))[:1]
    assert torch.equal(ops.mlp_train(x, one, m.linear, heads_of(m)).detach(),
                       torch.cat(ops.mlp_forward(x, one, m.linear, heads_of(m), mode="plain"), dim=-1))  # fmt: skip


# ---- 3. the C entry points on guarded buffers ---------------------------------------------------------------------------
def _entry_points(m_dev, x, aux, g_heads):
    """fg_mlp_train_fwd and fg_mlp_bwd into NaN-filled buffers with a NaN guard band on either side of each: (heads, enc,
    H, G); the bands must come back untouched and everything between them finite."""
    d, n, rows, keep = ops._mlp_desc("test", x, aux, m_dev.linear, heads_of(m_dev), _lib.MLP_PLAIN)
    arenas = [arena(n, sum(rows)), arena(n, _lib.mlp_enc_width(d.aux_width)), arena(8, n, 256), arena(8, n, 256)]
    (_, heads), (_, enc), (_, H), (_, G) = arenas
    ws = torch.empty(int(_lib.load().fg_mlp_train_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
    args = (ws.data_ptr(), ws.numel(), ops._stream())
    ops._call("fg_mlp_train_fwd", n, ctypes.addressof(d), heads.data_ptr(), enc.data_ptr(), H.data_ptr(), *args)
    assert bool(torch.isnan(G).all())  # (the forward does not know of it)
    g_heads = g_heads.to(DEV).contiguous()
    ops._call("fg_mlp_bwd", n, ctypes.addressof(d), g_heads.data_ptr(), H.data_ptr(), G.data_ptr(), *args)
    torch.cuda.synchronize()
    for flat, view in arenas:
        assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())
        assert bool(torch.isfinite(view).all())
    return heads, enc, H, G


@pytest.mark.parametrize("kind", ["deform", "control"])
def test_rows_are_independent_runs_repeat_and_nothing_else_is_written(kind):
    m = _net(kind).to(DEV)
    n = 2 * M + 3
    x, other = _inputs(kind, n, seed=5)
    x, aux = x.to(DEV), aux_of(m, other.to(DEV))
    g_heads = torch.randn(n, sum(head_rows(m)), generator=torch.Generator().manual_seed(6)).to(DEV)
    a = _entry_points(m, x, aux, g_heads)
    b = _entry_points(m, x, aux, g_heads)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(7)).to(DEV)
    c = _entry_points(m, x[perm], aux[perm], g_heads[perm])
    k = M + 1
    d = _entry_points(m, x[:k], aux[:k], g_heads[:k])
    for u, v, w, p in zip(a, b, c, d):
        rows_first = u if u.dim() == 2 else u.transpose(0, 1)  # [n, ...]
        assert torch.equal(u, v)
        assert torch.equal(rows_first[perm], w if w.dim() == 2 else w.transpose(0, 1))
        assert torch.equal(rows_first[:k], p if p.dim() == 2 else p.transpose(0, 1))
    # the encoded row: the module's own encoding, zero padded
    in_ch = m.input_ch
    assert rel_err(a[1][:, :in_ch], torch.cat([D.positional_encoding(x, m.multires), aux], dim=-1)) < REL_TOL
    assert bool((a[1][:, in_ch:] == 0).all())


# ---- 4. structure -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zeroed", ["input_columns", "hidden_columns"])
def test_skip_layer_halves_against_float64(zeroed, spy):
    m = _net("deform")
    in_ch = m.input_ch
    with torch.no_grad():
        if zeroed == "input_columns":
            m.linear[5].weight[:, :in_ch] = 0.0
        else:
            m.linear[5].weight[:, in_ch:] = 0.0
    n = M + 5
    x, other = _clear_inputs(m, "deform", n, seed=8)
    cots = cotangents(m, n)
    ref = manual_float64(m, x, other, cots)
    m_dev = copy.deepcopy(m).to(DEV)
    _, outs, grads = _fused_step(m_dev, x, other, cots)
    _check_against_float64(f"skip {zeroed}", m_dev, spy["bwd"][0], outs, grads, ref, n)
    # layer 5's weight gradient: [P_5^T inp | P_5^T h_4], each half on its own scale
    g5, w5 = grads["linear.5.weight"], ref["grads"]["linear.5.weight"]
    assert rel_err(g5[:, :in_ch], w5[:, :in_ch]) < REL_TOL and rel_err(g5[:, in_ch:], w5[:, in_ch:]) < REL_TOL
    assert float(g5[:, :in_ch].abs().max()) > 0 and float(g5[:, in_ch:].abs().max()) > 0
    G = spy["bwd"][0][2]
    front = [k for k in grads if k.split(".")[0] == "linear" and int(k.split(".")[1]) < 5]
    assert len(front) == 10
    if zeroed == "hidden_columns":
        # nothing flows back through the hidden columns, and the input columns carry no data gradient: layers 0..4 get none
        assert bool((G[:5] == 0).all()) and float(G[5:].abs().max()) > 0
        assert all(bool((grads[k] == 0).all()) for k in front)
    else:
        assert all(float(G[l].abs().max()) > 0 for l in range(8))
        assert all(float(grads[k].abs().max()) > 0 for k in front)


def test_relu_at_zero_gets_no_gradient(spy):
    """Pre-activations that are exactly 0 (zero weights, zero bias) and negative for every row (zero weights, bias -1) in a
    middle layer: G is exactly 0 there, as torch's ReLU backward has it (h > 0, not h >= 0)."""
    m = _net("deform")
    with torch.no_grad():
        m.linear[3].weight[:64] = 0.0
        m.linear[3].bias[:64] = 0.0
        m.linear[3].weight[64:128] = 0.0
        m.linear[3].bias[64:128] = -1.0
    n = M + 5
    x, other = _inputs("deform", n, seed=9)
    cots = cotangents(m, n)
    ref = manual_float64(m, x, other, cots)
    assert bool((ref["G"][3][:, :128] == 0).all()) and float(ref["G"][3][:, 128:].abs().max()) > 0
    m_dev = copy.deepcopy(m).to(DEV)
    _, outs, grads = _fused_step(m_dev, x, other, cots)
    _, H, G, _, _ = spy["bwd"][0]
    assert bool((H[3][:, :128] == 0).all()) and bool((G[3][:, :128] == 0).all())
    assert float(G[3][:, 128:].abs().max()) > 0
    assert bool((grads["linear.3.weight"][:128] == 0).all()) and bool((grads["linear.3.bias"][:128] == 0).all())
    _check_against_float64("relu at zero", m_dev, spy["bwd"][0], outs, grads, ref, n)


def test_unused_head_counts_as_zeros():
    """A loss that never touches d_scaling: the torch path leaves that head's gradients None, the fused path's are zeros,
    and every other gradient agrees."""
    m = _net("deform").to(DEV)
    n = 2 * M + 1
    x, other = _inputs("deform", n, seed=10)
    cots = cotangents(m, n, unused=2)
    _, _, fused = _fused_step(m, x, other, cots)
    m.zero_grad(set_to_none=True)
    outs = m(x.to(DEV), other.to(DEV))  # (below FUSED_MIN_ROWS and the variable unset: the torch ops)
    loss_of(outs, [None if c is None else c.to(DEV) for c in cots]).backward()
    assert m.gaussian_scaling.weight.grad is None
    plain = named_grads_or_zeros(m)
    assert bool((fused["gaussian_scaling.weight"] == 0).all()) and bool((fused["gaussian_scaling.bias"] == 0).all())
    for k in plain:
        if not k.startswith("gaussian_scaling"):
            assert rel_err(fused[k], plain[k]) < REL_TOL, k


# ---- 5. dispatch --------------------------------------------------------------------------------------------------------
def test_module_dispatch(spy, monkeypatch):
    fwd_calls = []
    real_fwd = ops.mlp_forward
    monkeypatch.setattr(ops, "mlp_forward", lambda *a, **k: fwd_calls.append(a) or real_fwd(*a, **k))
    monkeypatch.setenv("FG_FUSED_MLP", "1")
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "1")
    n = max(33_000, D.FUSED_MIN_ROWS)
    m = _net("deform").to(DEV)
    x = _inputs("deform", n, seed=11)[0].to(DEV)
    t = torch.full((1, 1), 0.3, device=DEV).expand(n, -1)
    fused = m(x, t)
    assert len(spy["train"]) == 1 and spy["train"][0][1].shape == (1, 21)  # the broadcast time: encoded on one row
    assert [tuple(o.shape) for o in fused] == [(n, 4, 4), (n, 4), (n, 3)] and all(o.requires_grad for o in fused)
    c = _net("control").to(DEV)
    got = c(x, torch.zeros(n, 3, device=DEV))
    assert len(spy["train"]) == 2 and [tuple(g.shape) for g in got] == [(n, 3), (n, 4), (n, 3)]
    # none of these takes it: too few rows, an input that wants a gradient, the blender net, the variable unset or not "1"
    k = D.FUSED_MIN_ROWS - 1
    m(x[:k], t[:k])
    m(x.clone().requires_grad_(True), t)
    D.FreeGaussianDeformableModel(is_blender=True).to(DEV)(x, t)
    for value in (None, "0", ""):
        monkeypatch.delenv("FG_FUSED_MLP_TRAIN") if value is None else monkeypatch.setenv("FG_FUSED_MLP_TRAIN", value)
        plain = m(x, t)
    assert len(spy["train"]) == 2 and not fwd_calls
    for a, b in zip(fused, plain):
        assert rel_err(a, b) < REL_TOL
    # the inference dispatch is what it was, with the new variable set
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "1")
    with torch.no_grad():
        m(x, t)
    assert len(fwd_calls) == 1 and len(spy["train"]) == 2
    monkeypatch.setenv("FG_FUSED_MLP", "0")
    with torch.no_grad():
        m(x, t)
    assert len(fwd_calls) == 1 and len(spy["train"]) == 2


def test_model_training_step_with_the_knob_on_and_off(spy, monkeypatch):
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    n, W, H = 33_000, 64, 48
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    # (is_blender=False: the 21-wide time encoding; the blender net's timenet keeps the torch path)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-3.8, is_blender=False)
    with torch.no_grad():
        model.gauss_params["scales"].normal_(-3.8, 0.3)
        model.gauss_params["features_rest"].normal_(0, 0.1)
        for q in model.deform.parameters():
            q.mul_(0.3)
        # Gaussians within fp32 rounding of a ReLU's kink are moved: there the two fp32 paths may each pick a mask, and one
        # flipped unit of the few hundred Gaussians in view at 64 x 48 moves a weight gradient by more than the bar
        time = 0.4
        means = model.gauss_params["means"]
        bad = ~rows_clear_of_the_kink(model.deform, means, torch.full((n, 1), time))
        pool = (torch.rand(n // 2, 3) - 0.5) * 2.0
        pool = pool[rows_clear_of_the_kink(model.deform, pool, torch.full((n // 2, 1), time))]
        assert 0 < int(bad.sum()) <= pool.shape[0]
        means[bad] = pool[: int(bad.sum())]
    model.step = 4000
    model = model.to(DEV).train()
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1
    cam = Camera(c2w[None, :3], 56.0, 60.0, W / 2, H / 2, W, H, times=torch.tensor([[time]]))
    gt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(12)).to(DEV)
    grads = {}
    for knob in ("1", None):
        monkeypatch.setenv("FG_FUSED_MLP_TRAIN", knob) if knob else monkeypatch.delenv("FG_FUSED_MLP_TRAIN")
        model.zero_grad(set_to_none=True)
        out = model.get_outputs(copy.deepcopy(cam))
        model.get_loss_dict(out, {"image": gt})["main_loss"].backward()
        grads[knob] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        assert len(spy["train"]) == 1  # the taped forward of the knob-on step, and no other
    on, off = grads["1"], grads[None]
    assert set(on) == set(off)
    deform = [k for k in on if k.startswith("deform.")]
    gauss = [k for k in on if k.startswith("gauss_params.")]
    assert len(deform) == 24 and len(gauss) >= 5
    errs = {k: rel_err(on[k], off[k]) for k in deform + gauss}
    print("mlp_train model step: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in deform + gauss:
        assert float(off[k].abs().max()) > 0, k
        assert errs[k] < REL_TOL, (k, errs[k])


# ---- 6. graph capture ---------------------------------------------------------------------------------------------------
def test_capture_and_replay_equal_the_eager_call(spy):
    m = _net("deform").to(DEV)
    n = CHUNK + 65
    x, other = _inputs("deform", n, seed=13)
    x, other, cots = x.to(DEV), other.to(DEV), [c.to(DEV) for c in cotangents(m, n)]  # (no host copy under capture)
    raw_e, _, grads_e = _fused_step(m, x, other, cots)
    G_e = spy["bwd"][0][2].clone()
    torch.cuda.synchronize()
    static = {}
    m.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static["raw"], _, _ = _fused_step(m, x, other, cots)
    static["G"] = spy["bwd"][1][2]
    params = dict(m.named_parameters())
    for _ in range(3):
        static["raw"].fill_(NAN)
        static["G"].fill_(NAN)
        for p in params.values():
            p.grad.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static["raw"], raw_e) and torch.equal(static["G"], G_e)
        for k, p in params.items():
            assert rel_err(p.grad, grads_e[k]) < REL_TOL, k
