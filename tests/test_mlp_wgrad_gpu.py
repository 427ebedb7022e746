"""GPU: the fused parameter-gradient call (``fg_mlp_param_grads`` / ``ops.mlp_param_grads``) by itself on random arrays
against ``deform.mlp_param_grads`` of the same arrays in float64 on the CPU, on guarded buffers, with outputs left out,
against itself (repeatability, graph replay), on constructed cases that are exact, and through ``ops.mlp_train``, the
modules and the model with ``FG_FUSED_MLP_WGRAD=1``.

Inputs of the stand-alone tests: ``H = relu(randn)`` (about half zeros), ``G = randn * (rand < 0.5) * 1e-3``, ``enc`` uniform
in [-1, 1], ``g_heads = randn * 1e-3``, seeded; one set of N_MAX rows per aux width, every smaller size a prefix of it.  On
these the fp32 chunked library path is within 4.1e-7 of float64 and a strictly sequential fp32 chain over 8192-row slabs
within 1.0e-6 (measured on the CPU), so ``helpers.REL_TOL`` = 1e-4 has two orders of room and no case is exempt.

Measured margins (MI355X): profiles/mlp_wgrad.md."""
import copy
import ctypes

import pytest
import torch

from freegaussian_amd import _lib
from freegaussian_amd import deform as D
from freegaussian_amd import ops
from helpers import REL_TOL, rel_err
from mlp_common import GUARD, NAN, arena, flat, grad_names, lib_calls, module_inputs, module_step, named_grads, out_shapes
from mlp_inputs_common import BLENDER_TIME, clear_inputs, float64_with_input_row, make_net
from mlp_train_common import aux_of, cotangents, head_rows, heads_of, manual_float64, rows_clear_of_the_kink

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK = D._TallLinear.CHUNK
N_MAX = 33_000
ROWS4 = (3, 3, 4, 3)


def _slab(n):
    return ops.mlp_wgrad_slab_rows(n)


# every size with (21, ROWS4) and (30, ROWS4); 511..513: where the cut goes from one slab to two; and each multi-slab
# size's own slab length +- 1 (one slab and a row either way)
_BASE = [1, 2, 63, 64, 65, 129, 511, 512, 513, 8191, 8192, 8193, 3 * CHUNK + 65, N_MAX]


def _sizes():
    lib = _lib.load()
    extra = set()
    for n in (8193, 3 * CHUNK + 65, N_MAX):
        s = int(lib.fg_mlp_param_grads_slab_rows(n))
        extra |= {s - 1, s, s + 1}
    return sorted(set(_BASE) | extra)


SIZES = _sizes()
AUX_WIDTHS = [1, 21, 30, 63, 64]  # in_ch 64, 84, 93, 126, 127: no pad, a pad of 4, an odd row stride and a pad of 3, ...
HEAD_ROWS = [ROWS4, (3, 4, 3), (16,), (1,)]

_ARRAYS = {}


def _arrays(A):
    """(enc, H, G, g_heads [rows, 16]) for aux width A on the CPU in float32; made once, never changed.  N_MAX rows for the
    two widths every size runs with, 8193 for the others."""
    if A not in _ARRAYS:
        g = torch.Generator().manual_seed(100 + A)
        rows = N_MAX if A in (21, 30) else 8193
        enc = torch.rand(rows, _lib.mlp_enc_width(A), generator=g) * 2 - 1
        enc[:, 63 + A :] = 0.0  # (as fg_mlp_train_fwd leaves the pad)
        H = torch.relu(torch.randn(8, rows, 256, generator=g))
        G = torch.randn(8, rows, 256, generator=g) * (torch.rand(8, rows, 256, generator=g) < 0.5) * 1e-3
        gh = torch.randn(rows, 16, generator=g) * 1e-3
        _ARRAYS[A] = (enc, H, G, gh)
    return _ARRAYS[A]


def _case(A, rows, n):
    enc, H, G, gh = _arrays(A)
    return enc[:n].contiguous(), H[:, :n].contiguous(), G[:, :n].contiguous(), gh[:n, : sum(rows)].contiguous()


_WANT = {}


def _float64(A, rows, n):
    """deform.mlp_param_grads of the case in float64 on the CPU, as one flat list in ``_MlpTrain``'s parameter order."""
    key = (A, tuple(rows), n)
    if key not in _WANT:
        enc, H, G, gh = (t.double() for t in _case(A, rows, n))
        gW, gb, gWh, gbh = D.mlp_param_grads(enc[:, : 63 + A], H, G, gh, rows)
        _WANT[key] = [*gW, *gb, *gWh, *gbh]
    return _WANT[key]


def _run(A, rows, n, want=None):
    dev = [t.to(DEV) for t in _case(A, rows, n)]
    return flat(ops.mlp_param_grads(*dev, A, rows, want=want))


def _check(tag, got, want, rows):
    worst = {}
    for name, g, w in zip(grad_names(rows), got, want):
        assert g.shape == w.shape and g.dtype == torch.float32, name
        assert bool(torch.isfinite(g).all()), name
        err = rel_err(g, w)
        worst[name.split("[")[0]] = max(worst.get(name.split("[")[0], 0.0), err)
        assert err < REL_TOL, (tag, name, err)
    print(f"mlp_wgrad {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ---- 1. parity against float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("A", [21, 30])
def test_every_size_against_float64(A, n):
    _check(f"A={A} n={n}", _run(A, ROWS4, n), _float64(A, ROWS4, n), ROWS4)


@pytest.mark.parametrize("n", [65, 8193])
@pytest.mark.parametrize("rows", HEAD_ROWS)
@pytest.mark.parametrize("A", AUX_WIDTHS)
def test_every_aux_width_and_head_set_against_float64(A, rows, n):
    got = _run(A, rows, n)
    assert got[0].shape == (256, 63 + A) and got[5].shape == (256, 63 + A + 256)
    _check(f"A={A} rows={rows} n={n}", got, _float64(A, rows, n), rows)


# ---- 2. only what is asked for is written, only what belongs is read -----------------------------------------------------
def _entry_point(A, rows, n, want=None):
    """fg_mlp_param_grads on inputs and outputs carved from NaN-filled arenas: NaN in enc's pad columns and directly behind
    acts[7, n - 1], g_pre[7, n - 1] and g_heads[n - 1] (the guard bands).  Returns (outputs, arenas of the outputs)."""
    k = len(rows)
    want = [True] * (16 + 2 * k) if want is None else want
    ins = [arena(*t.shape) for t in _case(A, rows, n)]
    for (flat, view), t in zip(ins, _case(A, rows, n)):
        view.copy_(t)
    ins[0][1][:, 63 + A :] = NAN
    before = [flat.clone() for flat, _ in ins]
    outs = [arena(*s) for s in out_shapes(A, rows)]
    d, g = _lib.MlpDesc(), _lib.MlpGrads()
    d.size, d.mode, d.depth, d.width, d.multires = ctypes.sizeof(_lib.MlpDesc), _lib.MLP_PLAIN, 8, 256, 10
    d.aux_width, d.n_heads, g.size = A, k, ctypes.sizeof(_lib.MlpGrads)
    for i, r in enumerate(rows):
        d.head_rows[i] = r
    ptr = lambda i: outs[i][1].data_ptr() if want[i] else None  # noqa: E731
    for i in range(8):
        g.weight[i], g.bias[i] = ptr(i), ptr(8 + i)
    for i in range(k):
        g.head_weight[i], g.head_bias[i] = ptr(16 + i), ptr(16 + k + i)
    ws_flat, ws = arena(int(_lib.load().fg_mlp_param_grads_workspace_bytes(n)) // 4)
    ops._call("fg_mlp_param_grads", n, ctypes.addressof(d), *(view.data_ptr() for _, view in ins), ctypes.addressof(g),
              ws.data_ptr(), ws.numel() * 4, ops._stream())  # fmt: skip
    torch.cuda.synchronize()
    for (flat, _), was in zip(ins, before):  # inputs are inputs: bit for bit what they were, NaN included
        assert torch.equal(flat.view(torch.int32), was.view(torch.int32))
    for flat in [f for f, _ in outs] + [ws_flat]:
        assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())
    return [view for _, view in outs], outs


@pytest.mark.parametrize("n", [1, 65, 8193])
def test_guarded_buffers(n):
    A = 30
    got, _ = _entry_point(A, ROWS4, n)
    _check(f"guarded A={A} n={n}", got, _float64(A, ROWS4, n), ROWS4)
    # the same bits as through ops (whose enc has zeros where this one has NaN)
    for a, b in zip(got, _run(A, ROWS4, n)):
        assert torch.equal(a, b)


# ---- 3. nullable outputs ------------------------------------------------------------------------------------------------
def _left_out():
    k = len(ROWS4)
    every = list(range(16 + 2 * k))
    return {"all weights": list(range(8)), "all biases": list(range(8, 16)), "one head's weight": [16 + 2], "layer 5's weight": [5],
            "all head weights": list(range(16, 16 + k)), "everything but one bias": [i for i in every if i != 8 + 3],
            "everything but one head bias": [i for i in every if i != 16 + k + 1]}  # fmt: skip


@pytest.mark.parametrize("group", list(_left_out()))
def test_nullable_outputs(group):
    A, n = 30, 129
    full = _run(A, ROWS4, n)
    skipped = _left_out()[group]
    want = [i not in skipped for i in range(len(full))]
    got, arenas = _entry_point(A, ROWS4, n, want)
    for i, (g, f) in enumerate(zip(got, full)):
        if want[i]:
            assert torch.equal(g, f), (group, i)
        else:
            assert bool(torch.isnan(arenas[i][0]).all()), (group, i)  # the stand-in of a skipped gradient: untouched
    through_ops = _run(A, ROWS4, n, want=want)
    for i, (g, f) in enumerate(zip(through_ops, full)):
        assert (g is None) if not want[i] else torch.equal(g, f), (group, i)


# ---- 4. repeatability ---------------------------------------------------------------------------------------------------
def test_two_calls_are_bitwise_equal_whatever_else_runs():
    A, n = 30, 8193
    dev = [t.to(DEV) for t in _case(A, ROWS4, n)]
    first = flat(ops.mlp_param_grads(*dev, A, ROWS4))
    again = flat(ops.mlp_param_grads(*dev, A, ROWS4))
    side = torch.cuda.Stream()
    a, b = torch.randn(2048, 2048, device=DEV), torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # an unrelated kernel queued on another stream, sharing the device with the call
        for _ in range(4):
            a = a @ b
    busy = flat(ops.mlp_param_grads(*dev, A, ROWS4))
    torch.cuda.synchronize()
    for x, y, z in zip(first, again, busy):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_capture_and_replay_equal_the_eager_call():
    A, n = 30, 8193
    static = [t.to(DEV) for t in _case(A, ROWS4, n)]
    ops.mlp_param_grads(*static, A, ROWS4)  # (the library is loaded, the allocator warm)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = flat(ops.mlp_param_grads(*static, A, ROWS4))
    # other inputs, written in place: rows n .. 2 n of the same pool
    enc, H, G, gh = _arrays(A)
    fresh = [enc[n : 2 * n], H[:, n : 2 * n], G[:, n : 2 * n], gh[n : 2 * n, : sum(ROWS4)]]
    for s, f in zip(static, fresh):
        s.copy_(f.to(DEV))
    for out in captured:
        out.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    eager = flat(ops.mlp_param_grads(*static, A, ROWS4))
    for c, e in zip(captured, eager):
        assert bool(torch.isfinite(c).all()) and torch.equal(c, e)


# ---- 5. exact cases -----------------------------------------------------------------------------------------------------
def test_zero_cotangents_give_exact_zeros():
    A, n = 30, 8193
    enc, H, G, gh = (t.to(DEV) for t in _case(A, ROWS4, n))
    for out in flat(ops.mlp_param_grads(enc, H, torch.zeros_like(G), torch.zeros_like(gh), A, ROWS4)):
        assert bool((out == 0).all())


@pytest.mark.parametrize("n", [65, 3 * CHUNK + 65])
def test_a_single_one_lands_in_one_row_of_one_gradient(n):
    """H and enc all ones, G one 1 at (l, r, j): gW_l[j, :] = 1, gb_l[j] = 1 and exact zeros elsewhere, for r at either end and
    on both sides of every kind of slab boundary; the same for g_heads.  Pins the row range of every slab without a tolerance."""
    A, rows = 30, ROWS4
    s = _slab(n)
    places = sorted({0, n - 1} | ({s - 1, s, 2 * s - 1, 2 * s, (n - 1) // s * s - 1, (n - 1) // s * s} if n > s else set()))
    assert all(0 <= r < n for r in places)
    enc = torch.ones(n, _lib.mlp_enc_width(A), device=DEV)
    H, G = torch.ones(8, n, 256, device=DEV), torch.zeros(8, n, 256, device=DEV)
    gh = torch.zeros(n, sum(rows), device=DEV)
    for i, r in enumerate(places):
        l, j = (i * 3 + 5) % 8, (i * 67 + 129) % 256
        G[l, r, j] = 1.0
        out = flat(ops.mlp_param_grads(enc, H, G, gh, A, rows))
        G[l, r, j] = 0.0
        for k, t in enumerate(out):
            want = torch.zeros_like(t)
            if k == l or k == 8 + l:
                want[j] = 1.0
            assert torch.equal(t, want), (r, l, j, k)
        o = (i * 5 + 4) % sum(rows)  # head cotangent column o = row o of the stacked head gradients
        gh[r, o] = 1.0
        out = flat(ops.mlp_param_grads(enc, H, G, gh, A, rows))
        gh[r, o] = 0.0
        assert all(bool((t == 0).all()) for t in out[:16])
        assert torch.equal(torch.cat(out[16:20]), torch.zeros(13, 256, device=DEV).index_fill_(0, torch.tensor([o], device=DEV), 1.0))
        assert torch.equal(torch.cat(out[20:24]), torch.zeros(13, device=DEV).index_fill_(0, torch.tensor([o], device=DEV), 1.0))


def test_rows_are_matched_with_their_own_rows():
    """Asymmetric exact data: H[l, r, c] = (r + c) % 7 and enc[r, c] = (r + 2 c) % 5, G ones at a few (l, r, j): every gradient is a small
    integer, exact in fp32 whatever the order -- a transposed tile or a row paired with another row's input shows."""
    A, rows, n = 30, ROWS4, 8193
    r_idx, c_idx = torch.arange(n).view(n, 1), torch.arange(256).view(1, 256)
    H = ((r_idx + c_idx) % 7).float().expand(8, n, 256).contiguous()
    enc_w = _lib.mlp_enc_width(A)
    enc = ((r_idx + 2 * torch.arange(enc_w).view(1, enc_w)) % 5).float()
    g = torch.Generator().manual_seed(7)
    G = (torch.rand(8, n, 256, generator=g) < 0.01).float()
    gh = (torch.rand(n, sum(rows), generator=g) < 0.05).float()
    want = flat(D.mlp_param_grads(enc[:, : 63 + A].double(), H.double(), G.double(), gh.double(), rows))
    got = flat(ops.mlp_param_grads(enc.to(DEV), H.to(DEV), G.to(DEV), gh.to(DEV), A, rows))
    for k, (a, b) in enumerate(zip(got, want)):
        assert float(b.abs().max()) < 2**24 and torch.equal(a.cpu().double(), b), k


# ---- 6. through ops.mlp_train -------------------------------------------------------------------------------------------
@pytest.fixture
def spy(monkeypatch):
    """Calls of deform.mlp_param_grads, of ops.mlp_param_grads and of the library's fg_mlp_param_grads."""
    seen = {"torch": [], "ops": [], "lib": lib_calls(monkeypatch, ("fg_mlp_param_grads",))}
    real_torch, real_ops = D.mlp_param_grads, ops.mlp_param_grads
    monkeypatch.setattr(D, "mlp_param_grads", lambda *a: seen["torch"].append(a) or real_torch(*a))
    monkeypatch.setattr(ops, "mlp_param_grads", lambda *a, **k: seen["ops"].append((a, k)) or real_ops(*a, **k))
    return seen


def _train_step(m_dev, x, aux, g_heads, **kw):
    m_dev.zero_grad(set_to_none=True)
    raw = ops.mlp_train(x, aux, m_dev.linear, heads_of(m_dev), **kw)
    raw.backward(g_heads)
    return raw.detach(), named_grads(m_dev)


@pytest.mark.parametrize("n", [65, 3 * CHUNK + 65])
@pytest.mark.parametrize("kind", ["deform", "control", "blender"])
def test_through_mlp_train_against_float64(kind, n, spy):
    m = make_net(kind)
    if kind == "blender":  # aux = timenet's output per row, wanting a gradient; the float64 run with the input row
        x, aux = clear_inputs(m, n)
        g_heads = torch.randn(n, 13, generator=torch.Generator().manual_seed(3))
        want = float64_with_input_row(m, x, aux, g_heads)["grads"]
        want = {k: v for k, v in want.items() if v is not None}
        kw = dict(input_grads=True)
    else:
        x, other = (t[: n + n // 2 + 64] for t in module_inputs(kind, n + n // 2 + 64))
        ok = rows_clear_of_the_kink(m, x, other)
        assert int(ok.sum()) >= n
        x, other = x[ok][:n].contiguous(), other[ok][:n].contiguous()
        ref = manual_float64(m, x, other, cotangents(m, n))
        aux, g_heads, want, kw = aux_of(m, other), ref["g_heads"].float(), ref["grads"], {}
    m_dev = copy.deepcopy(m).to(DEV)
    xd, gd = x.to(DEV), g_heads.to(DEV)
    ad = aux.to(DEV).requires_grad_(True) if kind == "blender" else aux.to(DEV)
    raw_off, off = _train_step(m_dev, xd, ad, gd, **kw)
    assert (len(spy["torch"]), len(spy["ops"]), len(spy["lib"])) == (1, 0, 0)
    g_aux_off = ad.grad.clone() if kind == "blender" else None
    if kind == "blender":
        ad.grad = None
    raw_on, on = _train_step(m_dev, xd, ad, gd, fused_param_grads=True, **kw)
    assert (len(spy["torch"]), len(spy["ops"]), len(spy["lib"])) == (1, 1, 1)  # the fused call once, the library path not again
    args, kwargs = spy["ops"][0]
    assert args[0].shape == (n, _lib.mlp_enc_width(m.input_ch - 63)) and args[0].is_contiguous()  # enc whole: no column copy
    assert list(kwargs["want"]) == [True] * (16 + 2 * len(head_rows(m)))
    assert torch.equal(raw_on, raw_off)
    if kind == "blender":
        assert torch.equal(ad.grad, g_aux_off)  # (the rest of the backward is untouched)
    errs = {}
    for k, w in want.items():
        assert float(w.abs().max()) > 0, k
        errs[k] = (rel_err(on[k], w), rel_err(off[k], w))
    print(f"mlp_wgrad through mlp_train {kind} n={n}: worst fused {max(e[0] for e in errs.values()):.2e}, "
          f"library {max(e[1] for e in errs.values()):.2e}")  # fmt: skip
    assert len(errs) == 2 * (8 + len(head_rows(m)))
    for k, (e_on, e_off) in errs.items():
        assert e_on < REL_TOL and e_off < REL_TOL, (k, e_on, e_off)


# ---- 7. through the modules and the model -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,train", [("deform", "1"), ("control", "1"), ("blender", "2")])
def test_modules_with_the_knob_set_and_unset(kind, train, spy, monkeypatch):
    n = D.FUSED_MIN_ROWS + 65
    m = make_net(kind)
    # (both settings form their gradients from the same H and G, bit for bit: no row has to be kept clear of the ReLU's kink)
    x, other = module_inputs(kind, n, seed=4)
    if kind == "blender":
        other = torch.full((1, 1), BLENDER_TIME).expand(n, -1)
    m_dev = copy.deepcopy(m).to(DEV)
    xd, od, cots = x.to(DEV), other.to(DEV), [c.to(DEV) for c in cotangents(m, n)]
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", train)
    monkeypatch.delenv("FG_FUSED_MLP_WGRAD", raising=False)
    off = module_step(m_dev, xd, od, cots)
    assert (len(spy["torch"]), len(spy["lib"])) == (1, 0)
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD", "1")
    on = module_step(m_dev, xd, od, cots)
    assert (len(spy["torch"]), len(spy["lib"])) == (1, 1)
    errs = {k: rel_err(on[k], off[k]) for k in off}
    print(f"mlp_wgrad module {kind}: worst {max(errs.values()):.2e}")
    assert len(errs) == 2 * (8 + len(head_rows(m))) + (4 if kind == "blender" else 0)
    for k, e in errs.items():
        assert float(off[k].abs().max()) > 0 and e < REL_TOL, (k, e)
    # one head and one trunk bias frozen: no gradient for them, the others the same bits as when they were wanted
    frozen = [heads_of(m_dev)[1].weight, heads_of(m_dev)[1].bias, m_dev.linear[3].bias]
    for p in frozen:
        p.requires_grad_(False)
    part = module_step(m_dev, xd, od, cots)
    args, kwargs = spy["ops"][-1]
    k_heads = len(head_rows(m))
    assert [i for i, w in enumerate(kwargs["want"]) if not w] == [8 + 3, 16 + 1, 16 + k_heads + 1]
    names = {id(p): k for k, p in m_dev.named_parameters()}
    for k in on:
        if k in [names[id(p)] for p in frozen]:
            assert part[k] is None, k
        else:
            assert torch.equal(part[k], on[k]), k
    # without the training knob the new one does nothing
    monkeypatch.delenv("FG_FUSED_MLP_TRAIN")
    calls = len(spy["lib"])
    module_step(m_dev, xd, od, cots)
    assert len(spy["lib"]) == calls


def test_model_training_step_with_the_knob_set_and_unset(spy, monkeypatch):
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    n, W, H = D.FUSED_MIN_ROWS, 64, 48  # the smallest count that reaches the dispatch
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-3.8, is_blender=False)
    with torch.no_grad():
        model.gauss_params["scales"].normal_(-3.8, 0.3)
        model.gauss_params["features_rest"].normal_(0, 0.1)
        for q in model.deform.parameters():
            q.mul_(0.3)
    time = 0.4
    model.step = 4000  # behind warm_up: the deformation net runs
    model = model.to(DEV).train()
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1
    cam = Camera(c2w[None, :3], 56.0, 60.0, W / 2, H / 2, W, H, times=torch.tensor([[time]]))
    gt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(12)).to(DEV)
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "1")
    grads, losses = {}, {}
    for knob in ("1", None):
        monkeypatch.setenv("FG_FUSED_MLP_WGRAD", knob) if knob else monkeypatch.delenv("FG_FUSED_MLP_WGRAD")
        model.zero_grad(set_to_none=True)
        out = model.get_outputs(copy.deepcopy(cam))
        loss = model.get_loss_dict(out, {"image": gt})["main_loss"]
        loss.backward()
        losses[knob] = loss.detach().clone()
        grads[knob] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    assert (len(spy["lib"]), len(spy["torch"])) == (1, 1)  # one step each
    on, off = grads["1"], grads[None]
    # the forward is the same kernels on the same bits, and so is the backward's data chain: nothing needs the kink's rows moved
    assert torch.equal(losses["1"], losses[None]) and set(on) == set(off)
    deform = [k for k in on if k.startswith("deform.")]
    gauss = [k for k in on if k.startswith("gauss_params.")]
    assert len(deform) == 24 and len(gauss) >= 5
    errs = {k: rel_err(on[k], off[k]) for k in deform}
    print("mlp_wgrad model step: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in gauss:  # (the Gaussians' gradients do not pass through the parameter gradients)
        assert rel_err(on[k], off[k]) < REL_TOL, k
    for k in deform:
        assert float(off[k].abs().max()) > 0 and errs[k] < REL_TOL, (k, errs[k])
