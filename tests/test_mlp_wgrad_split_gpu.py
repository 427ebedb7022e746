"""GPU: the split-bf16 mode of the fused parameter-gradient products (``fg_mlp_param_grads_p`` / ``fg_mlp_train_bwd_p``,
``ops.mlp_param_grads(precision="bf16x3")``; the contract in include/fgraster.h) on random arrays against
``deform.mlp_param_grads`` of the same arrays in float64, on constructed cases that are exact for the three-term product
and for no other, beside the fp32 mode, on guarded buffers, with outputs left out, against itself (repeatability, graph
replay), chunked (``ops.mlp_train_backward(param_grads_precision="bf16x3")``), and through ``ops.mlp_train`` and the modules
with ``FG_FUSED_MLP_WGRAD_PRECISION=bf16x3``.

Inputs of the stand-alone tests: the recipe of tests/test_mlp_wgrad_gpu.py restated -- ``H = relu(randn)``,
``G = randn * (rand < 0.5) * 1e-3``, ``enc`` uniform in [-1, 1], ``g_heads = randn * 1e-3``, seeded, one pool per aux width,
every size a prefix of it.  On these the three-term product emulated on the CPU sits at 4.3e-6 .. 9.1e-6 of float64 and the
two-term one at 1.7e-3 .. 2.7e-3, so ``helpers.REL_TOL`` = 1e-4 has an order of room and no case is exempt.

Measured margins (MI355X): profiles/mlp_wgrad_split.md."""
import copy
import ctypes

import pytest
import torch

from freegaussian_amd import _lib
from freegaussian_amd import deform as D
from freegaussian_amd import ops
from helpers import REL_TOL, rel_err
from mlp_common import GUARD, NAN, arena, flat, grad_names, lib_calls, module_inputs, module_step, out_shapes, train_step
from mlp_inputs_common import BLENDER_TIME, make_net
from mlp_split_common import ROWS, case, split
from mlp_train_common import cotangents, head_rows, heads_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_MAX = 33_000
ROWS4 = (3, 3, 4, 3)
SPLIT = "bf16x3"


def _slab(n):
    return ops.mlp_wgrad_slab_rows(n)


def _sizes():
    s = int(_lib.load().fg_mlp_param_grads_slab_rows(8193))
    return sorted({1, 15, 16, 17, 63, 64, 65, 129, 511, 512, 513, 8193, s - 1, s, s + 1})


SIZES = _sizes()
AUX_WIDTHS = [1, 21, 30, 63, 64]
HEAD_ROWS = [ROWS4, (3, 4, 3), (16,), (1,)]

_ARRAYS, _WANT = {}, {}


def _arrays(A):
    """(enc, H, G, g_heads [rows, 16]) for aux width A on the CPU in float32; made once, never changed.  N_MAX rows for
    the one width that runs at that size, 2 x 8193 for the others (the graph test takes a second set of rows)."""
    if A not in _ARRAYS:
        g = torch.Generator().manual_seed(100 + A)
        rows = N_MAX if A == 21 else 2 * 8193
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


def _float64(A, rows, n):
    """deform.mlp_param_grads of the case in float64 on the CPU, as one flat list in ``_MlpTrain``'s parameter order."""
    key = (A, tuple(rows), n)
    if key not in _WANT:
        enc, H, G, gh = (t.double() for t in _case(A, rows, n))
        gW, gb, gWh, gbh = D.mlp_param_grads(enc[:, : 63 + A], H, G, gh, rows)
        _WANT[key] = [*gW, *gb, *gWh, *gbh]
    return _WANT[key]


def _run(A, rows, n, want=None, precision=SPLIT):
    dev = [t.to(DEV) for t in _case(A, rows, n)]
    return flat(ops.mlp_param_grads(*dev, A, rows, want=want, precision=precision))


def _check(tag, got, want, rows):
    worst = {}
    for name, g, w in zip(grad_names(rows), got, want):
        assert g.shape == w.shape and g.dtype == torch.float32, name
        assert bool(torch.isfinite(g).all()), name
        err = rel_err(g, w)
        worst[name.split("[")[0]] = max(worst.get(name.split("[")[0], 0.0), err)
    print(f"mlp_wgrad_split {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, g, w in zip(grad_names(rows), got, want):
        assert rel_err(g, w) < REL_TOL, (tag, name, rel_err(g, w))


# ---- 1. parity against float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("A", [21, 30])
def test_every_size_against_float64(A, n):
    _check(f"A={A} n={n}", _run(A, ROWS4, n), _float64(A, ROWS4, n), ROWS4)


def test_many_slabs_against_float64():
    _check(f"A=21 n={N_MAX}", _run(21, ROWS4, N_MAX), _float64(21, ROWS4, N_MAX), ROWS4)


@pytest.mark.parametrize("n", [65, 8193])
@pytest.mark.parametrize("rows", HEAD_ROWS)
@pytest.mark.parametrize("A", AUX_WIDTHS)
def test_every_aux_width_and_head_set_against_float64(A, rows, n):
    got = _run(A, rows, n)
    assert got[0].shape == (256, 63 + A) and got[5].shape == (256, 63 + A + 256)
    _check(f"A={A} rows={rows} n={n}", got, _float64(A, rows, n), rows)


# ---- 2. identities that hold for the three-term product alone -----------------------------------------------------------
N3 = 1025  # three slabs of 384 rows


def _hi_plus_lo(v):
    hi, lo = split(v)
    return hi + lo


def _dense(A, n, seed):
    """Operands of normal magnitude without a zero: |v| in [0.25, 1.25), signs mixed (enc, H, P alike)."""
    g = torch.Generator().manual_seed(seed)
    draw = lambda *s: (torch.rand(*s, generator=g) + 0.25) * (torch.randint(0, 2, s, generator=g) * 2 - 1).float()  # noqa: E731
    enc = draw(n, _lib.mlp_enc_width(A))
    enc[:, 63 + A :] = 0.0
    return enc.to(DEV), draw(8, n, 256).to(DEV), draw(8, n, 256).to(DEV)


def _input_row(l, r, enc, H, in_ch):
    if l == 0:
        return enc[r, :in_ch]
    return torch.cat([enc[r, :in_ch], H[4, r]]) if l == 5 else H[l - 1, r]


def test_a_single_one_in_the_cotangents_returns_hi_plus_lo_of_the_input_row():
    """G a single 1.0 at (l, r, i): P_hi = 1, P_lo = 0, so row i of gW_l is in_hi[r] + in_lo[r] exactly (the fp32 mode returns
    in[r] itself, a two-term kernel in_hi[r]); every other row, and every other weight gradient, is exact zeros.  Rows of the
    first and of a later slab, at every offset kind inside a 16-row step; layers 0 and 5 are the enc products."""
    A, n, in_ch = 30, N3, 93
    s = _slab(n)
    assert -(-n // s) == 3
    enc, H, _ = _dense(A, n, seed=11)
    G, gh = torch.zeros(8, n, 256, device=DEV), torch.zeros(n, sum(ROWS4), device=DEV)
    places = [(0, 37, 200), (0, s + 5, 3), (5, 0, 129), (5, n - 1, 255), (3, s - 1, 64), (3, 2 * s + 8, 0), (7, 15, 31), (1, s + 16, 127)]
    for l, r, i in places:
        G[l, r, i] = 1.0
        got = flat(ops.mlp_param_grads(enc, H, G, gh, A, ROWS4, precision=SPLIT))
        exact = flat(ops.mlp_param_grads(enc, H, G, gh, A, ROWS4))
        G[l, r, i] = 0.0
        row = _input_row(l, r, enc, H, in_ch)
        want = torch.zeros_like(got[l])
        want[i] = _hi_plus_lo(row)
        assert torch.equal(got[l], want), (l, r, i)
        assert not torch.equal(want[i], row) and not torch.equal(want[i], split(row)[0])  # the case tells the three apart
        assert torch.equal(exact[l][i], row), (l, r, i)
        for k in range(8):
            if k != l:
                assert bool((got[k] == 0).all()), (l, r, i, k)
        bias = torch.zeros(256, device=DEV)
        bias[i] = 1.0
        assert torch.equal(got[8 + l], bias), (l, r, i)


def test_a_single_one_in_the_inputs_returns_hi_plus_lo_of_the_cotangent_row():
    """in_l a single 1.0 at (r, j): in_hi = 1, in_lo = 0, so column j of gW_l is P_hi[r] + P_lo[r] exactly; every other column
    is exact zeros.  H[l - 1] for the hidden products, enc for the input products of layers 0 and 5."""
    A, n, in_ch = 30, N3, 93
    s = _slab(n)
    _, _, G = _dense(A, n, seed=12)
    gh = torch.zeros(n, sum(ROWS4), device=DEV)
    enc, H = torch.zeros(n, _lib.mlp_enc_width(A), device=DEV), torch.zeros(8, n, 256, device=DEV)
    for l, r, j in [(1, 37, 200), (4, s + 5, 3), (5, 2 * s + 8, 129), (7, n - 1, 255), (2, s - 1, 0)]:
        H[l - 1, r, j] = 1.0
        got = flat(ops.mlp_param_grads(enc, H, G, gh, A, ROWS4, precision=SPLIT))
        exact = flat(ops.mlp_param_grads(enc, H, G, gh, A, ROWS4))
        H[l - 1, r, j] = 0.0
        col = j + (in_ch if l == 5 else 0)
        want = torch.zeros_like(got[l])
        want[:, col] = _hi_plus_lo(G[l, r])
        assert torch.equal(got[l], want), (l, r, j)
        assert not torch.equal(want[:, col], G[l, r]) and torch.equal(exact[l][:, col], G[l, r]), (l, r, j)
        for k in range(8):
            if k != l:
                assert bool((got[k] == 0).all()), (l, r, j, k)
    for r, j in [(37, 0), (s + 5, 62), (n - 1, in_ch - 1)]:  # enc: layers 0 and 5 at once
        enc[r, j] = 1.0
        got = flat(ops.mlp_param_grads(enc, H, G, gh, A, ROWS4, precision=SPLIT))
        enc[r, j] = 0.0
        for l in (0, 5):
            want = torch.zeros_like(got[l])
            want[:, j] = _hi_plus_lo(G[l, r])
            assert torch.equal(got[l], want), (l, r, j)
        for k in (1, 2, 3, 4, 6, 7):
            assert bool((got[k] == 0).all()), (r, j, k)


def test_rows_are_matched_with_their_own_rows():
    """The small-integer case of tests/test_mlp_wgrad_gpu.py: H[l, r, c] = (r + c) % 7, enc[r, c] = (r + 2 c) % 5, G ones at a
    few places.  Small integers split exactly (lo = 0), every gradient is a small integer: equal to float64 whatever the order."""
    A, rows, n = 30, ROWS4, 8193
    r_idx, c_idx = torch.arange(n).view(n, 1), torch.arange(256).view(1, 256)
    H = ((r_idx + c_idx) % 7).float().expand(8, n, 256).contiguous()
    enc_w = _lib.mlp_enc_width(A)
    enc = ((r_idx + 2 * torch.arange(enc_w).view(1, enc_w)) % 5).float()
    g = torch.Generator().manual_seed(7)
    G = (torch.rand(8, n, 256, generator=g) < 0.01).float()
    gh = (torch.rand(n, sum(rows), generator=g) < 0.05).float()
    want = flat(D.mlp_param_grads(enc[:, : 63 + A].double(), H.double(), G.double(), gh.double(), rows))
    got = flat(ops.mlp_param_grads(enc.to(DEV), H.to(DEV), G.to(DEV), gh.to(DEV), A, rows, precision=SPLIT))
    for k, (a, b) in enumerate(zip(got, want)):
        assert float(b.abs().max()) < 2**24 and torch.equal(a.cpu().double(), b), k


def test_zero_cotangents_give_exact_zeros():
    A, n = 30, 8193
    enc, H, G, gh = (t.to(DEV) for t in _case(A, ROWS4, n))
    for out in flat(ops.mlp_param_grads(enc, H, torch.zeros_like(G), torch.zeros_like(gh), A, ROWS4, precision=SPLIT)):
        assert bool((out == 0).all())


# ---- 3. beside the fp32 mode --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 8193])
def test_beside_the_fp32_mode(n):
    A = 30
    got, exact, want = _run(A, ROWS4, n), _run(A, ROWS4, n, precision="fp32"), _float64(A, ROWS4, n)
    k = len(ROWS4)
    for i in range(16, 16 + 2 * k):  # head weights and biases: the same jobs, the same code
        assert torch.equal(got[i], exact[i]), i
    for l in range(8):  # the mode is taken
        assert not torch.equal(got[l], exact[l]), l
    for l in range(8):  # fp32 sums of the unsplit P_l (in an order of their own)
        assert rel_err(got[8 + l], want[8 + l]) < REL_TOL, l
    errs = [max(rel_err(g[l], want[l]) for l in range(8)) for g in (got, exact)]
    print(f"mlp_wgrad_split beside fp32 n={n}: trunk weights split {errs[0]:.2e}, fp32 {errs[1]:.2e}")
    assert errs[1] < errs[0] < REL_TOL  # three bf16 terms keep 16 bits of each operand: not as close as fp32, well within the bar


# ---- 4. only what is asked for is written, only what belongs is read -----------------------------------------------------
def _entry_point(A, rows, n, want=None):
    """fg_mlp_param_grads_p (FG_MLP_BF16X3) on inputs and outputs carved from NaN-filled arenas: NaN in enc's pad columns and
    directly behind acts[7, n - 1], g_pre[7, n - 1] and g_heads[n - 1] (the guard bands).  Returns (outputs, their arenas)."""
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
    ops._call("fg_mlp_param_grads_p", n, ctypes.addressof(d), *(view.data_ptr() for _, view in ins), ctypes.addressof(g),
              _lib.MLP_BF16X3, ws.data_ptr(), ws.numel() * 4, ops._stream())  # fmt: skip
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
    for a, b in zip(got, _run(A, ROWS4, n)):  # the same bits as through ops (whose enc has zeros where this one has NaN)
        assert torch.equal(a, b)


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


# ---- 5. repeatability ---------------------------------------------------------------------------------------------------
def test_two_calls_are_bitwise_equal():
    A, n = 30, 8193
    dev = [t.to(DEV) for t in _case(A, ROWS4, n)]
    first = flat(ops.mlp_param_grads(*dev, A, ROWS4, precision=SPLIT))
    again = flat(ops.mlp_param_grads(*dev, A, ROWS4, precision=SPLIT))
    for x, y in zip(first, again):
        assert torch.equal(x, y)


def test_capture_and_replay_equal_the_eager_call():
    A, n = 30, 8193
    static = [t.to(DEV) for t in _case(A, ROWS4, n)]
    ops.mlp_param_grads(*static, A, ROWS4, precision=SPLIT)  # (the library is loaded, the allocator warm)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = flat(ops.mlp_param_grads(*static, A, ROWS4, precision=SPLIT))
    # other inputs, written in place: rows n .. 2 n of the same pool
    enc, H, G, gh = _arrays(A)
    fresh = [enc[n : 2 * n], H[:, n : 2 * n], G[:, n : 2 * n], gh[n : 2 * n, : sum(ROWS4)]]
    for s, f in zip(static, fresh):
        s.copy_(f.to(DEV))
    for out in captured:
        out.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    eager = flat(ops.mlp_param_grads(*static, A, ROWS4, precision=SPLIT))
    for c, e in zip(captured, eager):
        assert bool(torch.isfinite(c).all()) and torch.equal(c, e)


# ---- 6. the chunked call ------------------------------------------------------------------------------------------------
_CHAIN = {}


def _chain_case():
    """A live network (default init, seeded), its forward arrays over N3 rows and head cotangents, on the device."""
    if not _CHAIN:
        import torch.nn as nn

        A, n = 21, N3
        torch.manual_seed(31)
        trunk, heads = D._trunk(63 + A, 256, 8, 4).to(DEV), nn.ModuleList([nn.Linear(256, r) for r in ROWS4]).to(DEV)
        g = torch.Generator().manual_seed(131)
        x, aux = (torch.rand(n, 3, generator=g) * 2 - 1).to(DEV), (torch.rand(n, A, generator=g) * 2 - 1).to(DEV)
        gh = (torch.randn(n, sum(ROWS4), generator=g) * 1e-3).to(DEV)
        d, _, _, keep = ops._mlp_desc("test", x, aux, trunk, heads, _lib.MLP_PLAIN)
        out, enc, H = torch.empty(n, sum(ROWS4), device=DEV), torch.empty(n, _lib.mlp_enc_width(A), device=DEV), torch.empty(8, n, 256, device=DEV)
        ws = torch.empty(int(_lib.load().fg_mlp_train_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
        ops._call("fg_mlp_train_fwd", n, ctypes.addressof(d), out.data_ptr(), enc.data_ptr(), H.data_ptr(), ws.data_ptr(), ws.numel(),
                  ops._stream())  # fmt: skip
        torch.cuda.synchronize()
        _CHAIN.update(A=A, n=n, trunk=trunk, heads=heads, enc=enc, H=H, gh=gh)
    return _CHAIN


def _chain_then_products(chain, g_enc, wgrad):
    """``fg_mlp_bwd`` (``fg_mlp_bwd_inputs`` where ``g_enc``) under ``chain`` into a whole G, then ``ops.mlp_param_grads``."""
    c = _chain_case()
    A, n, enc, H, gh = c["A"], c["n"], c["enc"], c["H"], c["gh"]
    d, _, _, keep = ops._mlp_desc("test", None, A, c["trunk"], c["heads"], _lib.MLP_PLAIN)
    d.precision = ops._mlp_precision("test", chain)
    G, lib = torch.full_like(H, NAN), _lib.load()
    if g_enc:
        ge = torch.full_like(enc, NAN)
        ws = torch.empty(int(lib.fg_mlp_bwd_inputs_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
        ops._call("fg_mlp_bwd_inputs", n, ctypes.addressof(d), gh.data_ptr(), H.data_ptr(), G.data_ptr(), ge.data_ptr(), ws.data_ptr(),
                  ws.numel(), ops._stream())  # fmt: skip
    else:
        ge = None
        ws = torch.empty(int(lib.fg_mlp_train_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
        ops._call("fg_mlp_bwd", n, ctypes.addressof(d), gh.data_ptr(), H.data_ptr(), G.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
    return flat(ops.mlp_param_grads(enc, H, G, gh, A, ROWS4, precision=wgrad)), ge


@pytest.mark.parametrize("g_enc", [True, False])
@pytest.mark.parametrize("chain", ["fp32", SPLIT])
def test_the_chunked_call_equals_the_two_calls(chain, g_enc):
    c = _chain_case()
    assert -(-c["n"] // _slab(c["n"])) == 3
    want, want_ge = _chain_then_products(chain, g_enc, SPLIT)
    assert all(bool(torch.isfinite(t).all()) for t in want) and float(want[0].abs().max()) > 0 and float(want[7].abs().max()) > 0
    exact, _ = _chain_then_products(chain, g_enc, "fp32")
    assert not torch.equal(want[3], exact[3]) and torch.equal(want[16], exact[16])
    for chunk_slabs in (1, 2, 3):
        *grads4, ge = ops.mlp_train_backward(c["enc"], c["H"], c["gh"], c["trunk"], c["heads"], c["A"], ROWS4, want_g_enc=g_enc,
                                             chunk_slabs=chunk_slabs, precision=chain, param_grads_precision=SPLIT)  # fmt: skip
        for i, (a, b) in enumerate(zip(flat(grads4), want)):
            assert torch.equal(a, b), (chunk_slabs, i)
        assert (ge is None and want_ge is None) or torch.equal(ge, want_ge), chunk_slabs


# ---- 7. through ops.mlp_train -------------------------------------------------------------------------------------------
@pytest.fixture
def spy(monkeypatch):
    """The library calls by name."""
    return lib_calls(monkeypatch)


FORMS = {"two_calls": {"fused_param_grads": True},
         "chunked_1_inputs": {"fused_param_grads": True, "chunked_backward": 1, "input_grads": True}}  # fmt: skip


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind", ["deform", "control", "blender"])
def test_through_mlp_train_against_float64(kind, form, spy):
    c = case(kind)
    m, x, aux, gh = copy.deepcopy(c["m"]).to(DEV), c["x"].to(DEV), c["aux"].to(DEV), c["g_heads"].to(DEV)
    assert x.shape[0] == ROWS
    ref = c["ref"]
    want = {k: v for k, v in ref["grads"].items() if v is not None and not k.startswith("timenet")}
    new_name = "fg_mlp_train_bwd_p" if "chunked_backward" in FORMS[form] else "fg_mlp_param_grads_p"
    old_name = new_name[:-2]
    for chain in ("fp32", SPLIT):
        runs = {}
        for wgrad in ("fp32", SPLIT):
            del spy[:]
            runs[wgrad] = train_step(m, x, aux, gh, precision=chain, param_grads_precision=wgrad, **FORMS[form])
            assert (spy.count(new_name), spy.count(old_name)) == ((1, 0) if wgrad == SPLIT else (0, 1)), (chain, wgrad, spy)
            raw, grads, g_x, g_aux = runs[wgrad]
            assert set(grads) == set(want) and len(grads) == 2 * (8 + len(head_rows(m)))
            errs = {k: rel_err(grads[k], w) for k, w in want.items()}
            print(f"mlp_wgrad_split mlp_train {kind} {form} chain={chain} wgrad={wgrad}: worst {max(errs.values()):.2e}")
            for k, e in errs.items():
                assert e < REL_TOL, (chain, wgrad, k, e)
        (raw_a, grads_a, gx_a, ga_a), (raw_b, grads_b, gx_b, ga_b) = runs["fp32"], runs[SPLIT]
        assert torch.equal(raw_a, raw_b)  # the word touches nothing but the products
        if FORMS[form].get("input_grads"):
            assert torch.equal(gx_a, gx_b) and torch.equal(ga_a, ga_b)
        else:
            assert gx_a is None and gx_b is None and ga_a is None and ga_b is None
        names = dict((id(p), k) for k, p in m.named_parameters())
        trunk_w = [names[id(layer.weight)] for layer in m.linear]
        head_params = [names[id(p)] for hd in heads_of(m) for p in (hd.weight, hd.bias)]
        assert all(not torch.equal(grads_a[k], grads_b[k]) for k in trunk_w)
        assert all(torch.equal(grads_a[k], grads_b[k]) for k in head_params)


# ---- 8. through the modules ---------------------------------------------------------------------------------------------
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
    for name in ("FG_FUSED_MLP_PRECISION", "FG_FUSED_MLP_CHUNKED", "FG_FUSED_MLP_WGRAD_PRECISION"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", train)
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD", "1")
    off = module_step(m_dev, xd, od, cots)
    assert (spy.count("fg_mlp_param_grads"), spy.count("fg_mlp_param_grads_p")) == (1, 0)
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD_PRECISION", SPLIT)
    on = module_step(m_dev, xd, od, cots)
    assert (spy.count("fg_mlp_param_grads"), spy.count("fg_mlp_param_grads_p")) == (1, 1)
    errs = {k: rel_err(on[k], off[k]) for k in off}
    print(f"mlp_wgrad_split module {kind}: worst {max(errs.values()):.2e}")
    assert len(errs) == 2 * (8 + len(head_rows(m))) + (4 if kind == "blender" else 0)
    for k, e in errs.items():
        assert float(off[k].abs().max()) > 0 and e < REL_TOL, (k, e)
    assert not torch.equal(on["linear.2.weight"], off["linear.2.weight"])
    # one head and one trunk bias frozen: no gradient for them, the others the same bits as when they were wanted
    frozen = [heads_of(m_dev)[1].weight, heads_of(m_dev)[1].bias, m_dev.linear[3].bias]
    for p in frozen:
        p.requires_grad_(False)
    part = module_step(m_dev, xd, od, cots)
    assert spy.count("fg_mlp_param_grads_p") == 2
    names = {id(p): k for k, p in m_dev.named_parameters()}
    for k in on:
        if k in [names[id(p)] for p in frozen]:
            assert part[k] is None, k
        else:
            assert torch.equal(part[k], on[k]), k
    for p in frozen:
        p.requires_grad_(True)
    # without FG_FUSED_MLP_WGRAD the knob does nothing: the library products, the bits of the knob unset
    monkeypatch.delenv("FG_FUSED_MLP_WGRAD")
    calls = len(spy)
    with_knob = module_step(m_dev, xd, od, cots)
    assert "fg_mlp_param_grads_p" not in spy[calls:] and "fg_mlp_param_grads" not in spy[calls:]
    monkeypatch.delenv("FG_FUSED_MLP_WGRAD_PRECISION")
    without = module_step(m_dev, xd, od, cots)
    for k in without:
        assert torch.equal(with_knob[k], without[k]), k
