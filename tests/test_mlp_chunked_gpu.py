"""GPU: the fused backward in row chunks (``fg_mlp_train_bwd`` / ``ops.mlp_train_backward`` /
``ops.mlp_train(..., chunked_backward=...)``) against the two calls it combines -- ``fg_mlp_bwd`` / ``fg_mlp_bwd_inputs``
followed by ``fg_mlp_param_grads`` -- bit for bit, for every way of cutting the slabs into chunks; with outputs left out; on
guarded buffers; against itself (repeatability, graph replay); once against float64; through the modules and the model with
``FG_FUSED_MLP_CHUNKED=1``; and what the backward allocates.

Inputs of the stand-alone tests (the generators of tests/test_mlp_wgrad_gpu.py where they apply): a default-initialised
trunk of the given aux width, ``x`` uniform in [-1, 1]^3, ``aux`` uniform in [-1, 1], ``g_heads = randn * 1e-3``, seeded; one
real forward (``fg_mlp_train_fwd``) of N_MAX rows per network gives ``enc`` and ``H`` as the chain expects them, every smaller
size is a prefix of it (the forward's rows are independent bit for bit).  The reference of a case is computed once and kept.

Measured (MI355X): profiles/mlp_chunked_bwd.md."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

from freegaussian_amd import _lib
from freegaussian_amd import deform as D
from freegaussian_amd import ops
from helpers import REL_TOL, rel_err
from mlp_common import GUARD, NAN, arena, flat, lib_calls, module_inputs, module_step, named_grads, out_shapes
from mlp_inputs_common import BLENDER_TIME, clear_inputs, float64_with_input_row, make_net
from mlp_train_common import cotangents, head_rows, heads_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS4 = (3, 3, 4, 3)


def _slab(n):
    return ops.mlp_wgrad_slab_rows(n)


def _slabs(n):
    return -(-n // _slab(n))


# 5000 rows are 10 slabs of 512; 5056 = 79 x 64 is a whole number of tiles, 5057 one row into a new tile; 20 000 rows are 32
# slabs of 640; and the slab length of either +- 1 (one slab and a row either way)
_BASE = [1, 63, 64, 65, 511, 512, 513, 5000, 5056, 5057]
SIZES = sorted(set(_BASE) | {20_000} | {s + k for s in (512, 640) for k in (-1, 0, 1)})
N_MAX = max(SIZES)

_NETS, _FWD, _REF = {}, {}, {}


def _net(A, rows):
    """(trunk, heads) on the device for aux width A and the head rows: default init, seeded."""
    key = (A, tuple(rows))
    if key not in _NETS:
        torch.manual_seed(10 + A)
        trunk = D._trunk(63 + A, 256, 8, 4)
        heads = nn.ModuleList([nn.Linear(256, r) for r in rows])
        _NETS[key] = (trunk.to(DEV), heads.to(DEV))
    return _NETS[key]


def _forward(A, rows):
    """(enc [N_MAX, .], H [8, N_MAX, 256], g_heads [N_MAX, sum(rows)]) on the device: made once, never changed."""
    key = (A, tuple(rows))
    if key not in _FWD:
        trunk, heads = _net(A, rows)
        g = torch.Generator().manual_seed(100 + A)
        n = N_MAX if A in (21, 30) else 5000
        x = (torch.rand(n, 3, generator=g) * 2 - 1).to(DEV)
        aux = (torch.rand(n, A, generator=g) * 2 - 1).to(DEV)
        gh = (torch.randn(n, sum(rows), generator=g) * 1e-3).to(DEV)
        d, _, _, keep = ops._mlp_desc("test", x, aux, trunk, heads, _lib.MLP_PLAIN)
        out = torch.empty(n, sum(rows), device=DEV)
        enc, H = torch.empty(n, _lib.mlp_enc_width(A), device=DEV), torch.empty(8, n, 256, device=DEV)
        ws = torch.empty(int(_lib.load().fg_mlp_train_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
        ops._call("fg_mlp_train_fwd", n, ctypes.addressof(d), out.data_ptr(), enc.data_ptr(), H.data_ptr(), ws.data_ptr(), ws.numel(),
                  ops._stream())  # fmt: skip
        torch.cuda.synchronize()
        assert float((H > 0).float().mean(dim=(1, 2)).min()) > 0.05  # a live network: no layer is dead
        _FWD[key] = (enc, H, gh)
    return _FWD[key]


def _case(A, rows, n):
    enc, H, gh = _forward(A, rows)
    return enc[:n].contiguous(), H[:, :n].contiguous(), gh[:n].contiguous()


def _two_calls(A, rows, n, g_enc, want=None):
    """``fg_mlp_bwd`` (``fg_mlp_bwd_inputs`` where ``g_enc``) into a whole G, then ``ops.mlp_param_grads``:
    (flat gradients, g_enc or None)."""
    enc, H, gh = _case(A, rows, n)
    trunk, heads = _net(A, rows)
    d, _, _, keep = ops._mlp_desc("test", None, A, trunk, heads, _lib.MLP_PLAIN)
    G = torch.full_like(H, NAN)
    lib = _lib.load()
    if g_enc:
        ge = torch.full_like(enc, NAN)
        ws = torch.empty(int(lib.fg_mlp_bwd_inputs_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
        ops._call("fg_mlp_bwd_inputs", n, ctypes.addressof(d), gh.data_ptr(), H.data_ptr(), G.data_ptr(), ge.data_ptr(), ws.data_ptr(),
                  ws.numel(), ops._stream())  # fmt: skip
    else:
        ge = None
        ws = torch.empty(int(lib.fg_mlp_train_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
        ops._call("fg_mlp_bwd", n, ctypes.addressof(d), gh.data_ptr(), H.data_ptr(), G.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
    return flat(ops.mlp_param_grads(enc, H, G, gh, A, rows, want=want)), ge


def _reference(A, rows, n, g_enc):
    key = (A, tuple(rows), n, g_enc)
    if key not in _REF:
        grads, ge = _two_calls(A, rows, n, g_enc)
        assert all(bool(torch.isfinite(t).all()) for t in grads) and float(grads[0].abs().max()) > 0 and float(grads[7].abs().max()) > 0
        assert ge is None or (bool(torch.isfinite(ge).all()) and float(ge.abs().max()) > 0)
        _REF[key] = (grads, ge)
    return _REF[key]


def _chunked(A, rows, n, g_enc, chunk_slabs, want=None):
    enc, H, gh = _case(A, rows, n)
    trunk, heads = _net(A, rows)
    *grads4, ge = ops.mlp_train_backward(enc, H, gh, trunk, heads, A, rows, want=want, want_g_enc=g_enc, chunk_slabs=chunk_slabs)
    return flat(grads4), ge


def _chunkings(n):
    s = _slabs(n)
    return sorted({1, 3, s, 0, s + 7})


def _assert_same(tag, got, want):
    (grads, ge), (ref, ref_ge) = got, want
    assert len(grads) == len(ref)
    for i, (a, b) in enumerate(zip(grads, ref)):
        assert (a is None and b is None) or torch.equal(a, b), (tag, i)
    assert (ge is None and ref_ge is None) or torch.equal(ge, ref_ge), (tag, "g_enc")


# ---- 1. bit for bit against the two calls ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("A", [21, 30])
def test_every_size_and_chunking_equals_the_two_calls(A, n):
    assert _slabs(5000) == 10 and _slab(5000) == 512 and _slabs(20_000) == 32 and _slab(20_000) == 640
    for g_enc in (True, False):
        want = _reference(A, ROWS4, n, g_enc)
        assert len(want[0]) == 24
        for c in _chunkings(n):
            _assert_same((A, n, g_enc, c), _chunked(A, ROWS4, n, g_enc, c), want)


@pytest.mark.parametrize("A,rows", [(1, (16,)), (64, (1,)), (1, (1,)), (64, (16,))])
def test_other_aux_widths_and_head_sets_equal_the_two_calls(A, rows):
    n = 5000
    for g_enc in (True, False):
        want = _reference(A, rows, n, g_enc)
        assert len(want[0]) == 18 and want[0][0].shape == (256, 63 + A) and want[0][5].shape == (256, 63 + A + 256)
        for c in _chunkings(n):
            _assert_same((A, rows, g_enc, c), _chunked(A, rows, n, g_enc, c), want)


# ---- 2. outputs left out --------------------------------------------------------------------------------------------------
def _only():
    k = len(ROWS4)
    return {"only biases": list(range(8, 16)), "only head gradients": list(range(16, 16 + 2 * k)), "only weight[5]": [5], "nothing": []}


@pytest.mark.parametrize("group", list(_only()))
@pytest.mark.parametrize("g_enc", [True, False])
def test_outputs_left_out(group, g_enc):
    A, n = 30, 5000
    want = [i in _only()[group] for i in range(24)]
    ref = _two_calls(A, ROWS4, n, g_enc, want=want)
    full = _reference(A, ROWS4, n, g_enc)
    for i, w in enumerate(want):  # (the two-call path under the same want: the wanted ones are the full run's)
        assert (ref[0][i] is None) if not w else torch.equal(ref[0][i], full[0][i])
    for c in (1, 3, 0):
        got = _chunked(A, ROWS4, n, g_enc, c, want=want)
        assert [t is None for t in got[0]] == [not w for w in want]
        _assert_same((group, g_enc, c), got, ref)
    if group == "nothing" and not g_enc:  # nothing at all: no launch, FG_OK
        assert all(t is None for t in got[0]) and got[1] is None


# ---- 3. guarded buffers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g_enc", [True, False])
def test_guarded_buffers(g_enc):
    """Every array in an allocation of its own between NaN bands: enc, acts and g_heads end at row N - 1 (what follows them is
    NaN, as are enc's pad columns), g_enc, the outputs and the workspace must keep their bands, and every result is the
    unguarded run's."""
    A, rows, n, c = 30, ROWS4, 5000, 3
    k = len(rows)
    ins = [arena(*t.shape) for t in _case(A, rows, n)]
    for (_, view), t in zip(ins, _case(A, rows, n)):
        view.copy_(t)
    ins[0][1][:, 63 + A :] = NAN
    before = [flat.clone() for flat, _ in ins]
    (_, enc), (_, H), (_, gh) = ins
    outs = [arena(*s) for s in out_shapes(A, rows)]
    ge_flat, ge = arena(n, _lib.mlp_enc_width(A))
    trunk, heads = _net(A, rows)
    d, _, _, keep = ops._mlp_desc("test", None, A, trunk, heads, _lib.MLP_PLAIN)
    g = _lib.MlpGrads()
    g.size = ctypes.sizeof(_lib.MlpGrads)
    for i in range(8):
        g.weight[i], g.bias[i] = outs[i][1].data_ptr(), outs[8 + i][1].data_ptr()
    for i in range(k):
        g.head_weight[i], g.head_bias[i] = outs[16 + i][1].data_ptr(), outs[16 + k + i][1].data_ptr()
    need = int(_lib.load().fg_mlp_train_bwd_workspace_bytes(n, c, int(g_enc)))
    assert need % 4 == 0
    ws_flat, ws = arena(need // 4)
    ops._call("fg_mlp_train_bwd", n, ctypes.addressof(d), gh.data_ptr(), enc.data_ptr(), H.data_ptr(), ge.data_ptr() if g_enc else None,
              ctypes.addressof(g), c, ws.data_ptr(), need, ops._stream())  # fmt: skip
    torch.cuda.synchronize()
    for (flat, _), was in zip(ins, before):  # inputs are inputs: bit for bit what they were, NaN included
        assert torch.equal(flat.view(torch.int32), was.view(torch.int32))
    for flat in [f for f, _ in outs] + [ws_flat, ge_flat]:
        assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())
    if not g_enc:
        assert bool(torch.isnan(ge_flat).all())  # not asked for: not touched
    _assert_same(("guarded", g_enc), ([view for _, view in outs], ge if g_enc else None), _reference(A, rows, n, g_enc))


# ---- 4. repeatability -----------------------------------------------------------------------------------------------------
def test_two_calls_are_bitwise_equal():
    A, n = 30, 5000
    first = _chunked(A, ROWS4, n, True, 3)
    again = _chunked(A, ROWS4, n, True, 3)
    _assert_same("again", again, first)


@pytest.fixture
def spy(monkeypatch):
    """The library calls of the backward, by name."""
    return lib_calls(monkeypatch, ("fg_mlp_train_bwd", "fg_mlp_bwd", "fg_mlp_bwd_inputs", "fg_mlp_param_grads"))


def test_capture_and_replay_equal_the_eager_call(spy):
    n = 5000
    m = make_net("blender").to(DEV)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(n, 3, generator=g) * 2 - 1).to(DEV).requires_grad_(True)
    aux = (torch.rand(1, 30, generator=g) * 2 - 1).to(DEV).requires_grad_(True)  # one row for all: its column sum is captured too
    g_heads = (torch.randn(n, 13, generator=g) * 1e-3).to(DEV)

    def step():
        m.zero_grad(set_to_none=True)
        x.grad = aux.grad = None
        raw = ops.mlp_train(x, aux, m.linear, heads_of(m), input_grads=True, fused_param_grads=True, chunked_backward=3)
        raw.backward(g_heads)
        return raw.detach()

    raw_e = step().clone()
    assert spy == ["fg_mlp_train_bwd"]
    eager = dict(g_x=x.grad.clone(), g_aux=aux.grad.clone(), params={k: v for k, v in named_grads(m).items() if v is not None})
    assert len(eager["params"]) == 24 and float(eager["g_x"].abs().max()) > 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_s = step()
    params = {k: p for k, p in m.named_parameters() if p.grad is not None}
    assert set(params) == set(eager["params"])
    for _ in range(2):
        for buf in (raw_s, x.grad, aux.grad, *(p.grad for p in params.values())):
            buf.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(raw_s, raw_e) and torch.equal(x.grad, eager["g_x"]) and torch.equal(aux.grad, eager["g_aux"])
        for k, p in params.items():
            assert torch.equal(p.grad, eager["params"][k]), k


# ---- 5. float64 -----------------------------------------------------------------------------------------------------------
def test_blender_net_through_mlp_train_against_float64(spy):
    n = 5000
    m = make_net("blender")
    x, aux = clear_inputs(m, n)  # rows clear of the ReLU's kink
    g_heads = torch.randn(n, 13, generator=torch.Generator().manual_seed(3))
    ref = float64_with_input_row(m, x, aux, g_heads)
    want = {k: v for k, v in ref["grads"].items() if v is not None}
    m_dev = copy.deepcopy(m).to(DEV)
    xd, ad = x.to(DEV).requires_grad_(True), aux.to(DEV).requires_grad_(True)
    raw = ops.mlp_train(xd, ad, m_dev.linear, heads_of(m_dev), input_grads=True, fused_param_grads=True, chunked_backward=3)
    raw.backward(g_heads.to(DEV))
    assert spy == ["fg_mlp_train_bwd"]
    got = named_grads(m_dev)
    errs = {k: rel_err(got[k], w) for k, w in want.items()}
    errs["g_x"], errs["g_aux"], errs["raw"] = rel_err(xd.grad, ref["g_x"]), rel_err(ad.grad, ref["g_aux"]), rel_err(raw, ref["raw"])
    print("mlp_chunked blender n=5000 chunk_slabs=3 against float64: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert len(want) == 24 and all(float(w.abs().max()) > 0 for w in want.values())
    for k, e in errs.items():
        assert e < REL_TOL, (k, e)


# ---- 6. through the modules and the model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,train", [("deform", "1"), ("control", "1"), ("blender", "2"), ("deform", "2")])
def test_modules_with_the_knob_set_and_unset(kind, train, spy, monkeypatch):
    n = D.FUSED_MIN_ROWS
    m = make_net(kind)
    x, other = module_inputs(kind, n, seed=4)
    if kind == "blender":
        other = torch.full((1, 1), BLENDER_TIME).expand(n, -1)
    m_dev = copy.deepcopy(m).to(DEV)
    xd, od, cots = x.to(DEV), other.to(DEV), [c.to(DEV) for c in cotangents(m, n)]
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", train)
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD", "1")
    monkeypatch.delenv("FG_FUSED_MLP_CHUNKED", raising=False)
    off = module_step(m_dev, xd, od, cots)
    assert spy == ["fg_mlp_bwd_inputs" if kind == "blender" else "fg_mlp_bwd", "fg_mlp_param_grads"]
    monkeypatch.setenv("FG_FUSED_MLP_CHUNKED", "1")
    on = module_step(m_dev, xd, od, cots)
    assert spy[2:] == ["fg_mlp_train_bwd"]
    assert len(off) == 2 * (8 + len(head_rows(m))) + (4 if kind == "blender" else 0) and set(on) == set(off)
    for k in off:
        assert float(off[k].abs().max()) > 0 and torch.equal(on[k], off[k]), k
    # one head and one trunk bias frozen: no gradient for them, the others the same bits
    frozen = [heads_of(m_dev)[1].weight, heads_of(m_dev)[1].bias, m_dev.linear[3].bias]
    for p in frozen:
        p.requires_grad_(False)
    part = module_step(m_dev, xd, od, cots)
    names = {id(p): k for k, p in m_dev.named_parameters()}
    for k in on:
        assert (part[k] is None) if k in [names[id(p)] for p in frozen] else torch.equal(part[k], on[k]), k
    # without the parameter-gradient knob the new one does nothing
    monkeypatch.delenv("FG_FUSED_MLP_WGRAD")
    del spy[:]
    module_step(m_dev, xd, od, cots)
    assert "fg_mlp_train_bwd" not in spy and len(spy) == 1


def test_model_training_step_with_the_knob_set_and_unset(spy, monkeypatch):
    """The default (blender) model, one training step with the knob set and one with it unset: the loss and every gradient
    equal bit for bit.

    The render's backward adds into a splat's gradient with one float atomic per WAVEFRONT that has a contributing pixel, and
    two runs of it agree bit for bit only where no splat gets more than two such addends (0 + a + b = 0 + b + a; a third makes
    the order show: DESIGN.md, "atomic order").  An image of one 16 x 16 tile is one workgroup -- of FOUR wavefronts, four
    pixel rows each (the classic launch below 3000 tiles) -- so a splat gets one addend per 4-row strip it reaches, up to
    four.  This test used to draw its log-scales around -3.8: one of its 32 768 splats reached three strips, the step had two
    outcomes and the test failed one run in three (profiles/step_repeatability.md).  Around -5.2 the footprints are the
    0.3-pixel blur's, no splat reaches more than two strips -- counted below from the step's own records
    (tests/step_repeat_common.py ``addend_count``) -- and "equal" can be asked of everything."""
    import step_repeat_common as S

    model, cam, gt = S.make_step(DEV, S.SCALE_MEAN)
    n, W, H = model.num_points, S.W_STEP, S.H_STEP
    assert n == D.FUSED_MIN_ROWS  # the smallest count that reaches the dispatch
    rastered, real_raster = [], ops.rasterize_splats

    def raster(splats, means2d, channels, width, height, tile_size, offsets, ids, **kw):
        out = real_raster(splats, means2d, channels, width, height, tile_size, offsets, ids, **kw)
        rastered.append((splats.detach(), offsets, ids, out[2], width, height))
        return out

    monkeypatch.setattr(ops, "rasterize_splats", raster)
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "2")
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD", "1")
    grads, losses = {}, {}
    for knob in ("1", None):
        monkeypatch.setenv("FG_FUSED_MLP_CHUNKED", knob) if knob else monkeypatch.delenv("FG_FUSED_MLP_CHUNKED")
        model.zero_grad(set_to_none=True)
        out = model.get_outputs(copy.deepcopy(cam))
        loss = model.get_loss_dict(out, {"image": gt})["main_loss"]
        loss.backward()
        losses[knob] = loss.detach().clone()
        grads[knob] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    assert spy == ["fg_mlp_train_bwd", "fg_mlp_bwd_inputs", "fg_mlp_param_grads"]  # one step each
    # the census: both steps took the classic launch (no job lists at one tile), and no splat of either gets a third addend
    assert S.launch_of(W, H) == "classic" and int(_lib.load().fg_raster_jobs_words(W, H, 16, ops.current().cfg())) == 0
    assert len(rastered) >= 2
    for splats, offsets, ids, last_ids, w, h in rastered:
        assert (w, h) == (W, H)
        rec = splats.cpu()
        addends = S.addend_count(n, *S.strip_hits(rec[:, 0:2], rec[:, 3:6], rec[:, 2], offsets, ids, last_ids, W, H), S.groups_classic(1))
        census = S.census(addends)
        assert census["max"] <= 2, census
    assert census["1"] > 0 and census["2"] > 0, census  # (addends do meet: the order is exercised, and cannot show)
    on, off = grads["1"], grads[None]
    assert torch.equal(losses["1"], losses[None]) and set(on) == set(off)
    deform = [k for k in on if k.startswith("deform.")]
    assert len(deform) == 28 and len([k for k in on if k.startswith("gauss_params.")]) >= 5
    for k in on:
        assert torch.equal(on[k], off[k]), k
    for k in deform:
        assert float(off[k].abs().max()) > 0, k


# ---- 7. what the backward allocates ---------------------------------------------------------------------------------------
def test_the_backward_allocates_no_second_activation_sized_array():
    """65 536 rows are 32 slabs of 2048.  Chunks of 2 slabs: a workspace of 104 MB (34 MB of chunk array, 68 MB of partial
    blocks, the packed weights), g_enc of 25 MB and the gradients -- under half of G [8, N, 256] = 512 MB, which the unchunked
    backward allocates whole.  Both bounds are array sizes, not measurements."""
    n = 65_536
    assert _slab(n) == 2048 and _slabs(n) == 32
    m = make_net("blender").to(DEV)
    g = torch.Generator().manual_seed(6)
    x = (torch.rand(n, 3, generator=g) * 2 - 1).to(DEV)
    aux = (torch.rand(n, 30, generator=g) * 2 - 1).to(DEV).requires_grad_(True)
    g_heads = (torch.randn(n, 13, generator=g) * 1e-3).to(DEV)
    array = 8 * 256 * 4 * n
    peaks = {}
    for chunked in (2, False):
        m.zero_grad(set_to_none=True)
        aux.grad = None
        raw = ops.mlp_train(x, aux, m.linear, heads_of(m), input_grads=True, fused_param_grads=True, chunked_backward=chunked)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        raw.backward(g_heads)
        torch.cuda.synchronize()
        peaks[chunked] = torch.cuda.max_memory_allocated() - before
        del raw
    print(f"mlp_chunked backward peak above the level before it, n={n}: chunked {peaks[2] / 2**20:.1f} MiB, "
          f"unchunked {peaks[False] / 2**20:.1f} MiB (G = {array / 2**20:.0f} MiB)")  # fmt: skip
    assert peaks[2] < array // 2, peaks
    assert peaks[False] >= array, peaks
