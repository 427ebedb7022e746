"""CPU checks of the fused MLP training path's host side: the C ABI of ``fg_mlp_train_fwd`` / ``fg_mlp_bwd`` (argument
validation and the workspace query; every call returns before a launch), ``ops.mlp_train``'s refusals, the dispatch
predicate, and the parameter-gradient assembly (``deform.mlp_param_grads``) in float64 against autograd through the modules."""
import ctypes

import pytest
import torch

from freegaussian_amd import _lib
from freegaussian_amd import deform as D
from freegaussian_amd import ops
from helpers import rel_err
from mlp_common import PTR, addr, desc, header_text
from mlp_train_common import assembled, cotangents, half_dead_, head_rows, loss_of, manual_float64

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
BIG = 1 << 40  # a workspace that would do (every call below is refused before a launch)


def _desc(*a, **kw):
    return desc(*a, inputs=True, **kw)


def _fwd(n, d, heads=PTR, enc=PTR, acts=PTR, ws=PTR, ws_bytes=0):
    return _lib.load().fg_mlp_train_fwd(n, addr(d), heads, enc, acts, ws, ws_bytes, None)


def _bwd(n, d, g_heads=PTR, acts=PTR, g_pre=PTR, ws=PTR, ws_bytes=0):
    return _lib.load().fg_mlp_bwd(n, addr(d), g_heads, acts, g_pre, ws, ws_bytes, None)


def test_header_constants_and_binding_agree():
    text = header_text()
    assert f"#define FG_ABI_VERSION {_lib.ABI_VERSION}" in text and _lib.ABI_VERSION >= 12
    assert "#define FG_MLP_ENC_WIDTH(aux_width) ((63 + (aux_width) + 7) / 8 * 8)" in text
    assert [_lib.mlp_enc_width(a) for a in (1, 2, 21, 63, 64)] == [64, 72, 88, 128, 128]
    for name in ("fg_mlp_train_workspace_bytes", "fg_mlp_train_fwd", "fg_mlp_bwd"):
        assert name in _lib.SIGNATURES and f"{name}(" in text
    # the inference entry points and the descriptor are what they were
    assert _lib.SIGNATURES["fg_mlp_fwd"][1] == [ctypes.c_int64, _lib.P, _lib.P, ctypes.c_size_t, _lib.P]
    assert ctypes.sizeof(_lib.MlpDesc) == 12 * 4 + 8 + (2 + 8 + 8 + 3 * _lib.MLP_MAX_HEADS) * 8


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_error_codes_without_gpu(call):
    assert call(0, None, None, None, None, None, 0) == OK  # N = 0: nothing to do, nothing is looked at
    assert call(0, _desc(A=0)) == OK
    assert call(-1, _desc()) == INVALID
    assert call(100, None) == INVALID
    assert call(100, _desc()) == WORKSPACE  # everything else about it is accepted
    assert call(100, _desc(A=63, rows=(3, 4, 3))) == WORKSPACE and call(100, _desc(A=1, rows=(16,))) == WORKSPACE
    assert call(100, _desc(mode=_lib.MLP_SE3)) == INVALID  # raw heads only
    for A in (0, 65):
        assert call(100, _desc(A=A)) == INVALID
    for rows in ((0,), (17,), (8, 9)):
        assert call(100, _desc(rows=rows)) == INVALID
    d = _desc()
    d.size -= 8
    assert call(100, d) == INVALID
    for field, value in (("depth", 6), ("width", 128), ("multires", 6)):
        d = _desc()
        setattr(d, field, value)
        assert call(100, d) == UNSUPPORTED, field
    # null parameters, with a workspace that would do
    for field, count in (("weight", 8), ("bias", 8), ("head_weight", 4), ("head_bias", 4)):
        for i in range(count):
            d = _desc()
            getattr(d, field)[i] = None
            assert call(100, d, ws_bytes=BIG) == INVALID, (field, i)
    # null buffers
    for i in range(3):
        bufs = [PTR] * 3
        bufs[i] = None
        assert call(100, _desc(), *bufs, ws_bytes=BIG) == INVALID, i
    # no workspace, one that is not 16-byte aligned, one a byte short
    assert call(100, _desc(), ws=None, ws_bytes=BIG) == INVALID
    assert call(100, _desc(), ws=PTR + 4, ws_bytes=BIG) == INVALID
    need = int(_lib.load().fg_mlp_train_workspace_bytes(100))
    assert call(100, _desc(), ws_bytes=need - 1) == WORKSPACE


def test_inputs_are_required_by_the_forward_only():
    for field in ("x", "aux"):
        d = _desc()
        setattr(d, field, None)
        assert _fwd(100, d, ws_bytes=BIG) == INVALID, field
        assert _bwd(100, d) == WORKSPACE  # (accepted: the backward reads neither)


def test_workspace_query_is_monotone_and_covers_both_layouts():
    lib = _lib.load()
    sizes = [int(lib.fg_mlp_train_workspace_bytes(n)) for n in (0, 1, 63, 64, 65, 1000, 33_000, 1_000_000, 1 << 33)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert int(lib.fg_mlp_train_workspace_bytes(-1)) == 0
    # the forward's packed weights, and the backward's: the hidden columns of layers 1..7 and 16 head rows
    assert sizes[1] >= int(lib.fg_mlp_workspace_bytes(1)) and sizes[1] >= 4 * 256 * (7 * 256 + 16)


def test_ops_refuses_cpu_tensors_and_bad_shapes():
    m = D.FreeGaussianDeformableModel()
    heads = (m.branch_w, m.branch_v, m.gaussian_rotation, m.gaussian_scaling)
    x, aux = torch.zeros(4, 3), torch.zeros(4, 21)
    with pytest.raises(ValueError):
        ops.mlp_train(x, aux, m.linear, heads)  # CPU tensors
    with pytest.raises(ValueError):
        ops.mlp_train(torch.zeros(4, 2), aux, m.linear, heads)
    with pytest.raises(ValueError):
        ops.mlp_train(torch.zeros(0, 3), torch.zeros(0, 21), m.linear, heads)
    with pytest.raises(ValueError):
        ops.mlp_train(x, aux, list(m.linear)[:7], heads)
    with pytest.raises(ValueError):
        ops.mlp_train(x, aux, m.linear, ())
    with pytest.raises(ValueError):
        ops.mlp_train(x.double(), aux.double(), m.linear, heads)


def _net(kind, weights):
    torch.manual_seed(0)
    m = D.FreeGaussianControllableModel() if kind == "control" else D.FreeGaussianDeformableModel()
    return half_dead_(m) if weights == "half_dead" else m


def _inputs(kind, n):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(n, 3, generator=g) * 2 - 1
    return x, (torch.randn(n, 3, generator=g) * 0.1 if kind == "control" else torch.rand(n, 1, generator=g))


@pytest.mark.parametrize("n", [200, 8192 + 65])
@pytest.mark.parametrize("kind,weights", [("deform", "default"), ("deform", "half_dead"), ("control", "default")])
def test_parameter_gradient_assembly_equals_autograd_in_float64(kind, weights, n):
    m = _net(kind, weights)
    x, other = _inputs(kind, n)
    cots = cotangents(m, n)
    ref = manual_float64(m, x, other, cots)
    if weights == "half_dead":
        dead = float((ref["H"] <= 0).double().mean())
        assert 0.3 < dead < 0.7, dead
    # autograd through the module itself
    m64 = _net(kind, weights).double()
    loss_of(m64(x.double(), other.double()), cots).backward()
    got = assembled(m64, D.mlp_param_grads(ref["inp"], ref["H"], ref["G"], ref["g_heads"], head_rows(m64)))
    want = {k: p.grad for k, p in m64.named_parameters()}
    assert set(got) == set(want) and len(got) == 2 * (8 + len(head_rows(m64)))
    for k in want:
        assert got[k].shape == want[k].shape, k
        assert rel_err(got[k], want[k]) < 1e-10, k


def test_dispatch_predicate_is_off_unless_everything_holds(monkeypatch):
    n = D.FUSED_MIN_ROWS
    m = D.FreeGaussianDeformableModel()
    x, t = torch.zeros(n, 3), torch.zeros(n, 1)
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "1")
    assert not D.fused_train_applies(m, x, t)  # CPU tensors
    assert not D.fused_train_applies(D.FreeGaussianControllableModel(), x, torch.zeros(n, 3))
    # everything but the device: a stand-in that reports CUDA, so that each other condition is seen to matter alone
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    assert D.fused_train_applies(m, x, t)
    assert D.fused_train_applies(D.FreeGaussianControllableModel(), x, torch.zeros(n, 3))
    assert not D.fused_applies(m, x, t)  # (a taped forward of a module in training is not the inference path's)
    monkeypatch.delenv("FG_FUSED_MLP_TRAIN")
    assert not D.fused_train_applies(m, x, t)  # unset means off
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "0")
    assert not D.fused_train_applies(m, x, t)
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "1")
    assert not D.fused_train_applies(D.FreeGaussianDeformableModel(is_blender=True), x, t)
    assert not D.fused_train_applies(m, x.clone().requires_grad_(True), t)
    assert not D.fused_train_applies(m, x, t.clone().requires_grad_(True))
    with torch.no_grad():
        assert not D.fused_train_applies(m, x, t)
    assert not D.fused_train_applies(m, x[: n - 1], t[: n - 1])  # below FUSED_MIN_ROWS
    assert not D.fused_train_applies(m, x.double(), t.double())
    assert not D.fused_train_applies(D.FreeGaussianDeformableModel(W=128), x, t)
    assert not D.fused_train_applies(D.FreeGaussianDeformableModel().requires_grad_(False), x, t)  # nothing to train
    assert D.fused_train_applies(m, x, t)
