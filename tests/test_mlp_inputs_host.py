"""CPU checks of the host side of the fused MLP backward with input-row gradients: the C ABI of ``fg_mlp_bwd_inputs``
(argument validation and the workspace query; every call returns before a launch), the dispatch predicate under
``FG_FUSED_MLP_TRAIN=2``, and the chain from ``g_enc`` to the inputs (``ops.mlp_input_grads``) in float64 against autograd."""
import ctypes

import pytest
import torch

from freegaussian_amd import _lib
from freegaussian_amd import deform as D
from freegaussian_amd import ops
from freegaussian_amd.utils import positional_encoding
from helpers import rel_err
from mlp_common import PTR, addr, desc, header_text

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
BIG = 1 << 40  # a workspace that would do (every call below is refused before a launch)
TIN_BYTES = 2 * 32 * 128 * 8 * 4  # the input columns of layers 0 and 5, packed


def _desc(*a, **kw):
    return desc(*a, inputs=True, **kw)


def _call(n, d, g_heads=PTR, acts=PTR, g_pre=PTR, g_enc=PTR, ws=PTR, ws_bytes=0):
    return _lib.load().fg_mlp_bwd_inputs(n, addr(d), g_heads, acts, g_pre, g_enc, ws, ws_bytes, None)


def test_header_and_binding_agree():
    text = header_text()
    assert f"#define FG_ABI_VERSION {_lib.ABI_VERSION}" in text and _lib.ABI_VERSION >= 13
    assert _lib.load().fg_abi_version() == _lib.ABI_VERSION
    for name in ("fg_mlp_bwd_inputs_workspace_bytes", "fg_mlp_bwd_inputs"):
        assert name in _lib.SIGNATURES and f"{name}(" in text
    c64, sz, P = ctypes.c_int64, ctypes.c_size_t, _lib.P
    assert _lib.SIGNATURES["fg_mlp_bwd_inputs_workspace_bytes"] == (sz, [c64])
    assert _lib.SIGNATURES["fg_mlp_bwd_inputs"] == (ctypes.c_int, [c64, P, P, P, P, P, P, sz, P])
    # what was there is what it was
    assert _lib.SIGNATURES["fg_mlp_bwd"] == (ctypes.c_int, [c64, P, P, P, P, P, sz, P])
    assert _lib.SIGNATURES["fg_mlp_fwd"] == (ctypes.c_int, [c64, P, P, sz, P])
    assert ctypes.sizeof(_lib.MlpDesc) == 12 * 4 + 8 + (2 + 8 + 8 + 3 * _lib.MLP_MAX_HEADS) * 8


def test_error_codes_without_gpu():
    call = _call
    assert call(0, None, None, None, None, None, None, 0) == OK  # N = 0: nothing to do, nothing is looked at
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
    # null buffers: g_heads, acts, g_pre, g_enc
    for i in range(4):
        bufs = [PTR] * 4
        bufs[i] = None
        assert call(100, _desc(), *bufs, ws_bytes=BIG) == INVALID, i
    # the inputs are not read
    for field in ("x", "aux"):
        d = _desc()
        setattr(d, field, None)
        assert call(100, d) == WORKSPACE, field
    # no workspace, one that is not 16-byte aligned, one a byte short of the new query, the other calls' size
    assert call(100, _desc(), ws=None, ws_bytes=BIG) == INVALID
    assert call(100, _desc(), ws=PTR + 4, ws_bytes=BIG) == INVALID
    need = int(_lib.load().fg_mlp_bwd_inputs_workspace_bytes(100))
    assert call(100, _desc(), ws_bytes=need - 1) == WORKSPACE
    assert call(100, _desc(), ws_bytes=int(_lib.load().fg_mlp_train_workspace_bytes(100))) == WORKSPACE


def test_workspace_query():
    lib = _lib.load()
    sizes = [int(lib.fg_mlp_bwd_inputs_workspace_bytes(n)) for n in (0, 1, 63, 64, 65, 1000, 33_000, 1_000_000, 1 << 33)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert int(lib.fg_mlp_bwd_inputs_workspace_bytes(-1)) == 0
    assert sizes[1] >= int(lib.fg_mlp_train_workspace_bytes(1)) + TIN_BYTES
    assert sizes[1] % 16 == 0
    # the other calls' query: the forward's packed weights at the widest input row ([256 k-groups][256][8] + the heads)
    assert int(lib.fg_mlp_train_workspace_bytes(1)) == int(lib.fg_mlp_workspace_bytes(1)) == 4 * (256 * 2048 + 16 * 256 + 16)


def test_dispatch_predicate_under_each_value(monkeypatch):
    n = D.FUSED_MIN_ROWS
    m, blender, control = D.FreeGaussianDeformableModel(), D.FreeGaussianDeformableModel(is_blender=True), D.FreeGaussianControllableModel()
    x, t = torch.zeros(n, 3), torch.zeros(n, 1)
    xg, tg = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "2")
    assert not D.fused_train_applies(m, x, t) and not D.fused_train_applies(blender, x, t)  # CPU tensors
    # everything but the device: a stand-in that reports CUDA, so that each other condition is seen to matter alone
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    new_ground = [(blender, x, t), (m, xg, t), (m, x, tg), (blender, xg, tg), (control, xg, torch.zeros(n, 3, requires_grad=True))]
    old_ground = [(m, x, t), (control, x, torch.zeros(n, 3))]
    for case in new_ground + old_ground:
        assert D.fused_train_applies(*case)
    assert not D.fused_applies(blender, x, t)  # (a taped forward of a module in training is not the inference path's)
    for value in ("1", "0", "", None, "3", "on"):
        monkeypatch.delenv("FG_FUSED_MLP_TRAIN") if value is None else monkeypatch.setenv("FG_FUSED_MLP_TRAIN", value)
        for case in new_ground:
            assert not D.fused_train_applies(*case), value
        for case in old_ground:
            assert D.fused_train_applies(*case) == (value == "1"), value
    # the refusals that hold under every value, line by line
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "2")
    for net in (m, blender):
        with torch.no_grad():
            assert not D.fused_train_applies(net, x, t)
        assert not D.fused_train_applies(net, x[: n - 1], t[: n - 1])  # below FUSED_MIN_ROWS
        assert not D.fused_train_applies(net, x.double(), t.double())
        assert not D.fused_train_applies(net, x, torch.zeros(n, 2))
        assert not D.fused_train_applies(net, x, t[:1])
    assert not D.fused_train_applies(D.FreeGaussianDeformableModel(W=128), x, t)
    assert not D.fused_train_applies(D.FreeGaussianDeformableModel(W=128, is_blender=True), x, t)
    assert not D.fused_train_applies(D.FreeGaussianDeformableModel(is_blender=True).requires_grad_(False), x, t)  # nothing to train
    assert not D.fused_train_applies(D.FreeGaussianDeformableModel().requires_grad_(False), xg, t)
    assert D.fused_train_applies(blender, x, t)


@pytest.mark.parametrize("A,one_row", [(21, False), (30, True), (1, False), (64, True)])
def test_input_gradient_chain_equals_autograd_in_float64(A, one_row):
    """``mlp_input_grads`` on a random ``g_enc`` against autograd through ``positional_encoding`` + concat, with the padded
    widths of the kernel's arrays (the pad columns hold what they will: nothing may read them)."""
    n, g = 37, torch.Generator().manual_seed(A)
    x = (torch.rand(n, 3, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    aux = torch.randn(1 if one_row else n, A, generator=g, dtype=torch.float64).requires_grad_(True)
    inp = torch.cat([positional_encoding(x, 10), aux.expand(n, -1)], dim=-1)
    w = _lib.mlp_enc_width(A)
    g_enc = torch.randn(n, w, generator=g, dtype=torch.float64)
    (inp * g_enc[:, : 63 + A]).sum().backward()
    enc = torch.cat([inp.detach(), torch.full((n, w - 63 - A), 7.0, dtype=torch.float64)], dim=-1)
    g_x, g_aux = ops.mlp_input_grads(g_enc, enc, A, True, True, one_row)
    assert g_x.shape == x.shape and g_aux.shape == aux.shape
    assert rel_err(g_x, x.grad) < 1e-12 and rel_err(g_aux, aux.grad) < 1e-12
    # only what is wanted is formed
    assert ops.mlp_input_grads(g_enc, enc, A, False, True, one_row)[0] is None
    assert ops.mlp_input_grads(g_enc, enc, A, True, False, one_row)[1] is None


def test_ops_keyword_and_refusals_on_the_cpu():
    m = D.FreeGaussianDeformableModel()
    heads = (m.branch_w, m.branch_v, m.gaussian_rotation, m.gaussian_scaling)
    with pytest.raises(ValueError):
        ops.mlp_train(torch.zeros(4, 3), torch.zeros(4, 21), m.linear, heads, input_grads=True)  # CPU tensors
    with pytest.raises(ValueError):
        ops.mlp_train(torch.zeros(0, 3), torch.zeros(0, 21), m.linear, heads, input_grads=True)
