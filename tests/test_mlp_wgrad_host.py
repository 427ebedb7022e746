"""CPU checks of the fused parameter-gradient call's host side: the C ABI of ``fg_mlp_param_grads`` (argument validation
and the workspace query; every call returns before a launch), ``ops.mlp_param_grads``'s refusals, and the knob
``FG_FUSED_MLP_WGRAD`` in ``deform``'s dispatch."""
import ctypes
import os
import re

import pytest
import torch

from freegaussian_amd import _lib
from freegaussian_amd import deform as D
from freegaussian_amd import ops
from mlp_common import PTR, addr, desc, grads, header_text, stand_in_for_cuda

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
BIG = 1 << 40  # a workspace that would do (every call below is refused before a launch)


def _desc(*a, **kw):
    """The shape alone: every parameter and input pointer of the descriptor stays null."""
    return desc(*a, weights=False, **kw)


def _call(n, d, enc=PTR, acts=PTR, g_pre=PTR, g_heads=PTR, out="all", ws=PTR, ws_bytes=0):
    out = grads() if isinstance(out, str) else out
    return _lib.load().fg_mlp_param_grads(n, addr(d), enc, acts, g_pre, g_heads, addr(out), ws, ws_bytes, None)


def test_header_and_binding_agree():
    text = header_text()
    assert "#define FG_ABI_VERSION 14" in text and _lib.ABI_VERSION == 14 and _lib.load().fg_abi_version() == 14
    for name in ("fg_mlp_param_grads_workspace_bytes", "fg_mlp_param_grads"):
        assert name in _lib.SIGNATURES and f"{name}(" in text
    P, i64, sz = _lib.P, ctypes.c_int64, ctypes.c_size_t
    assert _lib.SIGNATURES["fg_mlp_param_grads_workspace_bytes"] == (ctypes.c_size_t, [i64])
    assert _lib.SIGNATURES["fg_mlp_param_grads"] == (ctypes.c_int, [i64, P, P, P, P, P, P, P, sz, P])
    # the struct as the header spells it: two int32, then 8 + 8 + MAX_HEADS + MAX_HEADS pointers
    body = re.search(r"typedef struct fg_mlp_grads \{(.*?)\} fg_mlp_grads;", text, re.S).group(1)
    fields = [f.strip() for f in re.sub(r"/\*.*?\*/", "", body).split(";") if f.strip()]
    assert fields == ["int32_t size", "int32_t reserved", "float* weight[8]", "float* bias[8]",
                      "float* head_weight[FG_MLP_MAX_HEADS]", "float* head_bias[FG_MLP_MAX_HEADS]"]  # fmt: skip
    assert [n for n, _ in _lib.MlpGrads._fields_] == ["size", "reserved", "weight", "bias", "head_weight", "head_bias"]
    assert ctypes.sizeof(_lib.MlpGrads) == 2 * 4 + (8 + 8 + 2 * _lib.MLP_MAX_HEADS) * 8
    assert f"#define FG_MLP_WGRAD_MAX_SLAB {_lib.MLP_WGRAD_MAX_SLAB}" in text and _lib.MLP_WGRAD_MAX_SLAB <= D._TallLinear.CHUNK
    assert f"#define FG_MLP_WGRAD_MIN_SPLIT {_lib.MLP_WGRAD_MIN_SPLIT}" in text
    # the older entry points and the descriptor are what they were
    assert _lib.SIGNATURES["fg_mlp_fwd"] == (ctypes.c_int, [i64, P, P, sz, P])
    assert _lib.SIGNATURES["fg_mlp_train_workspace_bytes"] == (sz, [i64])
    assert _lib.SIGNATURES["fg_mlp_train_fwd"] == (ctypes.c_int, [i64, P, P, P, P, P, sz, P])
    assert _lib.SIGNATURES["fg_mlp_bwd"] == (ctypes.c_int, [i64, P, P, P, P, P, sz, P])
    assert _lib.SIGNATURES["fg_mlp_bwd_inputs_workspace_bytes"] == (sz, [i64])
    assert _lib.SIGNATURES["fg_mlp_bwd_inputs"] == (ctypes.c_int, [i64, P, P, P, P, P, P, sz, P])
    assert ctypes.sizeof(_lib.MlpDesc) == 12 * 4 + 8 + (2 + 8 + 8 + 3 * _lib.MLP_MAX_HEADS) * 8


def test_error_codes_without_gpu():
    assert _call(0, None, None, None, None, None, None, None, 0) == OK  # N = 0: nothing to do, nothing is looked at
    assert _call(0, _desc(A=0)) == OK
    assert _call(-1, _desc()) == INVALID
    assert _call(100, None) == INVALID
    # a descriptor whose weight pointers are all null is accepted: everything but the workspace's size is in order
    assert _call(100, _desc()) == WORKSPACE
    assert _call(100, _desc(A=63, rows=(3, 4, 3))) == WORKSPACE and _call(100, _desc(A=1, rows=(16,))) == WORKSPACE
    assert _call(100, _desc(A=64, rows=(1,))) == WORKSPACE
    assert _call(100, _desc(mode=_lib.MLP_SE3)) == INVALID and _call(100, _desc(mode=7)) == INVALID
    for A in (0, 65):
        assert _call(100, _desc(A=A)) == INVALID
    for rows in ((0,), (17,), (8, 9)):
        assert _call(100, _desc(rows=rows)) == INVALID
    d = _desc()
    d.size -= 8
    assert _call(100, d) == INVALID
    for field, value in (("depth", 6), ("width", 128), ("multires", 6)):
        d = _desc()
        setattr(d, field, value)
        assert _call(100, d) == UNSUPPORTED, field
    # out: null, a wrong size field, every pointer null (nothing to do: no workspace is asked for)
    assert _call(100, _desc(), out=None, ws_bytes=BIG) == INVALID
    g = grads()
    g.size -= 8
    assert _call(100, _desc(), out=g, ws_bytes=BIG) == INVALID
    assert _call(100, _desc(), None, None, None, None, out=grads((), (), (), ()), ws=None, ws_bytes=0) == OK
    # each null input whose product is wanted
    for i in range(4):
        bufs = [PTR] * 4
        bufs[i] = None
        assert _call(100, _desc(), *bufs, ws_bytes=BIG) == INVALID, i
    # ... and a null input that no gradient asked for reads
    none = ((), (), (), ())
    only = lambda **kw: grads(**{**dict(zip(("weight", "bias", "head_weight", "head_bias"), none)), **kw})  # noqa: E731
    assert _call(100, _desc(), enc=None, out=grads(weight=(1, 2, 3, 4, 6, 7))) == WORKSPACE
    assert _call(100, _desc(), enc=None, out=grads(weight=(0,)), ws_bytes=BIG) == INVALID
    assert _call(100, _desc(), enc=None, out=grads(weight=(5,)), ws_bytes=BIG) == INVALID
    assert _call(100, _desc(), acts=None, out=only(weight=(0,), bias=range(8), head_bias=range(4))) == WORKSPACE
    assert _call(100, _desc(), acts=None, out=only(weight=(5,)), ws_bytes=BIG) == INVALID
    assert _call(100, _desc(), acts=None, out=only(head_weight=(2,)), ws_bytes=BIG) == INVALID
    assert _call(100, _desc(), enc=None, acts=None, g_pre=None, out=only(head_bias=(0,))) == WORKSPACE
    assert _call(100, _desc(), g_pre=None, out=only(bias=(3,)), ws_bytes=BIG) == INVALID
    assert _call(100, _desc(), enc=None, acts=None, g_heads=None, out=only(bias=(3,))) == WORKSPACE
    assert _call(100, _desc(), g_heads=None, out=only(head_bias=(1,)), ws_bytes=BIG) == INVALID
    # no workspace, one that is not 16-byte aligned, one a byte short
    assert _call(100, _desc(), ws=None, ws_bytes=BIG) == INVALID
    assert _call(100, _desc(), ws=PTR + 4, ws_bytes=BIG) == INVALID
    need = int(_lib.load().fg_mlp_param_grads_workspace_bytes(100))
    assert need > 0 and _call(100, _desc(), ws_bytes=need - 1) == WORKSPACE


def test_workspace_query_is_monotone_and_does_not_overflow():
    lib = _lib.load()
    ns = (0, 1, 63, 64, 65, 8192, 8193, 33_000, 1_000_000, 1 << 33)
    sizes = [int(lib.fg_mlp_param_grads_workspace_bytes(n)) for n in ns]
    assert sizes == sorted(sizes) and sizes[0] == 0 and sizes[1] > 0
    assert int(lib.fg_mlp_param_grads_workspace_bytes(-1)) == 0
    # one block per slab: every output (the input products 128 columns wide), 16 head rows
    block = 4 * (7 * 256 * 256 + 2 * 256 * 128 + 8 * 256 + 16 * 256 + 16)
    bound = lambda n: max(-(-n // 4096), min(32, -(-n // 512)))  # noqa: E731
    assert sizes[1:] == [bound(n) * block for n in ns[1:]]
    assert sizes[-1] == (1 << 21) * block < 1 << 63  # (4.4e12 bytes: far from the top of size_t, and exact)


def test_slab_cut_depends_on_n_alone_and_stays_within_the_chunk():
    lib = _lib.load()
    for n in (1, 2, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193, 3 * 8192 + 65, 33_000, 131_072, 131_073, 240_000, 1_000_000):
        rows = ops.mlp_wgrad_slab_rows(n)
        slabs = -(-n // rows)
        assert rows % 64 == 0 and 64 <= rows <= _lib.MLP_WGRAD_MAX_SLAB <= D._TallLinear.CHUNK, n  # (no chain beyond the chunk)
        assert slabs * int(lib.fg_mlp_param_grads_workspace_bytes(1)) <= int(lib.fg_mlp_param_grads_workspace_bytes(n)), n
        assert rows == ops.mlp_wgrad_slab_rows(n)
    # short slabs where long ones would leave the machine idle
    assert -(-33_000 // ops.mlp_wgrad_slab_rows(33_000)) >= 31 and ops.mlp_wgrad_slab_rows(1_000_000) == 4096
    assert ops.mlp_wgrad_slab_rows(0) == 0


def test_ops_refuses_cpu_tensors_and_bad_shapes(monkeypatch):
    n = 8
    enc, H, G, gh = torch.zeros(n, 88), torch.zeros(8, n, 256), torch.zeros(8, n, 256), torch.zeros(n, 13)
    rows = (3, 3, 4, 3)
    with pytest.raises(ValueError):
        ops.mlp_param_grads(enc, H, G, gh, 21, rows)  # CPU tensors
    # everything but the device: a stand-in that reports CUDA, so that each other refusal is seen to be its own
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a: calls.append(a))
    bad = [
        (enc.double(), H.double(), G.double(), gh.double(), 21, rows),  # float64
        (enc, H.transpose(0, 1).contiguous().transpose(0, 1), G, gh, 21, rows),  # a non-contiguous H
        (enc, H[:, :-1].contiguous(), G[:, :-1].contiguous(), gh, 21, rows),  # mismatched N
        (enc, H, torch.zeros(7, n, 256), gh, 21, rows),  # G.shape != H.shape
        (enc, H, G, gh, 21, (3, 3, 4)),  # head rows that do not sum to g_heads' width
        # an enc of another aux width: 63 + 26 pads to 96 (63 + 22 pads to enc's own 88, which ops has no reason to refuse)
        (enc, H, G, gh, 26, rows),
        (enc, H, G, gh, 21, rows, [True] * 5),  # a want of the wrong length
    ]
    for args in bad:
        with pytest.raises(ValueError):
            ops.mlp_param_grads(*args)
    assert not calls


def _stand_in_for_cuda(monkeypatch):
    return stand_in_for_cuda(monkeypatch, is_cuda=False)  # (the tests below decide themselves which tensors report CUDA)


def test_knob_unset_passes_no_fused_param_grads(monkeypatch):
    seen = _stand_in_for_cuda(monkeypatch)
    n = D.FUSED_MIN_ROWS
    x, t = torch.rand(n, 3), torch.rand(n, 1)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.delenv("FG_FUSED_MLP_WGRAD", raising=False)
    for value, m, want in (("1", D.FreeGaussianDeformableModel(), {}), ("2", D.FreeGaussianDeformableModel(is_blender=True), {"input_grads": True}),
                           ("1", D.FreeGaussianControllableModel(), {})):  # fmt: skip
        monkeypatch.setenv("FG_FUSED_MLP_TRAIN", value)
        m(x, torch.rand(n, 3) if isinstance(m, D.FreeGaussianControllableModel) else t)
        assert not seen[-1].get("fused_param_grads", False) and {k: v for k, v in seen[-1].items() if k != "fused_param_grads"} == want
    assert len(seen) == 3
    for value in ("0", "", "2", "yes"):  # only "1" turns it on
        monkeypatch.setenv("FG_FUSED_MLP_WGRAD", value)
        D.FreeGaussianDeformableModel()(x, t)
        assert not seen[-1].get("fused_param_grads", False)
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD", "1")
    D.FreeGaussianDeformableModel()(x, t)
    assert seen[-1] == {"fused_param_grads": True}
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "2")
    D.FreeGaussianDeformableModel(is_blender=True)(x, t)
    D.FreeGaussianControllableModel()(x, torch.rand(n, 3))
    assert seen[-2] == seen[-1] == {"input_grads": True, "fused_param_grads": True}


def test_knob_set_without_the_training_knob_runs_the_torch_path(monkeypatch):
    seen = _stand_in_for_cuda(monkeypatch)
    n = 200
    x, t = torch.rand(n, 3), torch.rand(n, 1)
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD", "1")
    monkeypatch.delenv("FG_FUSED_MLP_TRAIN", raising=False)
    torch.manual_seed(0)
    m = D.FreeGaussianDeformableModel()
    outs = m(x, t)
    sum(o.sum() for o in outs).backward()
    assert not seen and all(p.grad is not None for p in m.parameters())
    # the same with tensors that report CUDA and enough rows: still the torch ops, the knob alone dispatches nothing
    big_x, big_t = torch.rand(D.FUSED_MIN_ROWS, 3), torch.rand(D.FUSED_MIN_ROWS, 1)
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
        assert D.fused_train_mode(m, big_x, big_t) == ""
        for value in ("0", ""):
            mp.setenv("FG_FUSED_MLP_TRAIN", value)
            assert D.fused_train_mode(m, big_x, big_t) == ""
    assert not seen
    # the knob is read in deform.py and nowhere else in the package
    pkg = os.path.dirname(os.path.abspath(D.__file__))
    users = [f for f in sorted(os.listdir(pkg)) if f.endswith(".py") and "FG_FUSED_MLP_WGRAD" in open(os.path.join(pkg, f)).read()]
    assert users == ["deform.py"]
