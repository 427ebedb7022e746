"""CPU checks of the chunked fused backward's host side: the C ABI of ``fg_mlp_train_bwd`` (the two queries, argument
validation: every call returns before a launch), ``ops.mlp_train``'s refusal, and the knob ``FG_FUSED_MLP_CHUNKED`` in
``deform``'s dispatch."""
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
SIZES = (1, 512, 513, 5000, 33_000, 240_000, 1_000_000)
BLOCK = 4 * (7 * 256 * 256 + 2 * 256 * 128 + 8 * 256 + 16 * 256 + 16)  # one slab's partial results: 2 121 792 bytes


NOTHING = ((), (), (), ())


def _call(n, d, g_heads=PTR, enc=PTR, acts=PTR, g_enc=PTR, out="all", chunk_slabs=0, ws=PTR, ws_bytes=0):
    out = grads() if isinstance(out, str) else out
    return _lib.load().fg_mlp_train_bwd(n, addr(d), g_heads, enc, acts, g_enc, addr(out), chunk_slabs, ws, ws_bytes, None)


def test_header_and_binding_agree():
    text = header_text()
    lib = _lib.load()
    assert "#define FG_ABI_VERSION 14" in text and _lib.ABI_VERSION == 14 and lib.fg_abi_version() == 14
    assert re.search(r"^#define FG_ABI_MINOR 1\b", text, flags=re.M) and _lib.ABI_MINOR == 1 and lib.fg_abi_minor() >= 1
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for proto in (
        "int fg_abi_minor(void);",
        "int64_t fg_mlp_train_bwd_chunk_rows(int64_t N, int32_t chunk_slabs);",
        "size_t fg_mlp_train_bwd_workspace_bytes(int64_t N, int32_t chunk_slabs, int32_t want_g_enc);",
        "int fg_mlp_train_bwd(int64_t N, const fg_mlp_desc* desc, const float* g_heads, const float* enc, const float* acts, "
        "float* g_enc, const fg_mlp_grads* out, int32_t chunk_slabs, void* workspace, size_t workspace_bytes, fg_stream_t stream);",
    ):
        assert proto in code, proto
    P, i32, i64, sz = _lib.P, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    assert _lib.SIGNATURES["fg_abi_minor"] == (ctypes.c_int, [])
    assert _lib.SIGNATURES["fg_mlp_train_bwd_chunk_rows"] == (i64, [i64, i32])
    assert _lib.SIGNATURES["fg_mlp_train_bwd_workspace_bytes"] == (sz, [i64, i32, i32])
    assert _lib.SIGNATURES["fg_mlp_train_bwd"] == (ctypes.c_int, [i64, P, P, P, P, P, P, i32, P, sz, P])
    assert re.search(r"^#define FG_MLP_TRAIN_BWD_ALIGN 4096\b", text, flags=re.M)
    m = re.search(r"^#define FG_MLP_TRAIN_BWD_CHUNK_SLABS (\d+)", text, flags=re.M)
    assert m and int(m.group(1)) == _lib.MLP_TRAIN_BWD_CHUNK_SLABS and int(m.group(1)) in (16, 21, 32, 42)
    # the older entry points are what they were
    assert _lib.SIGNATURES["fg_mlp_fwd"] == (ctypes.c_int, [i64, P, P, sz, P])
    assert _lib.SIGNATURES["fg_mlp_train_workspace_bytes"] == (sz, [i64])
    assert _lib.SIGNATURES["fg_mlp_train_fwd"] == (ctypes.c_int, [i64, P, P, P, P, P, sz, P])
    assert _lib.SIGNATURES["fg_mlp_bwd"] == (ctypes.c_int, [i64, P, P, P, P, P, sz, P])
    assert _lib.SIGNATURES["fg_mlp_bwd_inputs_workspace_bytes"] == (sz, [i64])
    assert _lib.SIGNATURES["fg_mlp_bwd_inputs"] == (ctypes.c_int, [i64, P, P, P, P, P, P, sz, P])
    assert _lib.SIGNATURES["fg_mlp_param_grads_workspace_bytes"] == (sz, [i64])
    assert _lib.SIGNATURES["fg_mlp_param_grads_slab_rows"] == (ctypes.c_int, [i64])
    assert _lib.SIGNATURES["fg_mlp_param_grads"] == (ctypes.c_int, [i64, P, P, P, P, P, P, P, sz, P])


def test_chunk_rows_follow_the_slab_cut():
    lib = _lib.load()
    for n in SIZES:
        slab = ops.mlp_wgrad_slab_rows(n)
        slabs = -(-n // slab)
        for c in (1, 3, 0):
            want = min(c if c else _lib.MLP_TRAIN_BWD_CHUNK_SLABS, slabs) * slab
            got = ops.mlp_train_chunk_rows(n, c)
            assert got == want == int(lib.fg_mlp_train_bwd_chunk_rows(n, c)) and got % 64 == 0 and got > 0, (n, c)
            assert got == ops.mlp_train_chunk_rows(n, c)  # a function of its arguments alone
        assert ops.mlp_train_chunk_rows(n, slabs) == ops.mlp_train_chunk_rows(n, slabs + 5) == slabs * slab  # capped
    assert ops.mlp_train_chunk_rows(n) == ops.mlp_train_chunk_rows(n, 0)
    assert ops.mlp_train_chunk_rows(0, 1) == 0 and ops.mlp_train_chunk_rows(-3, 1) == 0


def test_workspace_is_the_documented_sum_and_does_not_grow_with_the_array():
    lib = _lib.load()
    for c in (1, 3, 0):
        for g_enc in (0, 1):
            sizes = []
            for n in SIZES:
                pack = int(lib.fg_mlp_bwd_inputs_workspace_bytes(n) if g_enc else lib.fg_mlp_train_workspace_bytes(n))
                pack = -(-pack // 4096) * 4096  # (FG_MLP_TRAIN_BWD_ALIGN: the chunk array starts on a 4 KB boundary)
                want = pack + 8 * ops.mlp_train_chunk_rows(n, c) * 256 * 4 + int(lib.fg_mlp_param_grads_workspace_bytes(n))
                sizes.append(int(lib.fg_mlp_train_bwd_workspace_bytes(n, c, g_enc)))
                assert sizes[-1] == want and want % 16 == 0, (n, c, g_enc)
            assert sizes == sorted(sizes), (c, g_enc)  # monotone in N
    # the partial blocks are fg_mlp_param_grads' own: one per slab of its bound
    assert int(lib.fg_mlp_param_grads_workspace_bytes(1_000_000)) == 245 * BLOCK
    for n in (0, -1):
        assert int(lib.fg_mlp_train_bwd_workspace_bytes(n, 0, 1)) == 0
    # the library's constant at 1M rows: under a quarter of the array it replaces (G: 8 x 256 x 4 bytes per row)
    n = 1_000_000
    assert int(lib.fg_mlp_train_bwd_workspace_bytes(n, 0, 1)) < 8 * 256 * 4 * n // 4
    # ... and once the chunk is full the only part that grows is the partial blocks: 2 121 792 bytes per 4096 rows
    step = int(lib.fg_mlp_train_bwd_workspace_bytes(2 * n, 0, 1)) - int(lib.fg_mlp_train_bwd_workspace_bytes(n, 0, 1))
    assert step == (-(-2 * n // 4096) - 245) * BLOCK


def test_error_codes_without_gpu():
    assert _call(0, None, None, None, None, None, None, 0, None, 0) == OK  # N = 0: nothing to do, nothing is looked at
    assert _call(0, desc(A=0), chunk_slabs=-1) == OK
    assert _call(-1, desc()) == INVALID
    assert _call(100, None) == INVALID
    assert _call(100, desc(), chunk_slabs=-1, ws_bytes=BIG) == INVALID
    # everything in order but the workspace's size
    assert _call(100, desc()) == WORKSPACE
    assert _call(100, desc(A=63, rows=(3, 4, 3))) == WORKSPACE and _call(100, desc(A=1, rows=(16,))) == WORKSPACE
    assert _call(100, desc(A=64, rows=(1,)), g_enc=None) == WORKSPACE
    # the chain reads the weights: a descriptor without them is refused (fg_mlp_param_grads alone accepts it)
    assert _call(100, desc(weights=False), ws_bytes=BIG) == INVALID
    for field in ("weight", "bias", "head_weight", "head_bias"):
        d = desc()
        getattr(d, field)[2] = None
        assert _call(100, d, ws_bytes=BIG) == INVALID, field
    d = desc()
    d.size -= 8
    assert _call(100, d, ws_bytes=BIG) == INVALID
    assert _call(100, desc(mode=_lib.MLP_SE3), ws_bytes=BIG) == INVALID and _call(100, desc(mode=7), ws_bytes=BIG) == INVALID
    for A in (0, 65):
        assert _call(100, desc(A=A), ws_bytes=BIG) == INVALID
    for rows in ((0,), (17,), (8, 9)):
        assert _call(100, desc(rows=rows), ws_bytes=BIG) == INVALID
    for field, value in (("depth", 6), ("width", 128), ("multires", 6)):
        d = desc()
        setattr(d, field, value)
        assert _call(100, d, ws_bytes=BIG) == UNSUPPORTED, field
    # out: null, a wrong size field
    assert _call(100, desc(), out=None, ws_bytes=BIG) == INVALID
    g = grads()
    g.size -= 8
    assert _call(100, desc(), out=g, ws_bytes=BIG) == INVALID
    # nothing asked for at all: FG_OK whatever else is null; with g_enc wanted the chunks run, so the chain's inputs are needed
    assert _call(100, desc(), None, None, None, None, out=grads(*NOTHING), ws=None, ws_bytes=0) == OK
    assert _call(100, desc(), enc=None, out=grads(*NOTHING)) == WORKSPACE  # (g_enc alone reads no enc)
    assert _call(100, desc(), g_heads=None, out=grads(*NOTHING), ws_bytes=BIG) == INVALID
    assert _call(100, desc(), acts=None, out=grads(*NOTHING), ws_bytes=BIG) == INVALID
    # g_heads and acts are read whatever is asked for, enc where weight[0] / weight[5] is
    only = lambda **kw: grads(**{**dict(zip(("weight", "bias", "head_weight", "head_bias"), NOTHING)), **kw})  # noqa: E731
    for out in ("all", only(bias=(3,)), only(head_bias=(1,))):
        assert _call(100, desc(), g_heads=None, out=out, g_enc=None, ws_bytes=BIG) == INVALID
        assert _call(100, desc(), acts=None, out=out, g_enc=None, ws_bytes=BIG) == INVALID
    assert _call(100, desc(), enc=None, out=grads(weight=(1, 2, 3, 4, 6, 7))) == WORKSPACE
    assert _call(100, desc(), enc=None, out=only(weight=(0,)), ws_bytes=BIG) == INVALID
    assert _call(100, desc(), enc=None, out=only(weight=(5,)), ws_bytes=BIG) == INVALID
    assert _call(100, desc(), enc=None, ws_bytes=BIG) == INVALID
    # no workspace, one that is not 16-byte aligned, one a byte short (with and without g_enc, for more than one chunk length)
    assert _call(100, desc(), ws=None, ws_bytes=BIG) == INVALID
    assert _call(100, desc(), ws=PTR + 4, ws_bytes=BIG) == INVALID
    lib = _lib.load()
    for n, c, g_enc in ((100, 0, PTR), (100, 0, None), (5000, 3, PTR), (5000, 1, None), (5000, 99, PTR)):
        need = int(lib.fg_mlp_train_bwd_workspace_bytes(n, c, int(g_enc is not None)))
        assert need > 0 and _call(n, desc(), g_enc=g_enc, chunk_slabs=c, ws_bytes=need - 1) == WORKSPACE, (n, c)
    assert int(lib.fg_mlp_train_bwd_workspace_bytes(5000, 3, 1)) > int(lib.fg_mlp_train_bwd_workspace_bytes(5000, 3, 0))


def _nets():
    return (("1", D.FreeGaussianDeformableModel(), {}), ("2", D.FreeGaussianDeformableModel(is_blender=True), {"input_grads": True}),
            ("1", D.FreeGaussianControllableModel(), {}), ("2", D.FreeGaussianControllableModel(), {"input_grads": True}))  # fmt: skip


def test_knob_in_the_dispatch(monkeypatch):
    seen = stand_in_for_cuda(monkeypatch)
    n = D.FUSED_MIN_ROWS
    x, t, v = torch.rand(n, 3), torch.rand(n, 1), torch.rand(n, 3)
    other = lambda m: v if isinstance(m, D.FreeGaussianControllableModel) else t  # noqa: E731
    # unset: the keywords of before, with and without the parameter-gradient knob
    monkeypatch.delenv("FG_FUSED_MLP_CHUNKED", raising=False)
    for wgrad in (None, "1"):
        monkeypatch.setenv("FG_FUSED_MLP_WGRAD", wgrad) if wgrad else monkeypatch.delenv("FG_FUSED_MLP_WGRAD", raising=False)
        for train, m, want in _nets():
            monkeypatch.setenv("FG_FUSED_MLP_TRAIN", train)
            m(x, other(m))
            assert seen[-1] == ({**want, "fused_param_grads": True} if wgrad else want)
            assert D._train_keywords(train) == seen[-1]
    # set, but the parameter-gradient knob unset or not "1": nothing is added
    monkeypatch.setenv("FG_FUSED_MLP_CHUNKED", "1")
    for wgrad in (None, "0", "", "2", "yes"):
        monkeypatch.setenv("FG_FUSED_MLP_WGRAD", wgrad) if wgrad is not None else monkeypatch.delenv("FG_FUSED_MLP_WGRAD", raising=False)
        for train, m, want in _nets():
            monkeypatch.setenv("FG_FUSED_MLP_TRAIN", train)
            m(x, other(m))
            assert seen[-1] == want, (wgrad, train)
    # both set
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD", "1")
    for train, m, want in _nets():
        monkeypatch.setenv("FG_FUSED_MLP_TRAIN", train)
        m(x, other(m))
        assert seen[-1] == {**want, "fused_param_grads": True, "chunked_backward": True}, train
    # only "1" turns it on
    monkeypatch.setenv("FG_FUSED_MLP_TRAIN", "1")
    for value in ("0", "", "2", "yes", "true"):
        monkeypatch.setenv("FG_FUSED_MLP_CHUNKED", value)
        D.FreeGaussianDeformableModel()(x, t)
        assert seen[-1] == {"fused_param_grads": True}, value
    # without the training knob nothing is dispatched at all
    monkeypatch.setenv("FG_FUSED_MLP_CHUNKED", "1")
    monkeypatch.delenv("FG_FUSED_MLP_TRAIN")
    calls = len(seen)
    m = D.FreeGaussianDeformableModel()
    assert D.fused_train_mode(m, x, t) == ""
    m(x, t)
    assert len(seen) == calls
    # the knob is read in deform.py and nowhere else in the package
    pkg = os.path.dirname(os.path.abspath(D.__file__))
    users = [f for f in sorted(os.listdir(pkg)) if f.endswith(".py") and "FG_FUSED_MLP_CHUNKED" in open(os.path.join(pkg, f)).read()]
    assert users == ["deform.py"]


def test_mlp_train_refuses_chunks_without_the_fused_parameter_gradients(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a))
    m = D.FreeGaussianDeformableModel()
    heads = (m.branch_w, m.branch_v, m.gaussian_rotation, m.gaussian_scaling)
    x, aux = torch.rand(8, 3), torch.rand(8, 21)
    for chunked in (True, 3):
        with pytest.raises(ValueError, match="fused_param_grads"):
            ops.mlp_train(x, aux, m.linear, heads, chunked_backward=chunked, fused_param_grads=False)
        with pytest.raises(ValueError, match="fused_param_grads"):
            ops.mlp_train(x, aux, m.linear, heads, chunked_backward=chunked)
    for chunked in (0, -2, 1.5, "1"):  # neither True nor a positive int
        with pytest.raises(ValueError, match="chunked_backward"):
            ops.mlp_train(x, aux, m.linear, heads, chunked_backward=chunked, fused_param_grads=True)
    assert not calls


def test_mlp_train_backward_refuses_cpu_tensors_and_bad_shapes(monkeypatch):
    m = D.FreeGaussianDeformableModel()
    heads = (m.branch_w, m.branch_v, m.gaussian_rotation, m.gaussian_scaling)
    n, rows = 8, (3, 3, 4, 3)
    enc, H, gh = torch.zeros(n, 88), torch.zeros(8, n, 256), torch.zeros(n, 13)
    with pytest.raises(ValueError):
        ops.mlp_train_backward(enc, H, gh, m.linear, heads, 21, rows)  # CPU tensors
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a))
    bad = [
        dict(enc=enc.double(), H=H.double(), gh=gh.double()),  # float64
        dict(H=H[:, :-1].contiguous()),  # mismatched N
        dict(rows=(3, 3, 4)),  # head rows that do not sum to g_heads' width
        dict(rows=(3, 4, 3, 3)),  # ... or are not the heads'
        dict(A=22),  # an enc of another aux width
        dict(want=[True] * 5),  # a want of the wrong length
        dict(chunk_slabs=-1),
        dict(chunk_slabs=True),
    ]
    for kw in bad:
        a = dict(enc=enc, H=H, gh=gh, A=21, rows=rows, want=None, chunk_slabs=0)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.mlp_train_backward(a["enc"], a["H"], a["gh"], m.linear, heads, a["A"], a["rows"], want=a["want"], chunk_slabs=a["chunk_slabs"])
    assert not calls
