"""CPU checks of the opt-in split-bf16 mode of the fused parameter-gradient products (``fg_mlp_param_grads_p`` /
``fg_mlp_train_bwd_p``, include/fgraster.h): the three symbols across header, binding and library, the new word's
validation (every call returns before a launch), the Python keywords and the ``FG_FUSED_MLP_WGRAD_PRECISION`` knob, and the
arithmetic of the contract emulated on the CPU (tests/mlp_split_common.py) against float64.

The emulation's measured errors (``max|a-b| / max|b|`` of the trunk weight gradients over the emulated split chain's arrays,
1024 rows, against the float64 run of the whole network): three terms 1.2e-5 .. 1.7e-5, two terms 1.7e-3 .. 2.7e-3."""
import ctypes
import re
import subprocess

import pytest
import torch

from freegaussian_amd import _lib
from freegaussian_amd import deform as D
from freegaussian_amd import ops
from helpers import REL_TOL, rel_err
from mlp_common import PTR, addr, desc, grads, header_text
from mlp_split_common import ROWS, case, emulate, product, trunk_weight_grads
from mlp_train_common import head_rows

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
BIG = 1 << 40  # a workspace that would do (every call below is refused before a launch)
FP32, BF16X3 = _lib.MLP_FP32, _lib.MLP_BF16X3


def _desc(precision=0, **kw):
    return desc(precision=precision, **kw)


def _pg(n, d, wprec, enc=PTR, acts=PTR, g_pre=PTR, g_heads=PTR, out="all", ws=PTR, ws_bytes=0):
    out = grads() if isinstance(out, str) else out
    return _lib.load().fg_mlp_param_grads_p(n, addr(d), enc, acts, g_pre, g_heads, addr(out), wprec, ws, ws_bytes, None)


def _pg_old(n, d, enc=PTR, acts=PTR, g_pre=PTR, g_heads=PTR, out="all", ws=PTR, ws_bytes=0):
    out = grads() if isinstance(out, str) else out
    return _lib.load().fg_mlp_param_grads(n, addr(d), enc, acts, g_pre, g_heads, addr(out), ws, ws_bytes, None)


def _tb(n, d, wprec, g_heads=PTR, enc=PTR, acts=PTR, g_enc=PTR, out="all", chunk=0, ws=PTR, ws_bytes=0):
    out = grads() if isinstance(out, str) else out
    return _lib.load().fg_mlp_train_bwd_p(n, addr(d), g_heads, enc, acts, g_enc, addr(out), chunk, wprec, ws, ws_bytes, None)


def _tb_old(n, d, g_heads=PTR, enc=PTR, acts=PTR, g_enc=PTR, out="all", chunk=0, ws=PTR, ws_bytes=0):
    out = grads() if isinstance(out, str) else out
    return _lib.load().fg_mlp_train_bwd(n, addr(d), g_heads, enc, acts, g_enc, addr(out), chunk, ws, ws_bytes, None)


# ---- the symbols --------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_three_symbols():
    text = header_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int fg_mlp_wgrad_precision_supported\(int32_t precision\);", code)
    assert re.search(r"int fg_mlp_param_grads_p\(int64_t N, const fg_mlp_desc\* desc, const float\* enc, const float\* acts, "
                     r"const float\* g_pre,\s*const float\* g_heads, const fg_mlp_grads\* out, int32_t wgrad_precision, "
                     r"void\* workspace,\s*size_t workspace_bytes, fg_stream_t stream\);", code)  # fmt: skip
    assert re.search(r"int fg_mlp_train_bwd_p\(int64_t N, const fg_mlp_desc\* desc, const float\* g_heads, const float\* enc, "
                     r"const float\* acts, float\* g_enc,\s*const fg_mlp_grads\* out, int32_t chunk_slabs, "
                     r"int32_t wgrad_precision, void\* workspace,\s*size_t workspace_bytes, fg_stream_t stream\);", code)  # fmt: skip
    P, i64, i32, sz = _lib.P, ctypes.c_int64, ctypes.c_int32, ctypes.c_size_t
    assert _lib.SIGNATURES["fg_mlp_wgrad_precision_supported"] == (ctypes.c_int, [i32])
    assert _lib.SIGNATURES["fg_mlp_param_grads_p"] == (ctypes.c_int, [i64, P, P, P, P, P, P, i32, P, sz, P])
    assert _lib.SIGNATURES["fg_mlp_train_bwd_p"] == (ctypes.c_int, [i64, P, P, P, P, P, P, i32, i32, P, sz, P])
    # the old calls keep their signatures
    assert _lib.SIGNATURES["fg_mlp_param_grads"] == (ctypes.c_int, [i64, P, P, P, P, P, P, P, sz, P])
    assert _lib.SIGNATURES["fg_mlp_train_bwd"] == (ctypes.c_int, [i64, P, P, P, P, P, P, i32, P, sz, P])
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("fg_mlp_wgrad_precision_supported", "fg_mlp_param_grads_p", "fg_mlp_train_bwd_p"):
        assert re.search(rf" T {name}$", exported, re.M), name
    # found by name: the version numbers stay
    lib = _lib.load()
    assert "#define FG_ABI_VERSION 14" in text and "#define FG_ABI_MINOR 1 " in text
    assert (int(lib.fg_abi_version()), int(lib.fg_abi_minor()), _lib.ABI_VERSION) == (14, 1, 14)
    by_name = text[text.index("BY NAME") : text.index("#define FG_COUNT_OUT_WORDS")]
    for name in ("fg_mlp_wgrad_precision_supported", "fg_mlp_param_grads_p", "fg_mlp_train_bwd_p"):
        assert name in by_name, name
    # fg_mlp_grads keeps its reserved word, the descriptor its layout
    assert [n for n, _ in _lib.MlpGrads._fields_][:2] == ["size", "reserved"]
    assert ctypes.sizeof(_lib.MlpDesc) == 12 * 4 + 8 + (2 + 8 + 8 + 3 * _lib.MLP_MAX_HEADS) * 8


def test_the_capability_query():
    lib = _lib.load()
    assert [int(lib.fg_mlp_wgrad_precision_supported(v)) for v in (0, 1, 7, -1, 2)] == [1, 1, 0, 0, 0]


# ---- the word across the ABI --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", [_pg, _tb], ids=["param_grads_p", "train_bwd_p"])
def test_the_word_is_validated_before_anything_else(call):
    for bad in (7, 2, -1, 1 << 20):
        assert call(100, _desc(), bad, ws_bytes=BIG) == INVALID, bad
        assert call(100, None, bad) == INVALID and call(0, None, bad) == INVALID and call(-1, _desc(), bad) == INVALID
    for good in (FP32, BF16X3):
        assert call(0, _desc(), good) == OK  # N = 0: nothing to do
        assert call(0, None, good, None, None, None, None, None, ws=None) == OK  # ... and nothing else is looked at
        assert call(100, _desc(), good, ws_bytes=0) == WORKSPACE  # everything else about it is accepted: the same need for both
        assert call(-1, _desc(), good) == INVALID


def test_param_grads_p_gives_the_old_calls_codes():
    """Every refusal of tests/test_mlp_wgrad_host.py, for both values of the word, beside the old call's own answer."""
    none = ((), (), (), ())
    only = lambda **kw: grads(**{**dict(zip(("weight", "bias", "head_weight", "head_bias"), none)), **kw})  # noqa: E731
    short_d, short_g = _desc(), grads()
    short_d.size -= 8
    short_g.size -= 8
    need = int(_lib.load().fg_mlp_param_grads_workspace_bytes(100))
    cases = [
        (dict(n=100, d=None), INVALID),
        (dict(n=100, d=_desc(mode=_lib.MLP_SE3)), INVALID),
        (dict(n=100, d=_desc(A=0)), INVALID),
        (dict(n=100, d=_desc(A=65)), INVALID),
        (dict(n=100, d=_desc(rows=(8, 9))), INVALID),
        (dict(n=100, d=short_d), INVALID),
        (dict(n=100, d=_desc(), out=None, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), out=short_g, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), enc=None, acts=None, g_pre=None, g_heads=None, out=grads(*none), ws=None), OK),
        (dict(n=100, d=_desc(), enc=None, out=grads(weight=(0,)), ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), enc=None, out=grads(weight=(1, 2, 3, 4, 6, 7))), WORKSPACE),
        (dict(n=100, d=_desc(), acts=None, out=only(weight=(5,)), ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), g_pre=None, out=only(bias=(3,)), ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), g_heads=None, out=only(head_bias=(1,)), ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), enc=PTR + 4, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), ws=None, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), ws=PTR + 4, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), ws_bytes=need - 1), WORKSPACE),
        (dict(n=100, d=_desc(precision=7)), WORKSPACE),  # the descriptor's word is still ignored here
    ]
    for field, value in (("depth", 6), ("width", 128), ("multires", 6)):
        d = _desc()
        setattr(d, field, value)
        cases.append((dict(n=100, d=d), UNSUPPORTED))
    for i, (kw, want) in enumerate(cases):
        assert _pg_old(**kw) == want, i
        for good in (FP32, BF16X3):
            assert _pg(wprec=good, **kw) == want, (i, good)


def test_train_bwd_p_gives_the_old_calls_codes():
    none = ((), (), (), ())
    short_g = grads()
    short_g.size -= 8
    no_weight = _desc()
    no_weight.weight[3] = None
    lib = _lib.load()
    cases = [
        (dict(n=100, d=None), INVALID),
        (dict(n=100, d=_desc(), chunk=-1, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(precision=7), ws_bytes=BIG), INVALID),  # the chain's word is the descriptor's, as before
        (dict(n=100, d=_desc(precision=BF16X3)), WORKSPACE),
        (dict(n=100, d=_desc(mode=_lib.MLP_SE3), ws_bytes=BIG), INVALID),
        (dict(n=100, d=no_weight, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), out=None, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), out=short_g, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), g_heads=None, enc=None, acts=None, g_enc=None, out=grads(*none), ws=None), OK),
        (dict(n=100, d=_desc(), g_heads=None, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), acts=None, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), enc=None, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), ws=None, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), ws=PTR + 4, ws_bytes=BIG), INVALID),
        (dict(n=100, d=_desc(), ws_bytes=int(lib.fg_mlp_train_bwd_workspace_bytes(100, 0, 1)) - 1), WORKSPACE),
        (dict(n=100, d=_desc(), g_enc=None, ws_bytes=int(lib.fg_mlp_train_bwd_workspace_bytes(100, 0, 0)) - 1), WORKSPACE),
    ]
    d = _desc()
    d.depth = 6
    cases.append((dict(n=100, d=d, ws_bytes=BIG), UNSUPPORTED))
    for i, (kw, want) in enumerate(cases):
        assert _tb_old(**kw) == want, i
        for good in (FP32, BF16X3):
            assert _tb(wprec=good, **kw) == want, (i, good)


def test_workspace_queries_return_what_they_returned():
    """The queries take no precision: one size for both (same slabs, same partial blocks)."""
    lib = _lib.load()
    block = 4 * (7 * 256 * 256 + 2 * 256 * 128 + 8 * 256 + 16 * 256 + 16)
    assert block == 2_121_792
    bound = lambda n: max(-(-n // 4096), min(32, -(-n // 512)))  # noqa: E731
    fwd = 4 * (2048 * (16 + 6 * 32 + 48) + 16 * 256 + 16)
    pack = -(-max(fwd, 4 * 2048 * (7 * 32 + 2)) // 4096) * 4096
    for n in (1, 64, 65, 8193, 33_000, 240_000, 1_000_000):
        assert int(lib.fg_mlp_param_grads_workspace_bytes(n)) == bound(n) * block
        rows = int(lib.fg_mlp_param_grads_slab_rows(n))
        assert rows % 64 == 0 and rows == -(-(-(-n // bound(n))) // 64) * 64
        chunk_rows = min(16, -(-n // rows)) * rows
        assert int(lib.fg_mlp_train_bwd_chunk_rows(n, 0)) == chunk_rows
        assert int(lib.fg_mlp_train_bwd_workspace_bytes(n, 0, 0)) == pack + 8 * chunk_rows * 256 * 4 + bound(n) * block
    assert int(lib.fg_mlp_param_grads_workspace_bytes(0)) == 0 and int(lib.fg_mlp_train_bwd_workspace_bytes(0, 0, 0)) == 0


# ---- Python -------------------------------------------------------------------------------------------------------------
def test_the_knob(monkeypatch):
    for name in ("FG_FUSED_MLP_WGRAD_PRECISION", "FG_FUSED_MLP_WGRAD", "FG_FUSED_MLP_PRECISION", "FG_FUSED_MLP_CHUNKED"):
        monkeypatch.delenv(name, raising=False)
    # unset: exactly what it returned
    assert D.fused_wgrad_precision() == "fp32"
    assert D._train_keywords("1") == {} and D._train_keywords("2") == {"input_grads": True}
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD", "1")
    assert D._train_keywords("1") == {"fused_param_grads": True}
    monkeypatch.setenv("FG_FUSED_MLP_CHUNKED", "1")
    assert D._train_keywords("2") == {"input_grads": True, "fused_param_grads": True, "chunked_backward": True}
    monkeypatch.delenv("FG_FUSED_MLP_CHUNKED")
    # fp32: the same
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD_PRECISION", "fp32")
    assert D.fused_wgrad_precision() == "fp32" and D._train_keywords("1") == {"fused_param_grads": True}
    # bf16x3: on top of FG_FUSED_MLP_WGRAD=1 only
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD_PRECISION", "bf16x3")
    assert D.fused_wgrad_precision() == "bf16x3"
    assert D._train_keywords("1") == {"fused_param_grads": True, "param_grads_precision": "bf16x3"}
    monkeypatch.setenv("FG_FUSED_MLP_CHUNKED", "1")
    assert D._train_keywords("2") == {"input_grads": True, "fused_param_grads": True, "chunked_backward": True,
                                      "param_grads_precision": "bf16x3"}  # fmt: skip
    monkeypatch.delenv("FG_FUSED_MLP_CHUNKED")
    monkeypatch.delenv("FG_FUSED_MLP_WGRAD")
    assert D._train_keywords("1") == {} and D._train_keywords("2") == {"input_grads": True}
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD", "0")
    assert D._train_keywords("1") == {}
    # a typo is an error that names the variable, with or without the other knob
    for bad in ("bf16", "BF16X3", "1", ""):
        monkeypatch.setenv("FG_FUSED_MLP_WGRAD_PRECISION", bad)
        for wgrad in ("1", "0"):
            monkeypatch.setenv("FG_FUSED_MLP_WGRAD", wgrad)
            with pytest.raises(ValueError, match="FG_FUSED_MLP_WGRAD_PRECISION"):
                D._train_keywords("1")
    # independent of FG_FUSED_MLP_PRECISION: all four combinations
    monkeypatch.setenv("FG_FUSED_MLP_WGRAD", "1")
    for chain in ("fp32", "bf16x3"):
        for wgrad in ("fp32", "bf16x3"):
            monkeypatch.setenv("FG_FUSED_MLP_PRECISION", chain)
            monkeypatch.setenv("FG_FUSED_MLP_WGRAD_PRECISION", wgrad)
            want = {"fused_param_grads": True}
            if chain == "bf16x3":
                want["precision"] = "bf16x3"
            if wgrad == "bf16x3":
                want["param_grads_precision"] = "bf16x3"
            assert D._train_keywords("1") == want, (chain, wgrad)
            assert D._precision_keywords() == ({"precision": "bf16x3"} if chain == "bf16x3" else {})  # the forward's: untouched


def test_ops_rejects_an_unknown_value_and_the_split_without_the_fused_products():
    m = D.FreeGaussianDeformableModel()
    heads = (m.branch_w, m.branch_v, m.gaussian_rotation, m.gaussian_scaling)
    x, aux = torch.zeros(4, 3), torch.zeros(4, 21)
    enc, H, gh = torch.zeros(4, 88), torch.zeros(8, 4, 256), torch.zeros(4, 13)
    for bad in ("bf16", "fp16", 1, None):
        with pytest.raises(ValueError, match="precision"):
            ops.mlp_param_grads(enc, H, H, gh, 21, (3, 3, 4, 3), precision=bad)
        with pytest.raises(ValueError, match="precision"):
            ops.mlp_train_backward(enc, H, gh, m.linear, heads, 21, (3, 3, 4, 3), param_grads_precision=bad)
        with pytest.raises(ValueError, match="precision"):
            ops.mlp_train(x, aux, m.linear, heads, fused_param_grads=True, param_grads_precision=bad)
    with pytest.raises(ValueError, match="fused_param_grads"):
        ops.mlp_train(x, aux, m.linear, heads, param_grads_precision="bf16x3")
    with pytest.raises(ValueError, match="fused_param_grads"):
        ops.mlp_train(x, aux, m.linear, heads, input_grads=True, precision="bf16x3", param_grads_precision="bf16x3")


# ---- the contract's arithmetic ------------------------------------------------------------------------------------------
def _split_weight_grads(m, em, terms):
    """gW_l = P_l^T in_l of the emulated arrays as split products (float32 sums; the rows are one slab)."""
    enc, H, G = em["enc"], em["H"], em["G"]
    out = []
    for l in range(8):
        if l == 0:
            out.append(product(G[0].t(), enc, terms))
        elif l == m.skip_at + 1:
            out.append(torch.cat([product(G[l].t(), enc, terms), product(G[l].t(), H[l - 1], terms)], dim=1))
        else:
            out.append(product(G[l].t(), H[l - 1], terms))
    return out


@pytest.mark.parametrize("kind,weights", [("deform", "default"), ("deform", "half_dead"), ("control", "default"),
                                          ("blender", "default"), ("A1", "default"), ("A64", "default")])  # fmt: skip
def test_emulated_products_against_float64(kind, weights):
    """Three terms hold the bar, two miss it: the trunk weight gradients as split products of the emulated chain's arrays,
    against the float64 run of the whole network, and against the float64 products of the same arrays."""
    c = case(kind, weights)
    m, ref = c["m"], c["ref"]
    em = emulate(m, c["x"], c["aux"], c["g_heads"])
    assert em["H"].shape == (8, ROWS, 256)
    want = trunk_weight_grads(m, ref["grads"])
    same = D.mlp_param_grads(em["enc"].double(), em["H"].double(), em["G"].double(), c["g_heads"].double(), head_rows(m))[0]
    three, two = _split_weight_grads(m, em, 3), _split_weight_grads(m, em, 2)
    e3 = max(rel_err(g, w) for g, w in zip(three, want))
    e2 = max(rel_err(g, w) for g, w in zip(two, want))
    s3 = max(rel_err(g, w) for g, w in zip(three, same))
    s2 = max(rel_err(g, w) for g, w in zip(two, same))
    print(f"mlp_wgrad_split emulation {kind} {weights}: whole network three {e3:.2e} two {e2:.2e}; same arrays three {s3:.2e} two {s2:.2e}")
    for g, w in zip(three, want):
        assert g.shape == w.shape
    assert e3 < REL_TOL < e2
    assert s3 < REL_TOL < s2
