"""CPU checks of the opt-in split-bf16 mode of the fused MLP calls (``FG_MLP_BF16X3``, include/fgraster.h): the capability
query and the descriptor's ``precision`` word across the C ABI (every call returns before a launch), the Python knobs, and
the arithmetic of the contract itself, emulated on the CPU (tests/mlp_split_common.py) against float64.

The emulation's measured errors (``max|a-b| / max|b|``, 1024 rows clear of the kink by 1e-4; three terms, then two):
about 5e-6 .. 1.5e-5 per array for the three-term product, some 1e-3 with the third term left out."""
import ctypes
import re
import subprocess

import pytest
import torch

from freegaussian_amd import _lib
from freegaussian_amd import deform as D
from freegaussian_amd import ops
from helpers import REL_TOL, rel_err
from mlp_common import PTR, desc, grads, header_text
from mlp_split_common import MARGIN, POOL, ROWS, case, emulate, product, split, trunk_weight_grads

OK, INVALID, WORKSPACE = 0, -1, -3
BIG = 1 << 40  # a workspace that would do (every call below is refused before a launch)


def _desc(precision, **kw):
    return desc(precision=precision, inputs=True, **kw)


def _grads():
    return grads(weight=(1,), bias=(), head_weight=(), head_bias=())


def _calls():
    """The five calls that honour ``precision``: name -> f(N, desc, workspace bytes)."""
    lib = _lib.load()
    a = ctypes.addressof
    g = _grads()
    return {
        "fg_mlp_fwd": lambda n, d, b: lib.fg_mlp_fwd(n, a(d), PTR, b, None),
        "fg_mlp_train_fwd": lambda n, d, b: lib.fg_mlp_train_fwd(n, a(d), PTR, PTR, PTR, PTR, b, None),
        "fg_mlp_bwd": lambda n, d, b: lib.fg_mlp_bwd(n, a(d), PTR, PTR, PTR, PTR, b, None),
        "fg_mlp_bwd_inputs": lambda n, d, b: lib.fg_mlp_bwd_inputs(n, a(d), PTR, PTR, PTR, PTR, PTR, b, None),
        "fg_mlp_train_bwd": lambda n, d, b: lib.fg_mlp_train_bwd(n, a(d), PTR, PTR, PTR, PTR, a(g), 0, PTR, b, None),
    }


def test_header_binding_and_library_agree_on_the_query():
    text = header_text()
    assert "int fg_mlp_precision_supported(int32_t precision);" in text
    assert "#define FG_MLP_FP32 0" in text and "#define FG_MLP_BF16X3 1" in text
    assert (_lib.MLP_FP32, _lib.MLP_BF16X3) == (0, 1)
    assert _lib.SIGNATURES["fg_mlp_precision_supported"] == (ctypes.c_int, [ctypes.c_int32])
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T fg_mlp_precision_supported$", exported, re.M)
    lib = _lib.load()
    assert [int(lib.fg_mlp_precision_supported(v)) for v in (0, 1, 7, -1, 2)] == [1, 1, 0, 0, 0]
    # the version numbers stay: the symbol is found by name
    assert "#define FG_ABI_VERSION 14" in text and "#define FG_ABI_MINOR 1 " in text and "BY NAME" in text


def test_the_descriptor_keeps_its_layout():
    fields = [n for n, _ in _lib.MlpDesc._fields_]
    assert "precision" in fields and "reserved" not in fields
    assert ctypes.sizeof(_lib.MlpDesc) == 12 * 4 + 8 + (2 + 8 + 8 + 3 * _lib.MLP_MAX_HEADS) * 8
    assert _lib.MlpDesc.precision.offset == 11 * 4 and _lib.MlpDesc.precision.size == 4
    assert _lib.MlpDesc().precision == _lib.MLP_FP32  # what every earlier caller passes
    text = header_text()
    body = text[text.index("typedef struct fg_mlp_desc {") : text.index("} fg_mlp_desc;")]
    assert re.search(r"int32_t head_rows\[FG_MLP_MAX_HEADS\];\s*int32_t precision;[^\n]*\n\s*int64_t aux_stride;", body)
    # fg_mlp_grads keeps its own reserved word
    assert [n for n, _ in _lib.MlpGrads._fields_][:2] == ["size", "reserved"]


@pytest.mark.parametrize("name", ["fg_mlp_fwd", "fg_mlp_train_fwd", "fg_mlp_bwd", "fg_mlp_bwd_inputs", "fg_mlp_train_bwd"])
def test_precision_is_validated_by_every_call_that_honours_it(name):
    call = _calls()[name]
    for bad in (7, 2, -1):
        assert call(100, _desc(bad), BIG) == INVALID, bad
    assert call(0, _desc(_lib.MLP_BF16X3), 0) == OK  # N = 0: nothing to do
    for good in (_lib.MLP_FP32, _lib.MLP_BF16X3):
        assert call(100, _desc(good), 0) == WORKSPACE  # everything else about it is accepted: the same need for both


def test_the_parameter_gradient_call_ignores_the_word():
    lib, g = _lib.load(), _grads()
    for precision in (0, 1, 7):
        d = _desc(precision)
        assert lib.fg_mlp_param_grads(100, ctypes.addressof(d), PTR, PTR, PTR, PTR, ctypes.addressof(g), PTR, 0, None) == WORKSPACE


def test_workspace_sizes_are_what_they_were():
    """The queries take no descriptor: one size for both precisions (the split planes have the fp32 packings' bytes)."""
    lib = _lib.load()
    fwd = 4 * (2048 * (16 + 6 * 32 + 48) + 16 * 256 + 16)  # the fp32 packing of the widest input row, and the heads
    bwd_t, tin = 4 * 2048 * (7 * 32 + 2), 4 * 2 * 32 * 128 * 8
    for n in (1, 64, 65, 33_000, 1_000_000):
        assert int(lib.fg_mlp_workspace_bytes(n)) == fwd
        assert int(lib.fg_mlp_train_workspace_bytes(n)) == max(fwd, bwd_t)
        assert int(lib.fg_mlp_bwd_inputs_workspace_bytes(n)) == max(fwd, bwd_t) + tin
    # the split forward packing of every aux width fits the documented size: steps of 16 against groups of 8
    for A in range(1, 65):
        s0 = (63 + A + 15) // 16
        assert 4 * (4096 * (s0 + 6 * 16 + s0 + 16) + 16 * 256 + 16) <= fwd, A


def test_fused_precision_knob(monkeypatch):
    monkeypatch.delenv("FG_FUSED_MLP_PRECISION", raising=False)
    assert D.fused_precision() == "fp32" and D._precision_keywords() == {}
    monkeypatch.setenv("FG_FUSED_MLP_PRECISION", "fp32")
    assert D.fused_precision() == "fp32" and D._precision_keywords() == {}
    monkeypatch.setenv("FG_FUSED_MLP_PRECISION", "bf16x3")
    assert D.fused_precision() == "bf16x3" and D._precision_keywords() == {"precision": "bf16x3"}
    assert D._train_keywords("2") == {"input_grads": True, "precision": "bf16x3"}
    for bad in ("bf16", "BF16X3", "1", ""):
        monkeypatch.setenv("FG_FUSED_MLP_PRECISION", bad)
        with pytest.raises(ValueError, match="FG_FUSED_MLP_PRECISION"):
            D.fused_precision()
    # no dispatch of its own: a call no fused path takes never reads the knob (CPU tensors: the torch ops)
    m = D.FreeGaussianDeformableModel()
    with torch.no_grad():
        assert m(torch.zeros(4, 3), torch.zeros(4, 1))[0].shape == (4, 4, 4)


def test_ops_rejects_an_unknown_precision():
    m = D.FreeGaussianDeformableModel()
    heads = (m.branch_w, m.branch_v, m.gaussian_rotation, m.gaussian_scaling)
    x, aux = torch.zeros(4, 3), torch.zeros(4, 21)
    for bad in ("bf16", "fp16", 1, None):
        with pytest.raises(ValueError, match="precision"):
            ops.mlp_forward(x, aux, m.linear, heads, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            ops.mlp_train(x, aux, m.linear, heads, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            ops.mlp_train_backward(torch.zeros(4, 88), torch.zeros(8, 4, 256), torch.zeros(4, 13), m.linear, heads, 21, (3, 3, 4, 3),
                                   precision=bad)  # fmt: skip


def test_split_is_the_contracts():
    v = torch.tensor([1.0, 1.0 + 2.0**-8, 1.0 + 2.0**-9, 3.14159274, -1e-3, 0.0, 1e30])
    hi, lo = split(v)
    assert torch.equal(hi, v.bfloat16().float()) and torch.equal(lo, (v - hi).bfloat16().float())
    assert float(hi[1]) == 1.0 and float(lo[1]) == 2.0**-8  # a tie: to even
    # hi + lo keeps 16 bits of the significand: the residue is below 2^-16 of the value's power of two
    assert bool(((v - hi - lo).abs() <= v.abs() * 2.0**-16).all())
    a, b = torch.randn(8, 32, generator=torch.Generator().manual_seed(0)), torch.randn(32, 8, generator=torch.Generator().manual_seed(1))
    exact = a.double() @ b.double()
    assert rel_err(product(a, b), exact) < 1e-4 < rel_err(product(a, b, terms=2), exact)


@pytest.mark.parametrize("kind,weights", [("deform", "default"), ("deform", "half_dead"), ("control", "default"),
                                          ("blender", "default"), ("A1", "default"), ("A64", "default")])  # fmt: skip
def test_emulated_contract_against_float64(kind, weights):
    """The written-down version of the issue's table: heads, P_l, g_enc and the trunk weight gradients of the three-term
    product stay below the bar on rows clear of the kink; without the third term the heads already miss it."""
    c = case(kind, weights)
    m, ref = c["m"], c["ref"]
    assert c["x"].shape[0] == ROWS and POOL == 4096 and MARGIN == 1e-4
    em = emulate(m, c["x"], c["aux"], c["g_heads"])
    in_ch = m.input_ch
    errs = {"raw": rel_err(em["raw"], ref["raw"]), "G": rel_err(em["G"], ref["G"]), "g_enc": rel_err(em["g_enc"], ref["g_enc"])}
    errs["gW"] = max(rel_err(g, w) for g, w in zip(em["grads"][0], trunk_weight_grads(m, ref["grads"])))
    print(f"mlp_split emulation {kind} {weights}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert em["g_enc"].shape == (ROWS, in_ch)
    for k, v in errs.items():
        assert v < REL_TOL, (k, v)
    two = emulate(m, c["x"], c["aux"], c["g_heads"], terms=2)
    assert rel_err(two["raw"], ref["raw"]) > REL_TOL
