"""CPU checks of the fused MLP forward's host side: the C ABI's argument validation and workspace query (no device is
touched: every call returns before a launch), and the dispatch predicate, which is false for CPU tensors so that both
modules keep matching the reference's outputs (tests/golden/g_mlp.npz) through the torch path."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from freegaussian_amd import _lib
from freegaussian_amd import deform as D
from freegaussian_amd import ops
from mlp_common import PTR, addr, desc, header_text

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
from make_golden import fill_params  # noqa: E402  (pure helper)

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4


def _desc(mode=_lib.MLP_SE3, A=21, head_rows=(3, 3, 4, 3), ptr=PTR):
    """A descriptor whose pointers are set to an address nobody reads (every call below is refused before a launch)."""
    return desc(mode, A, head_rows, inputs=True, outs=True, ptr=ptr)


def _fwd(n, d, ws=PTR, ws_bytes=0):
    """(workspace_bytes = 0: a descriptor that passes every other check still stops at FG_ERR_WORKSPACE)"""
    return _lib.load().fg_mlp_fwd(n, addr(d), ws, ws_bytes, None)


def test_descriptor_matches_the_header():
    text = header_text()
    for name, value in (("FG_MLP_ROW_TILE", _lib.MLP_ROW_TILE), ("FG_MLP_MAX_HEADS", _lib.MLP_MAX_HEADS),
                        ("FG_MLP_SE3", _lib.MLP_SE3), ("FG_MLP_PLAIN", _lib.MLP_PLAIN)):  # fmt: skip
        assert f"#define {name} {value}" in text, name
    assert ctypes.sizeof(_lib.MlpDesc) == 12 * 4 + 8 + (2 + 8 + 8 + 3 * _lib.MLP_MAX_HEADS) * 8
    assert ops.MLP_ROW_TILE == _lib.MLP_ROW_TILE


def test_nothing_to_do_and_invalid_arguments_without_gpu():
    assert _fwd(0, None, None, 0) == OK  # N = 0: nothing to do, nothing is looked at
    assert _fwd(0, _desc(A=0)) == OK
    assert _fwd(-1, _desc()) == INVALID
    assert _fwd(100, None) == INVALID
    good = _desc()
    assert _fwd(100, good) == WORKSPACE  # everything else about it is accepted
    assert _fwd(100, _desc(_lib.MLP_PLAIN, 63, (3, 4, 3))) == WORKSPACE
    assert _fwd(100, _desc(_lib.MLP_PLAIN, 1, (16,))) == WORKSPACE and _fwd(100, _desc(_lib.MLP_PLAIN, 64, (1,))) == WORKSPACE
    # aux width outside 1..64
    for A in (0, -3, 65, 1000):
        assert _fwd(100, _desc(A=A)) == INVALID, A
    # head rows outside 1..16, alone or together; no head; too many heads
    for rows in ((0,), (17,), (-1, 3), (8, 9), (16, 1), (4, 4, 4, 5)):
        assert _fwd(100, _desc(_lib.MLP_PLAIN, 21, rows)) == INVALID, rows
    for n_heads in (0, _lib.MLP_MAX_HEADS + 1):
        d = _desc()
        d.n_heads = n_heads
        assert _fwd(100, d) == INVALID
    assert _fwd(100, _desc(_lib.MLP_SE3, 21, (3, 4, 3))) == INVALID  # SE(3) wants (w, v, rotation, scaling)
    # an unknown mode
    for mode in (-1, 2, 7):
        assert _fwd(100, _desc(mode)) == INVALID, mode
    # a descriptor of another size
    d = _desc()
    d.size -= 8
    assert _fwd(100, d) == INVALID
    # a null required pointer with N > 0 (and a workspace that would do)
    big = 1 << 40
    for field in ("x", "aux"):
        d = _desc()
        setattr(d, field, None)
        assert _fwd(100, d, 4096, big) == INVALID, field
    for field, count in (("weight", 8), ("bias", 8), ("head_weight", 4), ("head_bias", 4)):
        for i in range(count):
            d = _desc()
            getattr(d, field)[i] = None
            assert _fwd(100, d, 4096, big) == INVALID, (field, i)
    assert _fwd(100, _desc(), None, big) == INVALID  # no workspace
    assert _fwd(100, _desc(), 4100, big) == INVALID  # ... or one that is not 16-byte aligned
    d = _desc()
    d.aux_stride = -21
    assert _fwd(100, d) == INVALID
    # other network shapes: unsupported, so that a caller can fall back
    for field, value in (("depth", 6), ("width", 128), ("multires", 6)):
        d = _desc()
        setattr(d, field, value)
        assert _fwd(100, d) == UNSUPPORTED, field
    need = int(_lib.load().fg_mlp_workspace_bytes(100))
    assert _fwd(100, _desc(), 4096, need - 1) == WORKSPACE


def test_workspace_query_is_monotone_in_n():
    lib = _lib.load()
    sizes = [int(lib.fg_mlp_workspace_bytes(n)) for n in (0, 1, 63, 64, 65, 1000, 33_000, 240_000, 1_000_000, 1 << 33)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    # the re-ordered copy of the widest network: 8 layers of [256, <= 128 | 256 | 384] floats and the heads
    assert sizes[-1] >= 4 * 256 * (128 + 6 * 256 + 384 + 16)
    assert int(lib.fg_mlp_workspace_bytes(-1)) == 0


def test_ops_refuses_cpu_tensors_and_bad_shapes():
    m = D.FreeGaussianDeformableModel()
    heads = (m.branch_w, m.branch_v, m.gaussian_rotation, m.gaussian_scaling)
    x, aux = torch.zeros(4, 3), torch.zeros(4, 21)
    with pytest.raises(_lib.FgRasterError):
        ops.mlp_forward(x, aux, m.linear, heads)
    with pytest.raises(ValueError):
        ops.mlp_forward(torch.zeros(4, 2), aux, m.linear, heads)
    with pytest.raises(ValueError):
        ops.mlp_forward(x, torch.zeros(3, 21), m.linear, heads)
    with pytest.raises(ValueError):
        ops.mlp_forward(x, torch.zeros(4, 65), m.linear, heads)
    with pytest.raises(ValueError):
        ops.mlp_forward(x, aux, list(m.linear)[:7], heads)
    with pytest.raises(ValueError):
        ops.mlp_forward(x, aux, m.linear, heads, mode="affine")


def _load(name):
    z = np.load(os.path.join(GOLD, name))
    return lambda k: torch.from_numpy(z[k])


def test_dispatch_is_off_for_cpu_tensors_and_the_modules_still_match_the_reference(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "mlp_forward", lambda *a, **k: calls.append(a) or pytest.fail("fused call on CPU tensors"))
    t = _load("g_mlp.npz")
    big = torch.zeros(D.FUSED_MIN_ROWS, 3)
    for tag, kw in (("deform", {}), ("deform_blender", {"is_blender": True})):
        m = D.FreeGaussianDeformableModel(**kw)
        fill_params(m)
        with torch.no_grad():
            assert not D.fused_applies(m, big, torch.zeros(D.FUSED_MIN_ROWS, 1))
            for ti, tt in enumerate((0.0, 0.5, 1.0)):
                dx, rot, sc = m(t("x"), torch.full((16, 1), tt))
                assert torch.allclose(dx, t(f"{tag}.t{ti}.d_xyz"), atol=1e-6)
                assert torch.allclose(rot, t(f"{tag}.t{ti}.rot"), atol=1e-6)
                assert torch.allclose(sc, t(f"{tag}.t{ti}.scale"), atol=1e-6)
    m = D.FreeGaussianControllableModel()
    fill_params(m)
    with torch.no_grad():
        assert not D.fused_applies(m, big, torch.zeros(D.FUSED_MIN_ROWS, 3))
        dx, rot, sc = m(t("x"), t("control.value"))
    assert torch.allclose(dx, t("control.d_xyz"), atol=1e-6) and torch.allclose(rot, t("control.rot"), atol=1e-6)
    assert torch.allclose(sc, t("control.scale"), atol=1e-6)
    assert not calls
    assert D.FUSED_MIN_ROWS >= 4 * D._TallLinear.CHUNK == 32768  # raised by measurement if need be, never lowered
