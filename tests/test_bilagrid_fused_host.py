"""The fused bilateral-grid slice (csrc/bilagrid.hip, ops.bilagrid_apply, FG_FUSED_BILAGRID), as far as a machine without a
GPU can check it: the float64 restatement the GPU tests compare against is pinned to the torch path on the CPU; the four
symbols are declared, bound and exported; the queries and the argument validation answer before any launch; the knob
parses; nothing but a CUDA tensor with the knob set reaches the fused call."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bilagrid_restatement as R
from freegaussian_amd import _lib, bilagrid, ops
from freegaussian_amd.bilagrid import BilateralGrid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fg_bilagrid_supported", "fg_bilagrid_bwd_workspace_bytes", "fg_bilagrid_slice_fwd", "fg_bilagrid_slice_bwd")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def _module(grids):
    num, _, GL, GY, GX = grids.shape
    m = BilateralGrid(num=num, grid_X=GX, grid_Y=GY, grid_W=GL)
    with torch.no_grad():
        m.grids.copy_(torch.from_numpy(np.array(grids)))
    return m


@pytest.mark.parametrize("H,W,GX,GY,GL,num,cam", [(7, 9, 5, 4, 3, 2, 1), (37, 53, 5, 4, 3, 3, 1), (12, 14, 16, 16, 8, 1, 0)])
def test_restatement_matches_the_torch_path_on_the_cpu(monkeypatch, H, W, GX, GY, GL, num, cam):
    """fp32 torch (grid_sample + multiply, autograd) against the float64 restatement: values and both gradients within 1e-5
    of each array's largest magnitude, on the repaired inputs -- black, white and out-of-range pixels included, none
    excluded."""
    monkeypatch.delenv("FG_FUSED_BILAGRID", raising=False)
    c = R.case(H, W, GX, GY, GL, num, cam)
    assert R.clear_of_knife_edges(c["rgb"], GL)
    m = _module(c["grids"])
    rgb = torch.from_numpy(np.array(c["rgb"])).requires_grad_(True)
    out = bilagrid.apply_to_render(m, rgb.unsqueeze(0), cam, H, W).squeeze(0)
    (out * torch.from_numpy(np.array(c["v_out"]))).sum().backward()
    errs = {"out": _rel(out.detach().numpy(), c["out"]), "v_rgb": _rel(rgb.grad.numpy(), c["v_rgb"]),
            "v_grid": _rel(m.grids.grad[cam].numpy(), c["v_grid"])}  # fmt: skip
    print("restatement against fp32 torch:", errs)
    assert all(e <= 1e-5 for e in errs.values()), errs
    others = [i for i in range(num) if i != cam]
    assert all(float(m.grids.grad[i].abs().max()) == 0.0 for i in others)
    # the guidance term: none at black, white and out-of-range pixels (v_rgb is A^T v_out alone there)
    z = R.guidance(c["rgb"], GL)
    assert ((z <= 0) | (z >= GL - 1)).sum() >= 8


def test_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "fgraster.h")).read()
    assert "#define FG_ABI_VERSION 14" in text and "#define FG_ABI_MINOR 1 " in text
    assert _lib.ABI_VERSION == 14 and _lib.ABI_MINOR == 1
    by_name = text[text.index("BY NAME") : text.index("#define FG_COUNT_OUT_WORDS")]
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    exported = set(re.findall(r" T (fg_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)))
    for name in NAMES:
        assert name in by_name, name
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _lib.SIGNATURES and name in exported and getattr(lib, name) is not None
    m = re.search(r"^#define FG_BILAGRID_CHUNK_PIXELS (\d+)", text, flags=re.M)
    assert m and int(m.group(1)) == 1024
    srcs = re.search(r"^SRCS := (.*)$", open(os.path.join(ROOT, "freegaussian_amd", "csrc", "Makefile")).read(), flags=re.M).group(1)
    assert "bilagrid.hip" in srcs.split()


def test_queries_and_validation_answer_without_a_gpu():
    lib = _lib.load()
    for GX, GY, GL, want in ((2, 2, 2, 1), (64, 64, 16, 1), (16, 16, 8, 1), (5, 4, 3, 1), (1, 16, 8, 0), (16, 1, 8, 0),
                             (16, 16, 1, 0), (65, 16, 8, 0), (16, 65, 8, 0), (16, 16, 17, 0), (-3, 16, 8, 0), (0, 0, 0, 0)):  # fmt: skip
        assert lib.fg_bilagrid_supported(GX, GY, GL) == want, (GX, GY, GL)
    q = lib.fg_bilagrid_bwd_workspace_bytes
    # chunks of the largest cell x GL x (4 corners x 12) x cells x 4 bytes; the cell of c: pixels ceil(c (S-1) / (n-1)) ...
    def longest(S, n):  # the header's rule, restated: the last cell also holds the pixel on the last node
        first = [-(-c * (S - 1) // (n - 1)) for c in range(n - 1)] + [S]
        return max(b - a for a, b in zip(first, first[1:]))

    def want_bytes(H, W, GX, GY, GL):
        return -(-longest(W, GX) * longest(H, GY) // 1024) * GL * 48 * (GX - 1) * (GY - 1) * 4

    for shape in ((1080, 1920, 16, 16, 8), (96, 160, 16, 16, 8), (37, 53, 5, 4, 3), (65, 65, 3, 3, 2), (61, 65, 3, 3, 2), (12, 14, 16, 16, 8)):
        assert q(*shape) == want_bytes(*shape), shape
    assert q(1080, 1920, 16, 16, 8) == 9 * 8 * 48 * 225 * 4  # cells of at most 128 x 72 = 9216 pixels: 9 chunks of 1024
    assert q(65, 65, 3, 3, 2) == 2 * 2 * 48 * 4 * 4  # the last cell holds 33 x 33 = 1089 pixels
    assert q(61, 65, 3, 3, 2) == 1 * 2 * 48 * 4 * 4  # 33 x 31
    assert q(1, 53, 5, 4, 3) == 0 and q(37, 1, 5, 4, 3) == 0 and q(37, 53, 65, 4, 3) == 0 and q(37, 53, 5, 4, 17) == 0
    assert q(16385, 53, 5, 4, 3) == 0 and q(16384, 16384, 64, 64, 16) > 0
    p, big = 4096, 1 << 40  # (an address nobody reads: every call below returns before a launch)
    fwd, bwd = lib.fg_bilagrid_slice_fwd, lib.fg_bilagrid_slice_bwd
    INVALID, WORKSPACE, UNSUPPORTED = -1, -3, -4
    img = 37 * 53 * 12
    assert fwd(37, 53, 5, 4, 3, None, p, p + (1 << 20), None) == INVALID
    assert fwd(37, 53, 5, 4, 3, p, None, p + (1 << 20), None) == INVALID
    assert fwd(37, 53, 5, 4, 3, p, p + (1 << 20), None, None) == INVALID
    assert fwd(1, 53, 5, 4, 3, p, p + (1 << 20), p + (2 << 20), None) == INVALID
    assert fwd(37, 1, 5, 4, 3, p, p + (1 << 20), p + (2 << 20), None) == INVALID
    assert fwd(37, 53, 5, 4, 3, p, p + (1 << 20), p + (1 << 20), None) == INVALID  # out aliases rgb
    assert fwd(37, 53, 5, 4, 3, p, p + (1 << 20), p + (1 << 20) + img - 4, None) == INVALID  # ... by one float
    assert fwd(37, 53, 65, 4, 3, p, p + (1 << 20), p + (2 << 20), None) == UNSUPPORTED
    assert fwd(37, 53, 5, 4, 1, p, p + (1 << 20), p + (2 << 20), None) == UNSUPPORTED
    a, b, c, d, e, w = (p + (i << 24) for i in range(6))  # grid, rgb, v_out, v_rgb, v_grid, workspace
    need = q(37, 53, 5, 4, 3)
    assert bwd(37, 53, 5, 4, 3, None, b, c, d, e, w, big, None) == INVALID
    assert bwd(37, 53, 5, 4, 3, a, None, c, d, e, w, big, None) == INVALID
    assert bwd(37, 53, 5, 4, 3, a, b, None, d, e, w, big, None) == INVALID
    assert bwd(1, 53, 5, 4, 3, a, b, c, d, e, w, big, None) == INVALID
    assert bwd(37, 53, 5, 4, 3, a, b, c, b, e, w, big, None) == INVALID  # v_rgb aliases rgb
    assert bwd(37, 53, 5, 4, 3, a, b, c, c, e, w, big, None) == INVALID  # ... v_out
    assert bwd(37, 53, 5, 4, 3, a, b, c, d, a, w, big, None) == INVALID  # v_grid aliases grid
    assert bwd(37, 53, 5, 4, 3, a, b, c, d, e, None, big, None) == INVALID
    assert bwd(37, 53, 5, 4, 3, a, b, c, d, e, w + 4, big, None) == INVALID  # misaligned
    assert bwd(37, 53, 5, 4, 3, a, b, c, d, e, e, big, None) == INVALID  # the workspace is v_grid
    assert bwd(37, 53, 5, 4, 3, a, b, c, d, e, w, need - 1, None) == WORKSPACE
    assert bwd(37, 53, 5, 4, 3, a, b, c, d, e, w, 0, None) == WORKSPACE
    assert bwd(37, 53, 5, 2, 17, a, b, c, d, e, w, big, None) == UNSUPPORTED
    assert bwd(37, 53, 5, 4, 3, a, b, c, None, None, None, 0, None) == 0  # neither gradient asked for: nothing to do


def test_knob_parses_and_cpu_tensors_never_take_the_fused_call(monkeypatch):
    g = BilateralGrid(num=2, grid_X=5, grid_Y=4, grid_W=3)
    rgb = torch.rand(1, 9, 7, 3)
    monkeypatch.delenv("FG_FUSED_BILAGRID", raising=False)
    assert bilagrid.fused_bilagrid() is False and bilagrid.fused_applies(g, rgb) is False
    monkeypatch.setenv("FG_FUSED_BILAGRID", "0")
    assert bilagrid.fused_bilagrid() is False and bilagrid.fused_applies(g, rgb) is False
    monkeypatch.setenv("FG_FUSED_BILAGRID", "1")
    assert bilagrid.fused_bilagrid() is True and bilagrid.fused_applies(g, rgb) is False  # CPU tensors
    for bad in ("", "yes", "2", "true", " 1"):
        monkeypatch.setenv("FG_FUSED_BILAGRID", bad)
        with pytest.raises(ValueError, match="FG_FUSED_BILAGRID"):
            bilagrid.fused_bilagrid()
        with pytest.raises(ValueError, match="FG_FUSED_BILAGRID"):
            bilagrid.apply_to_render(g, rgb, 1, 9, 7)
    with pytest.raises(_lib.FgRasterError):
        ops.bilagrid_apply(g.grids, 1, rgb[0])
    with pytest.raises(ValueError):
        ops.bilagrid_apply(g.grids[0], 0, rgb[0])


def test_knob_unset_never_reaches_the_fused_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("ops.bilagrid_apply reached")

    monkeypatch.setattr(ops, "bilagrid_apply", boom)
    g = BilateralGrid(num=2, grid_X=5, grid_Y=4, grid_W=3)
    rgb = torch.rand(1, 9, 7, 3, requires_grad=True)
    for knob in (None, "0", "1"):  # ("1": CPU tensors stay on the torch ops too)
        monkeypatch.delenv("FG_FUSED_BILAGRID", raising=False) if knob is None else monkeypatch.setenv("FG_FUSED_BILAGRID", knob)
        out = bilagrid.apply_to_render(g, rgb, 1, 9, 7)
        assert torch.allclose(out, rgb, atol=1e-6)
        out.sum().backward()
