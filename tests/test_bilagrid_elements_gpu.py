"""The fused bilateral-grid slice (csrc/bilagrid.hip through ``ops.bilagrid_apply``), every element of ``out``, ``v_rgb`` and
``v_grid`` compared with the float64 restatement of tests/bilagrid_restatement.py, one forward and one backward per shape.

Shapes, (H x W, grid X, Y, L) -- a row of the slice is cut into 256-pixel segments, a cell of the gather into 1024-pixel chunks:
    3 x 523, (7, 2, 3)      three segments of 256, 256 and 11 pixels; cx_lo = 0, 2, 5; 4, 5 and 2 x nodes in LDS
    5 x 257, (9, 3, 3)      a last segment of one pixel, the last column (t = 1); every 32nd pixel on an x node, every 2nd row
                            on a y node
    4 x 769, (3, 2, 2)      four segments; x cells of 384 and 385 pixels, two chunks per cell
    700 x 3, (2, 2, 2)      one cell, nx = 3, 2100 pixels: three chunks, the third partial
    7 x 130, (64, 64, 16)   the largest grid: 49 152 B of dynamic LDS; fewer rows than y nodes, so unreached nodes exist
    5 x 300, (64, 4, 16)    55 and 11 x nodes in two segments, cx_lo = 53
    2 x 2, (2, 2, 2)        the minimum: every pixel on a node
    9 x 49, (5, 3, 2)       (W-1) % (GX-1) == 0 and (H-1) % (GY-1) == 0: node pixels on both axes
    24 x 600, (16, 3, 8)    the coherent input: waves of the gather that hold pixels and skip levels; three segments
    37 x 53, (5, 4, 3)      camera 1 of 3: the odd case of tests/test_bilagrid_fused_gpu.py, now per element
(tests/test_bilagrid_elements_host.py asserts, from the integer maps, that each shape holds what its line says.)

PER ELEMENT:  |x_hip - x64| / A64  <=  F * E32(regime, array), no element left out, under every regime the element carries.
tests/parity_common.py has the protocol (A, E32, the floor, F); the fp32 restatement is plain numpy, F and FLOOR are
bilagrid_restatement's, the recorded table is in profiles/bilagrid_parity.md.
EXACT: a node no pixel reaches, and the blocks of the other cameras, are 0.0; every output is finite; a second forward and
backward gives the same bits; either gradient asked for alone gives the bits of the joint call.

``PYTHONPATH=. python tests/test_bilagrid_elements_gpu.py REPORT.jsonl`` turns the records of a run under FG_PARITY_REPORT into
the table of profiles/bilagrid_parity.md.
"""
import functools
import sys

import numpy as np
import pytest
import torch

import bilagrid_restatement as R
import parity_common as P
from freegaussian_amd import ops
from parity_common import need_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = ["%dx%d-%d-%d-%d-%s" % (s[0], s[1], s[2], s[3], s[4], s[7]) for s in R.SHAPES]


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _run(shape, want_rgb=True, want_grids=True):
    """One forward and one backward of ops.bilagrid_apply -> (out, v_rgb or None, v_grids [num,12,GL,GY,GX] or None), numpy."""
    c = R.regime_case(*shape)
    grids = _t(c["grids"]).requires_grad_(want_grids)
    rgb = _t(c["rgb"]).requires_grad_(want_rgb)
    out = ops.bilagrid_apply(grids, c["cam"], rgb)
    out.backward(_t(c["v_out"]))
    torch.cuda.synchronize()
    return tuple(None if a is None else a.detach().cpu().numpy() for a in (out, rgb.grad, grids.grad))


_first = functools.lru_cache(maxsize=None)(_run)  # the joint call, once per shape: what the other calls are compared with


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_every_element(shape):
    c = R.regime_case(*shape)
    out, v_rgb, v_grids = _first(shape)
    hip = {"out": out, "v_rgb": v_rgb, "v_grid": v_grids[c["cam"]]}
    failures = []
    for name in R.ARRAYS:  # every ratio is recorded before anything is asserted
        r64, masks, e32 = c["r64"], c["masks"][name], c["e32"][name]
        assert hip[name].shape == r64[name].shape and hip[name].dtype == np.float32
        # (every element carries a regime: tests/test_bilagrid_elements_host.py asserts it)
        d = P.distance(hip[name], r64[name], r64[name + "_acc"])
        P.check(f"{c['tag']}|{name}|{{regime}}", masks, d, e32, R.F, failures)
    for name, a in hip.items():
        assert bool(np.isfinite(a).all()), f"{name}: {int((~np.isfinite(a)).sum())} elements are not finite"
    unreached = c["r64"]["reach"] == 0
    stray = hip["v_grid"][:, unreached] != 0.0
    assert not stray.any(), f"{int(stray.sum())} sums of nodes that no pixel reaches are not exactly 0.0"
    assert bool((c["r64"]["v_grid_acc"][:, unreached] == 0).all())
    for i in range(v_grids.shape[0]):
        if i != c["cam"]:
            assert not v_grids[i].any(), f"the gradient block of camera {i} is not exactly 0.0"
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_second_call_gives_the_same_bits(shape):
    """No atomics, one order of addition: a second forward and backward equals the first bit for bit."""
    for name, a, b in zip(R.ARRAYS, _first(shape), _run(shape)):
        assert _same_bits(a, b), name


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_either_gradient_alone_gives_the_bits_of_the_joint_call(shape):
    """The slice backward and the gather are independent launches."""
    out, v_rgb, v_grids = _first(shape)
    out1, v_rgb1, none = _run(shape, want_grids=False)
    assert none is None and _same_bits(out, out1) and _same_bits(v_rgb, v_rgb1)
    out2, none, v_grids2 = _run(shape, want_rgb=False)
    assert none is None and _same_bits(out, out2) and _same_bits(v_grids, v_grids2)


def _report(path):
    """Markdown of a run's records (FG_PARITY_REPORT): per shape and array, the HIP ratio and (E32) of every regime."""
    ratio, e32 = P.read_records(path, "test_bilagrid_elements_gpu")
    worst = max(ratio, key=ratio.get)
    print(f"Bilateral-grid slice: worst ratio {ratio[worst]:.2f} at {' | '.join(worst)}; {len(ratio)} cells.\n")
    for arrays, cols in ((("out", "v_rgb"), R.PIXEL_REGIMES), (("v_grid",), R.NODE_REGIMES)):
        print("| shape | array | " + " | ".join(cols) + " |\n|---|---|" + "---|" * len(cols))
        for tag, what in dict.fromkeys(k[:2] for k in ratio if k[1] in arrays):
            cells = [f"{ratio[(tag, what, c)]:.2f} ({e32[(tag, what, c)]:.1e})" if (tag, what, c) in ratio else "" for c in cols]
            print(f"| {tag} | {what} | " + " | ".join(cells) + " |")
        print()


if __name__ == "__main__":
    _report(sys.argv[1])
