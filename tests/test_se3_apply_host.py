"""The fused SE(3) transform of the means, everything that is decided without a GPU: the float64 restatement of
tests/se3_restatement.py is torch's float64 autograd of ``deform._se3`` + ``utils.transform_points``; the bound of the GPU test
catches each wrong restatement, and that caps F; ``FG_FUSED_SE3`` is parsed in one place and, unset, changes nothing;
``forward`` is the heads method followed by ``_se3`` bit for bit; the header declares both entry points, found BY NAME, with the
ABI numbers unchanged; ``ops.se3_apply`` refuses CPU tensors; and the entry points' argument validation returns the header's
codes before any launch."""
import os
import re

import pytest
import torch

import parity_common as P
import se3_restatement as R
from freegaussian_amd import _lib, deform, ops
from freegaussian_amd.deform import FreeGaussianDeformableModel
from freegaussian_amd.utils import transform_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_BOUND = 1e-12  # max |restatement - autograd| / max |autograd| over an array, both float64


def _autograd64(c):
    w, v, x = (c[k].double().requires_grad_(True) for k in ("w", "v", "x"))
    out = transform_points(FreeGaussianDeformableModel._se3(w, v), x)
    (out * c["g"].double()).sum().backward()
    return {"out": out.detach(), "g_w": w.grad, "g_v": v.grad, "g_pts": x.grad}


def test_float64_restatement_is_torch_float64_autograd():
    """1e-12 of the array's largest element, on every array.  One array needs a word: float64 autograd forms g_w through
    1 / theta^2 times terms of size |v| |g| that cancel, so ITS OWN rounding is about 2^-52 |v| |g| / theta^2 -- 2e-9 of the row
    at theta = 1e-4, which no restatement can agree with to 1e-12 (measured: 5.8e-9 of a row, 6e-12 of the array's largest
    element).  g_w is therefore held to 1e-12 over the rows with theta >= 1e-2 (3584 of 4096), where that rounding is below
    1e-12, and row by row below 1e-2 to 1e-12 + 4 x that rounding (measured: at most 0.3 x).  out, g_v and g_pts: all rows."""
    c = R.regime_case(0)
    a64 = _autograd64(c)
    theta = c["w"].double().norm(dim=-1)
    sound = theta >= 1e-2
    for name in R.ARRAYS:
        rows = sound if name == "g_w" else torch.ones_like(sound)
        rel = float((c["r64"][name] - a64[name])[rows].abs().max() / a64[name][rows].abs().max())
        print(f"{name}: float64 restatement against float64 autograd, {rel:.2e} of the largest element over {int(rows.sum())} rows")
        assert rel <= TORCH_BOUND, (name, rel)
    d = P.distance(c["r64"]["g_w"], a64["g_w"], a64["g_w"], rows=True)
    own = 2.0**-52 * c["v"].double().norm(dim=-1) * c["g"].double().norm(dim=-1) / (theta * theta * a64["g_w"].norm(dim=-1))
    print(f"g_w below 1e-2: worst row {float(d[~sound].max()):.2e}, {float((d / own)[~sound].max()):.2f} x autograd's own rounding")
    assert bool((d[~sound] <= TORCH_BOUND + 4 * own[~sound]).all())


def test_regimes_hold_what_the_helper_says():
    c = R.regime_case(0)
    count = {k: int(m.sum()) for k, m in c["masks"].items()}
    print(count)
    assert [count[n] for n in R.REGIME_NAMES] == list(R.ROWS_PER_REGIME) and sum(R.ROWS_PER_REGIME) == R.ROWS == 4096
    assert 5 * (count[R.SMALL[0]] + count[R.SMALL[1]]) <= R.ROWS  # at most a fifth below 1e-2
    assert count["far_point"] == R.ROWS // R.FAR_EVERY
    assert all(int((c["masks"]["far_point"] & c["masks"][n]).sum()) >= 2 for n in R.REGIME_NAMES)
    far = c["x"][c["masks"]["far_point"]].norm(dim=-1)
    assert 50 < float(far.median()) < 200 and float(c["x"][~c["masks"]["far_point"]].norm(dim=-1).median()) < 4
    assert float(c["w"].double().norm(dim=-1).min()) >= 1e-4
    assert R.FLOOR == 16 * 2.0**-24
    for a in R.ARRAYS:
        assert bool(torch.isfinite(c["r64"][a]).all()) and bool(torch.isfinite(c["r32"][a]).all())
        for name, e in c["e32"][a].items():
            assert R.FLOOR <= e < 1e-3, (a, name, e)
    # the stable backward's yardstick stays at fp32 rounding where autograd's fp32 gradient of w is lost (profiles/se3_apply_parity.md)
    assert max(c["e32"]["g_w"][n] for n in R.SMALL) < 1e-5


def test_mutants_are_caught_and_cap_F():
    """Each deliberate mistake is at least 4 * F * E32 of the row from the true float64 result on three quarters of the rows:
    the largest F at which that holds is the mutant's cap, and F is at most the smallest."""
    caps = R.mutant_caps(0)
    assert {m for m, _ in caps} == set(R.MUTANTS) and len(R.MUTANTS) >= 4
    for (mutant, array), cap in caps.items():
        print(f"{mutant} | {array}: caps F at {cap:.3g}")
    smallest = min(caps.values())
    print(f"the cap on F: {smallest:.3g}")
    assert smallest >= 4  # (a bound of less than 4 x the yardstick would be no bound on a correct kernel either)
    assert R.F is None or R.F <= smallest


def test_F_is_set_from_the_committed_table():
    """F = 4 x the worst recorded ratio, rounded up to a power of two; the table is profiles/se3_apply_parity.md."""
    assert R.F is not None
    text = open(os.path.join(ROOT, "profiles", "se3_apply_parity.md")).read()
    worst = float(re.search(r"worst ratio ([0-9.]+)", text).group(1))
    want = 1.0
    while want < 4 * worst:
        want *= 2
    assert R.F == want, (R.F, worst, want)


@pytest.mark.parametrize("value,want", [(None, False), ("0", False), ("1", True)])
def test_knob_values(monkeypatch, value, want):
    if value is None:
        monkeypatch.delenv("FG_FUSED_SE3", raising=False)
    else:
        monkeypatch.setenv("FG_FUSED_SE3", value)
    assert deform.fused_se3() is want


@pytest.mark.parametrize("value", ["yes", "", "2", "true"])
def test_knob_typo_is_an_error_naming_the_variable(monkeypatch, value):
    monkeypatch.setenv("FG_FUSED_SE3", value)
    with pytest.raises(ValueError, match="FG_FUSED_SE3"):
        deform.fused_se3()


def test_knob_is_read_in_one_place():
    hits = []
    for base, _, files in os.walk(os.path.join(ROOT, "freegaussian_amd")):
        for f in files:
            if f.endswith(".py") and re.search(r"environ[^\n]*FG_FUSED_SE3", open(os.path.join(base, f)).read()):
                hits.append(f)
    assert hits == ["deform.py"]


def _small_net(seed=0):
    torch.manual_seed(seed)
    net = FreeGaussianDeformableModel()
    x, t = torch.randn(37, 3), torch.rand(1, 1).expand(37, -1)
    return net, x, t


def test_forward_is_heads_then_se3_bit_for_bit():
    net, x, t = _small_net()
    T, rot, scale = net(x, t)
    w, v, rot2, scale2 = net.heads(x, t)
    assert w.shape == v.shape == (37, 3) and rot2.shape == (37, 4) and scale2.shape == (37, 3)
    assert torch.equal(T, net._se3(w, v)) and torch.equal(rot, rot2) and torch.equal(scale, scale2)
    assert T.shape == (37, 4, 4)
    # and the gradients of a loss through all three outputs
    grads = []
    for run in (lambda: net(x, t), lambda: (lambda w, v, r, s: (net._se3(w, v), r, s))(*net.heads(x, t))):
        net.zero_grad()
        T, rot, scale = run()
        (T.square().sum() + rot.sum() + scale.square().sum()).backward()
        grads.append([p.grad.clone() for p in net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_unset_knob_never_calls_the_fused_op(monkeypatch):
    """A CPU forward and backward of the deformation net and the transform of the points with ``ops.se3_apply`` replaced by
    something that raises."""

    def boom(*a, **k):
        raise AssertionError("ops.se3_apply called with FG_FUSED_SE3 unset")

    monkeypatch.delenv("FG_FUSED_SE3", raising=False)
    monkeypatch.setattr(ops, "se3_apply", boom)
    net, x, t = _small_net(1)
    T, _, _ = net(x, t)
    transform_points(T, x).sum().backward()
    from freegaussian_amd import model

    assert model._se3_fused_for(x, t) is False
    monkeypatch.setenv("FG_FUSED_SE3", "1")
    assert model._se3_fused_for(x, t) is False  # (CPU tensors keep the torch ops whatever the knob says)


def test_ops_se3_apply_refuses_cpu_tensors():
    a = torch.randn(5, 3)
    with pytest.raises(_lib.FgRasterError, match="GPU only"):
        ops.se3_apply(a, a.clone(), a.clone())
    with pytest.raises(ValueError):
        ops.se3_apply(a, a.clone(), torch.randn(4, 3))


def test_header_declares_both_symbols_by_name_and_abi_numbers_stay():
    text = open(os.path.join(ROOT, "include", "fgraster.h")).read()
    assert re.search(r"#define FG_ABI_VERSION 14\b", text) and re.search(r"#define FG_ABI_MINOR 1\b", text)
    assert (_lib.ABI_VERSION, _lib.ABI_MINOR) == (14, 1)
    note = text[text.index("#define FG_ABI_MINOR") : text.index("#define FG_COUNT_OUT_WORDS")]
    assert re.search(r"BY NAME: fg_se3_apply_fwd and fg_se3_apply_bwd", note)
    section = text[text.index("/* ---- SE ") :]
    assert "found BY NAME" in section.split("*/")[0]
    for name in ("fg_se3_apply_fwd", "fg_se3_apply_bwd"):
        assert re.search(r"^int %s\(int64_t N, const float\* w, int64_t w_stride," % name, section, re.M), name
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.fg_abi_version() == 14 and lib.fg_abi_minor() == 1
    assert hasattr(lib, "fg_se3_apply_fwd") and hasattr(lib, "fg_se3_apply_bwd")


def test_argument_validation_returns_before_any_launch():
    """Through ctypes, without a GPU: every call here is refused (or has nothing to do) before it would launch."""
    lib = _lib.load()
    OK, INVALID, UNSUPPORTED = 0, -1, -4
    at = lambda i: (1 << 30) + (i << 24)  # noqa: E731  addresses nobody reads, 16 MiB apart
    N = 1000
    fwd = lambda *a: lib.fg_se3_apply_fwd(*a, None)  # noqa: E731
    bwd = lambda *a: lib.fg_se3_apply_bwd(*a, None)  # noqa: E731
    assert lib.fg_error_string(INVALID) and lib.fg_error_string(UNSUPPORTED)
    # row counts
    for n in (-(2**63), -1):
        assert fwd(n, at(0), 3, at(1), 3, at(2), at(3)) == INVALID
        assert bwd(n, at(0), 3, at(1), 3, at(2), at(3), at(4), 3, at(5), 3, at(6)) == INVALID
    assert fwd(0, at(0), 3, at(1), 3, at(2), at(3)) == OK
    assert bwd(0, at(0), 3, at(1), 3, at(2), at(3), at(4), 3, at(5), 3, at(6)) == OK
    assert fwd(2**38 + 1, at(0), 3, at(1), 3, at(2), at(3)) == UNSUPPORTED
    assert bwd(2**63 - 1, at(0), 3, at(1), 3, at(2), at(3), at(4), 3, at(5), 3, at(6)) == UNSUPPORTED
    # null pointers
    for k in range(4):
        args = [at(0), 3, at(1), 3, at(2), at(3)]
        args[(0, 2, 4, 5)[k]] = None
        assert fwd(N, *args) == INVALID
    for k in range(4):
        args = [at(0), 3, at(1), 3, at(2), at(3), at(4), 3, at(5), 3, at(6)]
        args[(0, 2, 4, 5)[k]] = None
        assert bwd(N, *args) == INVALID
    assert bwd(N, at(0), 3, at(1), 3, at(2), at(3), None, 0, None, 0, None) == OK  # nothing asked for
    # strides
    for s in (2, 0, -3):
        assert fwd(N, at(0), s, at(1), 3, at(2), at(3)) == INVALID
        assert fwd(N, at(0), 3, at(1), s, at(2), at(3)) == INVALID
        assert bwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), s, at(5), 3, at(6)) == INVALID
        assert bwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 3, at(5), s, at(6)) == INVALID
    assert fwd(N, at(0), 2**16 + 1, at(1), 3, at(2), at(3)) == UNSUPPORTED
    # aliasing, whole and by the last float, with strides 3 and 13
    rows = 4 * (3 * N - 1)  # bytes from the first to the last float of a contiguous [N,3]
    for s, w, v in ((3, at(0), at(1)), (13, at(7), at(7) + 12)):
        span = 4 * ((N - 1) * s + 2)
        for bad in (w, v, at(2), w + span, v + span, at(2) + rows, w - rows, at(2) - rows):
            assert fwd(N, w, s, v, s, at(2), bad) == INVALID
            for o in range(3):
                outs = [at(4), 3, at(5), 3, at(6)]
                outs[2 * o] = bad
                assert bwd(N, w, s, v, s, at(2), at(3), *outs) == INVALID
                alone = [None, 3, None, 3, None]
                alone[2 * o] = bad
                assert bwd(N, w, s, v, s, at(2), at(3), *alone) == INVALID
        assert bwd(N, w, s, v, s, at(2), at(3), at(3), 3, None, 0, None) == INVALID  # on g_out
        assert bwd(N, w, s, v, s, at(2), at(3), at(4), 3, at(4) + rows, 3, at(6)) == INVALID  # outputs on each other
        assert bwd(N, w, s, v, s, at(2), at(3), at(4), 3, at(5), 3, at(5) - rows) == INVALID
