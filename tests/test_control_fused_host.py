"""The fused stage-2 control stage (``FG_FUSED_CONTROL``), what can be pinned without a GPU: the plan of a mask against brute
force, its cache in the model, the restatements of tests/control_restatement.py against the torch lines of
``FreeGaussianControlModel._control_stage``, the knob, ``fused_control_applies``, and a CPU model that computes what it
computed whatever the knob says."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import control_restatement as R
import make_golden as G
from freegaussian_amd import _lib, deform, model as model_mod, ops
from freegaussian_amd.model import Camera, FreeGaussianControlModel, FreeGaussianModelConfig, OrientedBox


def _random_mask():
    g = torch.Generator().manual_seed(3)
    mask = torch.rand(300, 32, generator=g) < 0.08
    mask[17] = True  # (all 32 bits: the word 0xffffffff)
    mask[40:60] = False
    mask[5, 31] = True
    return mask


MASKS = {"base": lambda: G.control_mask("base"), "overlap": lambda: G.control_mask("overlap"), "random": _random_mask}


@pytest.mark.parametrize("name", list(MASKS))
def test_plan_contents_against_brute_force(name):
    mask = MASKS[name]()
    plan = ops.control_plan(mask)
    sel, bits, rank, counts = R.plan_brute(mask)
    assert (plan.N, plan.M, plan.n) == (mask.shape[0], mask.shape[1], len(sel)) and 0 < plan.n < plan.N
    assert plan.sel_index.dtype == torch.int32 and plan.sel_index.tolist() == sel
    assert plan.sel_index64.dtype == torch.int64 and plan.sel_index64.tolist() == sel
    assert plan.bits.dtype == torch.uint32 and plan.bits.view(torch.int32).to(torch.int64).bitwise_and(0xFFFFFFFF).tolist() == bits
    assert plan.rank.dtype == torch.int32 and plan.rank.tolist() == rank
    assert plan.counts.dtype == torch.int32 and plan.counts.tolist() == counts and plan.counts_host == tuple(counts)
    assert list(plan._counts_c) == counts
    assert torch.equal(R.mask_of_bits(plan.bits.view(torch.int32), plan.M), mask[plan.sel_index64])
    assert plan.refusal() is None
    if name == "random":
        assert 0xFFFFFFFF in bits and max(bits) >= 2**31


def test_plan_refuses_what_it_cannot_hold():
    with pytest.raises(ValueError):
        ops.control_plan(torch.zeros(10, 33, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.control_plan(torch.zeros(10, 0, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.control_plan(torch.zeros(10, 3))
    with pytest.raises(ValueError):
        ops.control_plan(torch.zeros(10, dtype=torch.bool))
    empty = G.control_mask("base")
    empty[:, 2] = False
    assert "attribute 2" in ops.control_plan(empty).refusal()
    assert "no row" in ops.control_plan(torch.zeros(10, 3, dtype=torch.bool)).refusal()


def _control_model(mask=None, n=G.CONTROL_N):
    torch.manual_seed(0)
    init = Camera(torch.eye(4)[None, :3], 50.0, 50.0, 16.0, 16.0, 32, 32, times=torch.tensor([[0.0]]))
    cm = FreeGaussianControlModel(G.control_mask("base") if mask is None else mask, init,
                                  config=FreeGaussianModelConfig(background_color="black"), seed_points=torch.rand(n, 3) - 0.5,
                                  init_scales=-3.0)  # fmt: skip
    cam = Camera(init.camera_to_worlds, 50.0, 50.0, 16.0, 16.0, 32, 32, times=torch.tensor([[0.7]]), metadata={"cameras0": init})
    return cm, cam


def test_model_rebuilds_the_plan_when_the_mask_changes():
    cm, _ = _control_model()
    first = cm._control_plan()
    assert cm._control_plan() is first  # kept
    cm.gaussian_mask[130:140, 1] = True  # an in-place edit
    second = cm._control_plan()
    assert second is not first and second.n == first.n + 10 and second.counts_host[1] == first.counts_host[1] + 10
    assert cm._control_plan() is second
    cm.gaussian_mask = cm.gaussian_mask.clone()  # a new tensor of the same contents
    third = cm._control_plan()
    assert third is not second and third.sel_index.tolist() == second.sel_index.tolist()
    cm.gaussian_mask = cm.gaussian_mask[:, :2].contiguous()  # another shape
    assert cm._control_plan().M == 2
    keys = {model_mod._mask_key(m) for m in (cm.gaussian_mask, cm.gaussian_mask.clone())}
    assert len(keys) == 2


@pytest.mark.parametrize("name", list(MASKS))
def test_restatement_equals_the_torch_lines(name):
    """The float64 statements against the torch lines evaluated in float64, the fp32 ones within the derived bounds of the
    float64 ones (the mean: torch's own; the value rows: the kernel's order and torch's product), the scatter bit for bit
    through the plan's indices as through the boolean mask."""
    mask = MASKS[name]()
    plan = ops.control_plan(mask)
    sel = mask.any(-1)
    pmask = mask[sel]
    g = torch.Generator().manual_seed(11)
    a, b = torch.randn(plan.n, 3, generator=g), torch.randn(plan.n, 3, generator=g)
    x64, A64 = R.attr_mean64(a, b, pmask)
    delta64 = (a - b).double()
    assert torch.allclose(x64, R.attr_mean_torch(delta64, torch.zeros_like(delta64), pmask), rtol=1e-13, atol=1e-15)
    # torch's fp32 mean sums in fp32: n 2^-24 of the magnitudes at the worst, far outside the fused bound and inside this one
    d_avg = R.attr_mean_torch(a, b, pmask)
    assert bool(((d_avg.double() - x64).abs() <= 2.0**-23 * x64.abs() + plan.n * 2.0**-24 * A64).all())
    v64, s_over_p = R.value_rows64(pmask, d_avg)
    assert torch.allclose(v64, pmask.double() @ d_avg.double() / pmask.sum(-1, keepdim=True), rtol=1e-13, atol=1e-15)  # (:140 in float64)
    bound = R.value_rows_bound(pmask, s_over_p)
    for v32 in (R.value_rows32(pmask, d_avg), R.value_rows_torch(pmask, d_avg)):
        assert v32.dtype == torch.float32 and bool(((v32.double() - v64).abs() <= bound).all())
    # the scatter
    means, heads = torch.randn(plan.N, 3, generator=g), torch.randn(plan.n, 10, generator=g)
    d_xyz, d_rot, d_scale = heads.split((3, 4, 3), dim=-1)
    idx = (sel.nonzero().squeeze(-1),)
    want = (means + torch.zeros_like(means).index_put(idx, d_xyz), torch.zeros(plan.N, 4).index_put(idx, d_rot),
            torch.zeros(plan.N, 3).index_put(idx, d_scale))  # fmt: skip
    for got, w in zip(R.scatter_torch(plan.sel_index64, means, d_xyz, d_rot, d_scale), want):
        assert torch.equal(got, w)
    # ... and through the rank array, as the kernel reads it
    r = plan.rank.long()
    picked = torch.where((r >= 0)[:, None], d_xyz[r.clamp(min=0)], torch.zeros(1, 3))
    assert torch.equal(means + picked, want[0])


@pytest.mark.parametrize("value,want", [(None, False), ("0", False), ("1", True)])
def test_knob_values(monkeypatch, value, want):
    if value is None:
        monkeypatch.delenv("FG_FUSED_CONTROL", raising=False)
    else:
        monkeypatch.setenv("FG_FUSED_CONTROL", value)
    assert deform.fused_control() is want


@pytest.mark.parametrize("value", ["2", "", "true", "01"])
def test_knob_typos_raise(monkeypatch, value):
    monkeypatch.setenv("FG_FUSED_CONTROL", value)
    with pytest.raises(ValueError, match="FG_FUSED_CONTROL"):
        deform.fused_control()
    with pytest.raises(ValueError, match="FG_FUSED_CONTROL"):
        model_mod.fused_control_applies(torch.zeros(4, 3), torch.ones(4, 3, dtype=torch.bool), None)


class _OnGpu:
    """A stand-in that says it lives on a GPU, for the conditions that are looked at before anything is computed."""

    def __init__(self, t):
        self.t = t
        self.is_cuda, self.device, self.dtype, self.shape = True, "cuda:0", t.dtype, t.shape

    def dim(self):
        return self.t.dim()


def test_fused_control_applies_conditions(monkeypatch):
    means, mask = torch.zeros(160, 3), G.control_mask("base")
    applies = model_mod.fused_control_applies
    monkeypatch.delenv("FG_FUSED_CONTROL", raising=False)
    assert applies(_OnGpu(means), _OnGpu(mask), None) is False  # the knob is unset
    monkeypatch.setenv("FG_FUSED_CONTROL", "1")
    assert applies(_OnGpu(means), _OnGpu(mask), None) is True  # (the stand-ins: everything in order)
    assert applies(_OnGpu(means), _OnGpu(mask), None, ops.control_plan(mask)) is True
    assert applies(means, mask, None) is False  # CPU tensors
    assert applies(means, _OnGpu(mask), None) is False and applies(_OnGpu(means), mask, None) is False
    assert applies(_OnGpu(means), _OnGpu(mask), torch.ones(160, dtype=torch.bool)) is False  # an active crop
    empty = mask.clone()
    empty[:, 2] = False
    assert applies(_OnGpu(means), _OnGpu(empty), None, ops.control_plan(empty)) is False  # an attribute without a row
    none = torch.zeros(160, 3, dtype=torch.bool)
    assert applies(_OnGpu(means), _OnGpu(none), None, ops.control_plan(none)) is False  # no row at all
    assert applies(_OnGpu(means), _OnGpu(torch.ones(160, 33, dtype=torch.bool)), None) is False  # M = 33
    assert applies(_OnGpu(means), _OnGpu(torch.ones(160, 32, dtype=torch.bool)), None) is True
    assert applies(_OnGpu(means.double()), _OnGpu(mask), None) is False  # not float32
    assert applies(_OnGpu(means), _OnGpu(mask.float()), None) is False  # not a bool mask
    assert applies(_OnGpu(means[:100]), _OnGpu(mask), None) is False  # rows that do not match
    assert _lib.CONTROL_MAX_ATTRS == 32


def _boom(*a, **k):
    raise AssertionError("an ops.control_* call on a CPU model")


def test_cpu_model_is_the_same_with_the_knob(monkeypatch):
    cm, cam = _control_model()
    for name in ("control_plan", "control_attr_mean", "control_value_rows", "control_scatter"):
        monkeypatch.setattr(ops, name, _boom)
    results = {}
    for knob in (None, "1"):
        if knob is None:
            monkeypatch.delenv("FG_FUSED_CONTROL", raising=False)
        else:
            monkeypatch.setenv("FG_FUSED_CONTROL", knob)
        cm.zero_grad()
        outs = cm._control_stage(cam)
        sum((o * (i + 1.0)).sum() for i, o in enumerate(outs)).backward()
        results[knob] = [o.detach().clone() for o in outs] + [p.grad.clone() for p in cm.parameters() if p.grad is not None]
    assert len(results[None]) > 5
    for a, b in zip(results[None], results["1"]):
        assert torch.equal(a, b)
    # ... and under a crop, in eval mode
    cm.eval()
    cm.set_crop(OrientedBox(torch.eye(3), torch.tensor([0.1, 0.0, 0.0]), torch.tensor([0.9, 1.0, 1.0])))
    crop = cm._crop_ids()
    assert 0 < int(crop.sum()) < cm.num_points
    object.__setattr__(cm, "_active_crop", crop)
    with torch.no_grad():
        outs = cm._control_stage(cam)
    assert outs[0].shape[0] == int(crop.sum())


def test_ops_refuse_cpu_tensors_and_wrong_shapes():
    mask = G.control_mask("base")
    plan = ops.control_plan(mask)
    rows = torch.zeros(plan.n, 3)
    with pytest.raises(_lib.FgRasterError, match="GPU only"):
        ops.control_attr_mean(plan, rows, rows.clone())
    with pytest.raises(_lib.FgRasterError, match="GPU only"):
        ops.control_value_rows(plan, torch.zeros(3, 3))
    with pytest.raises(_lib.FgRasterError, match="GPU only"):
        ops.control_scatter(plan, torch.zeros(160, 3), rows, torch.zeros(plan.n, 4), rows)
    with pytest.raises(ValueError):
        ops.control_attr_mean(plan, torch.zeros(plan.n + 1, 3), rows)
    with pytest.raises(ValueError):
        ops.control_value_rows(plan, torch.zeros(4, 3))
    with pytest.raises(ValueError):
        ops.control_scatter(plan, torch.zeros(159, 3), rows, torch.zeros(plan.n, 4), rows)


def test_entry_points_are_declared_found_by_name_and_validate():
    """The header declares the six entry points, found BY NAME with the ABI numbers unchanged; a few refusals through the
    binding (csrc/check/control_args.cpp, ``make control-check``, has the whole table under the host sanitizers)."""
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "fgraster.h")).read()
    names = ("fg_control_supported", "fg_control_workspace_bytes", "fg_control_attr_mean", "fg_control_value_rows",
             "fg_control_scatter_fwd", "fg_control_scatter_bwd")  # fmt: skip
    note = text[text.index("#define FG_ABI_MINOR") : text.index("#define FG_COUNT_OUT_WORDS")]
    for name in names:
        assert name in note and name in _lib.SIGNATURES, name
    assert re.search(r"^#define FG_ABI_VERSION 14$", text, flags=re.M) and re.search(r"^#define FG_ABI_MINOR 1 ", text, flags=re.M)
    assert (_lib.ABI_VERSION, _lib.ABI_MINOR) == (14, 1)
    lib = _lib.load()
    assert [lib.fg_control_supported(m) for m in (0, 1, 32, 33)] == [0, 1, 1, 0]
    assert lib.fg_control_workspace_bytes(0, 3) == 0 and lib.fg_control_workspace_bytes(1025, 3) == 2 * 9 * 8
    import ctypes

    p = 1 << 32
    counts = (ctypes.c_int32 * 3)(5, 0, 5)
    assert lib.fg_control_attr_mean(100, 3, p, 3, p + (1 << 26), 3, p + (2 << 26), ctypes.addressof(counts), p + (3 << 26), 1 << 20,
                                    p + (4 << 26), None) == -1  # an attribute without a row  # fmt: skip
    assert lib.fg_control_value_rows(-1, 3, p, p, p, None) == -1 and lib.fg_control_value_rows(0, 3, p, p, p, None) == 0
    assert lib.fg_control_scatter_fwd(10, 11, p, p, p, 3, p, 4, p, 3, p, p, p, None) == -1
    assert lib.fg_control_scatter_bwd(10, 20, p, None, None, None, None, 0, None, 0, None, 0, None) == 0  # nothing asked for
