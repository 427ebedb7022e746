"""The fused stage-2 control stage (csrc/control.hip through ``ops.control_*``; ``FG_FUSED_CONTROL=1``) on the GPU.

Kernels: the attribute means and the value rows against float64 of the same fp32 inputs, within the DERIVED bounds of
tests/control_restatement.py (nothing measured enters them); the scatter and its backward ``torch.equal`` with the torch
statement (``zeros_like().index_put`` and autograd).  Model: the reference's own stage-2 runs (tests/golden/g_control.npz)
with the knob set, through the checks of ``test_reference_goldens._run_stage2``; the knob against unset on the 2 000-Gaussian
scene of tests/test_se3_apply_gpu.py in training mode; and the second call of the control stage without one host
synchronisation."""
import contextlib
import copy
import functools

import pytest
import torch

import control_restatement as R
import helpers
import test_reference_goldens as TG
import test_se3_apply_gpu as S
from freegaussian_amd import _lib, model as model_mod, ops
from parity_common import need_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _plan_of(pmask):
    """A plan whose every row is selected (n = N): what the two reductions see of a mask."""
    plan = ops.control_plan(pmask.to(DEV))
    assert plan.n == pmask.shape[0]
    return plan


# ---------------------------------------------------------------------------------------------------------------------
# attribute means


@functools.lru_cache(maxsize=None)
def _mean_reference(n, M):
    a, b, pmask = R.mean_case(n, M)
    x64, A64 = R.attr_mean64(a, b, pmask)
    return a, b, pmask, x64, A64


@pytest.mark.parametrize("layout", ["contiguous", "columns"])
@pytest.mark.parametrize("M", R.MEAN_ATTRS)
@pytest.mark.parametrize("n", R.MEAN_ROWS)
def test_attribute_means_within_the_derived_bound(n, M, layout):
    a, b, pmask, x64, A64 = _mean_reference(n, M)
    counts = pmask.sum(0)
    assert int(counts[0]) == n and (M == 1 or int(counts[-1]) == 1) and int(counts.min()) >= 1
    plan = _plan_of(pmask)
    if layout == "columns":  # a and b as columns 1..3 and 5..7 of one [n,9] block
        block = torch.full((n, 9), float("nan"))
        block[:, 1:4], block[:, 5:8] = a, b
        block = block.to(DEV)
        ga, gb = block[:, 1:4], block[:, 5:8]
        assert n == 1 or (ga.stride() == (9, 1) and gb.data_ptr() == ga.data_ptr() + 16)
    else:
        ga, gb = a.to(DEV), b.to(DEV)
    first = ops.control_attr_mean(plan, ga, gb)
    second = ops.control_attr_mean(plan, ga, gb)
    torch.cuda.synchronize()
    assert first.shape == (M, 3) and first.dtype == torch.float32
    assert torch.equal(first, second)  # no atomics: a second run gives the same bits
    err, bound = (first.cpu().double() - x64).abs(), R.attr_mean_bound(x64, A64, n)
    worst = float((err / bound.clamp(min=1e-300)).max())
    helpers._record("attr_mean|error over bound", worst, 1)
    print(f"n {n} M {M} {layout}: worst error / bound {worst:.3g}")
    assert bool((err <= bound).all()), (n, M, worst)


def test_attribute_mean_layouts_give_the_same_bits_and_an_empty_attribute_raises():
    a, b, pmask, _, _ = _mean_reference(4097, 3)
    plan = _plan_of(pmask)
    block = torch.zeros(4097, 9)
    block[:, 1:4], block[:, 5:8] = a, b
    block = block.to(DEV)
    assert torch.equal(ops.control_attr_mean(plan, a.to(DEV), b.to(DEV)), ops.control_attr_mean(plan, block[:, 1:4], block[:, 5:8]))
    # bits at or above M are ignored: the same rows under a plan whose words carry more
    wide = torch.cat([pmask, torch.ones(4097, 2, dtype=torch.bool)], dim=1)
    wide_plan = _plan_of(wide)
    wide_plan.M, wide_plan.counts_host = 3, wide_plan.counts_host[:3]
    import ctypes

    wide_plan._counts_c = (ctypes.c_int32 * 3)(*wide_plan.counts_host)
    assert torch.equal(ops.control_attr_mean(wide_plan, a.to(DEV), b.to(DEV)), ops.control_attr_mean(plan, a.to(DEV), b.to(DEV)))
    empty = pmask.clone()
    empty[:, 2] = False
    with pytest.raises(ValueError, match="attribute 2"):
        ops.control_attr_mean(_plan_of(empty), a.to(DEV), b.to(DEV))


# ---------------------------------------------------------------------------------------------------------------------
# value rows


@pytest.mark.parametrize("M", R.MEAN_ATTRS)
@pytest.mark.parametrize("n", R.MEAN_ROWS)
def test_value_rows_within_the_derived_bound(n, M):
    _, _, pmask, x64, _ = _mean_reference(n, M)
    d_avg = (x64 * 3.0 + 0.01).float()  # (any [M,3]: the means themselves, moved off zero)
    v64, s_over_p = R.value_rows64(pmask, d_avg)
    plan = _plan_of(pmask)
    value = ops.control_value_rows(plan, d_avg.to(DEV))
    torch.cuda.synchronize()
    assert value.shape == (n, 3) and value.dtype == torch.float32
    err, bound = (value.cpu().double() - v64).abs(), R.value_rows_bound(pmask, s_over_p)
    worst = float((err / bound.clamp(min=1e-300)).max())
    helpers._record("value_rows|error over bound", worst, 1)
    print(f"n {n} M {M}: worst error / bound {worst:.3g}")
    assert bool((err <= bound).all()), (n, M, worst)
    assert torch.equal(value.cpu(), R.value_rows32(pmask, d_avg))  # the kernel's order, restated: the same bits


# ---------------------------------------------------------------------------------------------------------------------
# scatter forward and backward


def _heads(heads, layout):
    """The three heads on the GPU: columns 0..2, 3..6, 7..9 of the [n,10] block in place, or three contiguous tensors."""
    if layout == "block":
        block = heads.to(DEV).requires_grad_(True)
        return block, block.split((3, 4, 3), dim=-1)
    leaves = [h.contiguous().to(DEV).requires_grad_(True) for h in heads.split((3, 4, 3), dim=-1)]
    return leaves, leaves


def _head_grads(leaf, layout):
    if layout == "block":
        return None if leaf.grad is None else leaf.grad.split((3, 4, 3), dim=-1)
    return [h.grad for h in leaf]


@functools.lru_cache(maxsize=None)
def _scatter_torch(N, sparse):
    """The torch statement on the GPU, forward and autograd: (outputs, gradients of means and of the three heads)."""
    mask, means, heads, ups = R.scatter_case(N, sparse)
    means = means.to(DEV).requires_grad_(True)
    leaves, hs = _heads(heads, "contiguous")
    outs = R.scatter_torch(mask.any(-1).nonzero().squeeze(-1).to(DEV), means, *hs)
    torch.autograd.backward(outs, [u.to(DEV) for u in ups])
    return [o.detach() for o in outs], [means.grad] + [h.grad for h in leaves]


def _scatter_fused(N, sparse, layout, want=(True, True, True, True), ups_present=(True, True, True)):
    mask, means, heads, ups = R.scatter_case(N, sparse)
    plan = ops.control_plan(mask.to(DEV))
    means = means.to(DEV).requires_grad_(want[0])
    if layout == "block":
        leaf, hs = _heads(heads, layout)
    elif layout == "columns":  # columns of the [n,10] block read in place, each a leaf of its own: any set of them may want
        block = heads.to(DEV)
        leaf = [h.detach().requires_grad_(w) for h, w in zip(block.split((3, 4, 3), dim=-1), want[1:])]
        assert plan.n == 1 or all(h.stride() == (10, 1) for h in leaf)
        hs = leaf
    else:
        leaf = [h.contiguous().to(DEV).requires_grad_(w) for h, w in zip(heads.split((3, 4, 3), dim=-1), want[1:])]
        hs = leaf
    outs = ops.control_scatter(plan, means, *hs)
    picked = [(o, u.to(DEV)) for o, u, p in zip(outs, ups, ups_present) if p]
    if any(want) and picked:
        torch.autograd.backward([o for o, _ in picked], [u for _, u in picked])
    torch.cuda.synchronize()
    return plan, [o.detach() for o in outs], means.grad, _head_grads(leaf, layout)


@pytest.mark.parametrize("layout", ["block", "contiguous"])
@pytest.mark.parametrize("sparse", [False, True], ids=["all-rows", "sparse"])
@pytest.mark.parametrize("N", R.SCATTER_ROWS)
def test_scatter_equals_the_torch_statement(N, sparse, layout):
    want_outs, want_grads = _scatter_torch(N, sparse)
    plan, outs, g_means, g_heads = _scatter_fused(N, sparse, layout)
    assert plan.n == (N if not sparse else int(R.scatter_mask(N, True).any(-1).sum()))
    for got, want in zip(outs, want_outs):
        assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(g_means, want_grads[0])
    for got, want in zip(g_heads, want_grads[1:]):
        assert got.shape == want.shape and torch.equal(got, want)


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["means", "d_xyz", "d_rot", "d_scale"])
@pytest.mark.parametrize("layout", ["contiguous", "columns"])
def test_each_gradient_alone_gives_the_bits_of_the_joint_call(which, layout):
    _, want_grads = _scatter_torch(257, True)
    want = tuple(i == which for i in range(4))
    _, _, g_means, g_heads = _scatter_fused(257, True, layout, want=want)
    got = [g_means] + list(g_heads)
    for i in range(4):
        assert (got[i] is None) == (i != which), i
    assert torch.equal(got[which], want_grads[which])


def test_the_gradient_of_means_is_the_upstream_tensor_itself():
    mask, means, heads, ups = R.scatter_case(257, True)
    plan = ops.control_plan(mask.to(DEV))
    means = means.to(DEV).requires_grad_(True)
    out = ops.control_scatter(plan, means, *(h.contiguous() for h in heads.to(DEV).split((3, 4, 3), dim=-1)))[0]
    up = ups[0].to(DEV)
    (g,) = torch.autograd.grad(out, means, up)
    assert g.data_ptr() == up.data_ptr()


@pytest.mark.parametrize("present", [(True, False, False), (False, True, True), (False, False, True)])
@pytest.mark.parametrize("layout", ["contiguous", "columns"])
def test_an_absent_upstream_gradient_counts_as_zeros(present, layout):
    _, want_grads = _scatter_torch(257, True)
    _, _, g_means, g_heads = _scatter_fused(257, True, layout, ups_present=present)
    assert (g_means is None) == (not present[0])
    for got, want, p in zip(g_heads, want_grads[1:], present):
        assert got.shape == want.shape
        assert torch.equal(got, want) if p else not bool(got.any())


def test_strided_gradient_outputs_through_the_c_abi():
    """g_d_xyz, g_d_rot, g_d_scale written as columns 1..3, 4..7, 9..11 of one [n,13] block: the bits of the joint call, the
    other columns untouched; and with g_d_rot alone, the rest of the block untouched."""
    mask, _, _, ups = R.scatter_case(257, True)
    _, want_grads = _scatter_torch(257, True)
    plan = ops.control_plan(mask.to(DEV))
    ups = [u.to(DEV) for u in ups]
    stream = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    block = torch.full((plan.n, 13), 7.0, device=DEV)
    base = block.data_ptr()
    rc = lib.fg_control_scatter_bwd(plan.n, plan.N, plan.sel_index.data_ptr(), ups[0].data_ptr(), ups[1].data_ptr(), ups[2].data_ptr(),
                                    base + 4, 13, base + 16, 13, base + 36, 13, stream)  # fmt: skip
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(block[:, 1:4], want_grads[1]) and torch.equal(block[:, 4:8], want_grads[2]) and torch.equal(block[:, 9:12], want_grads[3])
    assert bool((block[:, [0, 8, 12]] == 7.0).all())
    block.fill_(7.0)
    rc = lib.fg_control_scatter_bwd(plan.n, plan.N, plan.sel_index.data_ptr(), None, ups[1].data_ptr(), None, None, 0, base + 16, 13, None,
                                    0, stream)  # fmt: skip
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(block[:, 4:8], want_grads[2]) and bool((block[:, :4] == 7.0).all()) and bool((block[:, 8:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# against the reference's own stage-2 runs


@contextlib.contextmanager
def _spies(monkeypatch):
    calls = {"attr_mean": 0, "value_rows": 0, "scatter": 0}

    def spy(name):
        real = getattr(ops, f"control_{name}")

        def wrapped(*a, **k):
            calls[name] += 1
            return real(*a, **k)

        monkeypatch.setattr(ops, f"control_{name}", wrapped)

    for name in calls:
        spy(name)
    yield calls


@pytest.mark.parametrize("case", TG.G.CONTROL_CASES, ids=[c[0] for c in TG.G.CONTROL_CASES])
def test_stage2_get_outputs_with_the_knob_matches_reference_run(case, monkeypatch):
    """``_run_stage2``'s checks -- outputs by ``close_except_knife_edge``, equal radii, every gradient at REL_TOL -- with
    ``FG_FUSED_CONTROL=1``.  The four cases without a crop go through the fused calls (the mean only where there is a
    cameras0); the cropped one does not, and passes as it does unset."""
    tag, _, cam0, _, crop = case
    monkeypatch.setenv("FG_FUSED_CONTROL", "1")
    with _spies(monkeypatch) as calls:
        TG._run_stage2(case, "cuda", fused=True)
    if crop is None:
        assert calls == {"attr_mean": 1 if cam0 else 0, "value_rows": 1, "scatter": 1}, (tag, calls)
    else:
        assert calls == {"attr_mean": 0, "value_rows": 0, "scatter": 0}, (tag, calls)


# ---------------------------------------------------------------------------------------------------------------------
# model pair: the knob against unset


def _control_model():
    """The scene and the masks of test_se3_apply_gpu.test_control_model_displacement_fused_against_unset, in training mode."""
    from freegaussian_amd.model import FreeGaussianControlModel, FreeGaussianModelConfig

    base, cam = S._model_and_camera()
    mask = torch.zeros(2000, 3, dtype=torch.bool)
    mask[:60, 0] = True
    mask[40:100, 1] = True
    mask[200:230, 2] = True
    init_cam = type(cam)(cam.camera_to_worlds, cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, times=torch.tensor([[0.0]]))
    cm = FreeGaussianControlModel(mask, init_cam, config=FreeGaussianModelConfig(background_color="black"),
                                  seed_points=base.means.detach().clone())  # fmt: skip
    cm.load_state_dict(base.state_dict(), strict=False)
    cam.metadata["cameras0"] = init_cam
    return cm.train(), cam


def _boom(*a, **k):
    raise AssertionError("an ops.control_* call with FG_FUSED_CONTROL unset")


def _step(cm, cam):
    cm.zero_grad(set_to_none=True)
    out = cm.get_outputs(cam)
    ((out["rgb"] - 0.4).square().mean()).backward()
    torch.cuda.synchronize()
    return out["rgb"].detach().cpu(), {k: p.grad.detach().cpu() for k, p in cm.named_parameters() if p.grad is not None}


def _compare(tag, fused, unset):
    (rgb1, g1), (rgb0, g0) = fused, unset
    assert float(rgb0.max()) > 0.05
    assert set(g0) == set(g1) and "gauss_params.means" in g0 and any(k.startswith("control.d_xyz") for k in g0)
    worst = {"rgb": S._bar(rgb1, rgb0)}
    for k in g0:
        if float(g0[k].abs().max()) > 0:
            worst[k] = S._bar(g1[k], g0[k])
        else:
            assert not bool(g1[k].any()), k
    for k, v in worst.items():
        helpers._record(f"control_model_bar|{tag}|{k}", v, 2)
    print(tag, {k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) <= helpers.REL_TOL, (tag, worst)


def test_control_model_step_fused_against_unset_and_a_mask_edit_is_followed(monkeypatch):
    base, cam = _control_model()

    def edit(cm):  # in place: thirty more rows in attribute 2, ten fewer in attribute 0
        cm.gaussian_mask[300:330, 2] = True
        cm.gaussian_mask[:10, 0] = False

    # unset: the torch ops, with the fused calls replaced by something that raises
    monkeypatch.delenv("FG_FUSED_CONTROL", raising=False)
    for name in ("control_plan", "control_attr_mean", "control_value_rows", "control_scatter"):
        monkeypatch.setattr(ops, name, _boom)
    plain = copy.deepcopy(base).to(DEV)
    unset_before = _step(plain, cam)
    edit(plain)
    unset_after = _step(plain, cam)
    monkeypatch.undo()
    # the knob
    monkeypatch.setenv("FG_FUSED_CONTROL", "1")
    fused = copy.deepcopy(base).to(DEV)
    with _spies(monkeypatch) as calls:
        fused_before = _step(fused, cam)
        plan_before = fused._control_plan()
        edit(fused)
        fused_after = _step(fused, cam)
    assert calls == {"attr_mean": 2, "value_rows": 2, "scatter": 2}
    assert fused._control_plan() is not plan_before and fused._control_plan().n == plan_before.n + 20
    _compare("before the edit", fused_before, unset_before)
    _compare("after the edit", fused_after, unset_after)
    assert S._bar(unset_after[0], unset_before[0]) > 10 * helpers.REL_TOL  # (the edit shows in the image: following it is visible)


def test_fused_control_applies_on_the_gpu(monkeypatch):
    cm, _ = _control_model()
    cm = cm.to(DEV)
    means, mask = cm.gauss_params["means"], cm.gaussian_mask
    monkeypatch.setenv("FG_FUSED_CONTROL", "1")
    assert model_mod.fused_control_applies(means, mask, None, cm._control_plan())
    assert not model_mod.fused_control_applies(means, mask, torch.ones(2000, dtype=torch.bool, device=DEV))
    assert not model_mod.fused_control_applies(means.cpu(), mask.cpu(), None)
    empty = mask.clone()
    empty[:, 1] = False
    assert not model_mod.fused_control_applies(means, empty, None, ops.control_plan(empty))
    monkeypatch.setenv("FG_FUSED_CONTROL", "0")
    assert not model_mod.fused_control_applies(means, mask, None)
    # an empty attribute keeps the torch ops, NaN and all
    monkeypatch.setenv("FG_FUSED_CONTROL", "1")
    cm.gaussian_mask[:, 1] = False
    with _spies(monkeypatch) as calls, torch.no_grad():
        moved = cm._control_stage(_control_model()[1])[0]
    assert calls == {"attr_mean": 0, "value_rows": 0, "scatter": 0} and bool(torch.isnan(moved).any())


# ---------------------------------------------------------------------------------------------------------------------
# no host synchronisation


def _resident(cm, cam):
    """The model on the GPU with both cameras' times there too: a time on the host is uploaded by a blocking copy, as in
    stage 1, which the debug mode counts."""
    cm = cm.to(DEV)
    cam.times = cam.times.to(DEV)
    cm.init_camera.times = cm.init_camera.times.to(DEV)
    return cm, cam


def _stage_forward_backward(cm, cam):
    cm.zero_grad(set_to_none=True)
    means, d_rotation, d_scaling = cm._control_stage(cam)
    (means.sum() + 2.0 * d_rotation.sum() + 3.0 * d_scaling.sum()).backward()


def test_second_call_of_the_control_stage_does_not_synchronise(monkeypatch):
    monkeypatch.setenv("FG_FUSED_CONTROL", "1")
    cm, cam = _resident(*_control_model())
    with _spies(monkeypatch) as calls:
        _stage_forward_backward(cm, cam)  # the first call builds the plan: read-backs are allowed there, and only there
        torch.cuda.synchronize()
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            inert = False
            try:  # the canary: a read-back under the same mode must raise
                torch.ones(4, device=DEV).nonzero()
                inert = True
            except RuntimeError:
                pass
            assert not inert, "torch.cuda.set_sync_debug_mode('error') is inert on this build: nonzero() did not raise"
            _stage_forward_backward(cm, cam)
        finally:
            torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert calls == {"attr_mean": 2, "value_rows": 2, "scatter": 2}
    assert cm.gauss_params["means"].grad is not None and cm.control.d_xyz.weight.grad is not None
    # the torch ops do synchronise: the mode is not blind to this stage
    monkeypatch.setenv("FG_FUSED_CONTROL", "0")
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            _stage_forward_backward(cm, cam)
    finally:
        torch.cuda.set_sync_debug_mode(before)


def test_second_call_of_the_control_stage_reads_nothing_back(monkeypatch):
    """The same region under a spy on the calls that read back: ``Tensor.nonzero``, ``item``, ``tolist`` and indexing with a
    bool tensor.  (The torch ops make M + 3 of them.)"""
    reads = []

    def count(name):
        real = getattr(torch.Tensor, name)

        def wrapped(self, *a, **k):
            if self.is_cuda and (name != "__getitem__" or any(isinstance(i, torch.Tensor) and i.dtype == torch.bool
                                                               for i in (a[0] if isinstance(a[0], tuple) else (a[0],)))):  # fmt: skip
                reads.append(name)
            return real(self, *a, **k)

        monkeypatch.setattr(torch.Tensor, name, wrapped)

    cm, cam = _resident(*_control_model())
    monkeypatch.setenv("FG_FUSED_CONTROL", "1")
    _stage_forward_backward(cm, cam)
    for name in ("nonzero", "item", "tolist", "__getitem__"):
        count(name)
    _stage_forward_backward(cm, cam)
    assert reads == [], reads
    monkeypatch.setenv("FG_FUSED_CONTROL", "0")
    _stage_forward_backward(cm, cam)
    assert reads.count("nonzero") == 1 and reads.count("__getitem__") == 2 + cm.gaussian_mask.shape[1], reads
