"""GPU: what every stage of a training step gives when it is run AGAIN on the same bits (tests/step_repeat_common.py: the
step of ``tests/test_mlp_chunked_gpu.py::test_model_training_step_with_the_knob_set_and_unset`` cut at its stage boundaries).
Each stage runs 8 times in one process on recorded inputs and is held to one of two contracts.

BIT-REPEATABLE: every output ``torch.equal`` across the 8 runs.  Holds for a stage whose kernels have no float atomic;
read for that (``atomic``, every spelling): csrc/mlp.hip, mlp_wgrad.hip, preprocess.hip, sh.hip, loss.hip -- none at all;
csrc/stbin.hip, radix_sort.h, jobs_build.h, binning.hip, sort.hip -- integer atomics only (counts and cursors; the lists are
sorted by (tile, depth, id), so no arrival order can show); the raster FORWARD (csrc/raster.hip ``raster_fwd_body``) -- an
integer ``atomicAdd`` / ``atomicOr`` on the heavy tiles' open list and liveness words, a pixel's sum is one lane's.

    mlp_forward, mlp_backward (``FG_FUSED_MLP_CHUNKED`` set and unset, parameter gradients fp32 and bf16x3),
    transform_forward / _backward (torch), per_gaussian_forward / _backward (``ops.preprocess_raw``; and ``ops.preprocess`` on
    the same tensors), binning, raster_forward, loss (+ its backward)

ORDER-BOUNDED: the raster backward, the one stage with float atomics (csrc/raster.hip ``raster_bwd_body``, three
``__hip_atomic_fetch_add`` sites, one taken per build).  ``k`` = the addends a splat's record gradient receives on the launch
taken (step_repeat_common, "THE COUNT": where each factor was read).  Rows with k <= 2 are bit-equal across the runs; a slot
of a row with k >= 3 spreads by at most ``2 (k - 1) 2^-24 A``, A its absolute accumulation in the float64 restatement
(tests/raster_restatement.py): the reordering bound of a k-term fp32 sum.  On three small scenes with every class
populated (tests/test_step_repeat_host.py), on the classic launch (one and two tiles), on job lists with list shares and
with pixel strips; and on the step's own records, at the flaky test's log-scales and at the repaired test's.

THE CHAIN: the whole step 8 times with every stage fed the first run's records, and 8 times with a run's own outputs
flowing: the first stage whose outputs differ is named.

Measured (MI355X): profiles/step_repeatability.md."""
import functools

import pytest
import torch

import raster_restatement as R
import step_repeat_common as C
from freegaussian_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
BIT_STAGES = ("mlp_forward", "transform_forward", "per_gaussian_forward", "binning", "raster_forward", "loss",
              "per_gaussian_backward", "transform_backward")  # fmt: skip


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (no CPU fallback exists)")
    _lib.load()


@functools.lru_cache(maxsize=None)
def _recorded(which):
    """(Step, the records of one run, that run's outputs by stage) -- made once, never changed."""
    with C.knobs():
        step = C.Step(DEV, C.OLD_SCALE_MEAN if which == "old" else C.SCALE_MEAN)
        rec, outs = step.record()
    return step, rec, outs


@functools.lru_cache(maxsize=None)
def _step_count(which):
    """(k [N], bound [N,16]) of the step's raster backward, from its own records and the forward's own last_ids."""
    step, rec, _ = _recorded(which)
    assert int(_lib.load().fg_raster_jobs_words(step.W, step.H, C.TILE, ops.current().cfg())) == 0  # the classic launch
    rc = rec["splats"].cpu()
    gid, tile, hits = C.strip_hits(rc[:, 0:2], rc[:, 3:6], rc[:, 2], rec["offsets"], rec["flatten_ids"], rec["last_ids"], step.W, step.H)
    k = C.addend_count(step.n, gid, tile, hits, C.groups_classic(1))
    # A: the float64 restatement on the records, with the cotangents the kernel forms from v_render (a clamped channel
    # -- the finished image is exactly 0 or 1 there -- passes nothing; d/dalpha of (1 - alpha) * background)
    colours = torch.zeros(step.n, 8)
    colours[:, :3] = rc[:, 6:9]
    sc = R.RegimeScene(rc[:, 0:2].contiguous(), rc[:, 3:6].contiguous(), rc[:, 2].contiguous(), rec["depths"].cpu(), rec["radii"].cpu(),
                       colours, ["step"] * step.n, rec["offsets"].cpu(), rec["flatten_ids"].cpu(), step.W, step.H)  # fmt: skip
    render = rec["render"].cpu().double().reshape(step.H, step.W, 3)
    vr = rec["v_render"].cpu().double().reshape(step.H, step.W, 3) * ((render > 0) & (render < 1))
    va = -(vr * step.background.cpu().double()).sum(-1)
    _, accum = R.backward(sc, 3, vr, va, rec["alphas"].cpu().double().reshape(step.H, step.W), torch.float64)
    return k, C.order_bound(k, C.accum_slots(accum))


def _fail(failures):
    assert not failures, "\n".join(failures)


# ---- 1. the cut is the step --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["old", "new"])
def test_the_stages_chained_are_the_models_step(which):
    """The loss and every gradient of ``model.get_outputs`` + ``loss.backward()`` against the chain's: bit for bit where no
    row has three addends; else bit for bit on the loss, and every gradient within 1e-5 of its largest element."""
    step, rec, _ = _recorded(which)
    k, _ = _step_count(which)
    with C.knobs():
        loss, grads = C.model_step(step.model, step.cam, step.gt)
    step.model.zero_grad(set_to_none=True)
    mine = step.final_gradients(rec)
    assert torch.equal(loss, rec["loss"]) and set(mine) == set(grads) and len(grads) == 34
    for name, g in grads.items():
        a = mine[name].reshape(g.shape)
        if int(k.max()) <= 2:
            assert torch.equal(a, g), name
        else:
            assert float((a - g).abs().max()) <= 1e-5 * float(g.abs().max()), name
        assert float(g.abs().max()) > 0, name


# ---- 2. bit-repeatable stages ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", BIT_STAGES)
@pytest.mark.parametrize("which", ["old", "new"])
def test_stage_is_bit_repeatable(which, stage):
    step, rec, outs = _recorded(which)
    with C.knobs():
        runs = [outs[stage]] + [getattr(step, stage)(rec) for _ in range(C.REPEATS)]
    torch.cuda.synchronize()
    assert all(v is not None and v.numel() > 0 for v in runs[0].values())
    _fail(C.bit_failures(f"{which} {stage}", runs))


@pytest.mark.parametrize("wgrad", [None, "bf16x3"])
@pytest.mark.parametrize("which", ["old", "new"])
def test_mlp_backward_is_bit_repeatable_with_the_knob_set_and_unset(which, wgrad):
    """8 runs with ``FG_FUSED_MLP_CHUNKED=1`` and 8 without, on the same cotangents: 28 parameter gradients and the input-row
    gradient, all 16 runs equal bit for bit (the chunked backward IS the two calls: tests/test_mlp_chunked_gpu.py)."""
    step, rec, outs = _recorded(which)
    runs = []
    for chunked in (True, False):
        with C.knobs(chunked=chunked, wgrad_precision=wgrad):
            runs += [step.mlp_backward(rec) for _ in range(C.REPEATS)]
    torch.cuda.synchronize()
    assert len(runs[0]) == 29 and all(float(v.abs().max()) > 0 for v in runs[0].values())
    if wgrad is None:
        runs = [outs["mlp_backward"]] + runs
    _fail(C.bit_failures(f"{which} mlp_backward wgrad={wgrad}", runs))


def _activated_pass(step, rec):
    """``ops.preprocess`` as ``rasterization()`` calls it (activated parameters, ``overlap=True``), forward and
    backward on the step's recorded tensors: the other per-Gaussian pass (``fg_preprocess_fwd / _bwd``)."""
    p = step.model.gauss_params
    with torch.no_grad():
        ins = [rec["means_d"], p["quats"] / p["quats"].norm(dim=-1, keepdim=True) + rec["d_rotation"],
               torch.exp(p["scales"]) + rec["d_scaling"], torch.sigmoid(p["opacities"]).squeeze(-1),
               torch.cat((p["features_dc"][:, None, :], p["features_rest"]), dim=1)]  # fmt: skip
    ins = [t.detach().clone().requires_grad_(True) for t in ins]
    radii, means2d, depths, conics, tiles, splats = ops.preprocess(*ins, None, step.viewmat[0], step.K[0], step.W, step.H, 0.3, 0.01,
                                                                   1e10, 0.0, C.TILE, False, step.sh_degree, False, overlap=True)  # fmt: skip
    ops._wait_ready(splats)
    v = rec["v_splats"]
    grads = torch.autograd.grad((means2d, splats), ins, (v[:, 0:2], v))
    out = dict(radii=radii, means2d=means2d, depths=depths, conics=conics, tiles=tiles, splats=splats)
    out.update({f"v_{n}": g for n, g in zip(("means", "quats", "scales", "opacities", "colors"), grads)})
    torch.cuda.synchronize()
    return {k: t.detach().clone() for k, t in out.items()}


@pytest.mark.parametrize("which", ["old", "new"])
def test_the_activated_per_gaussian_pass_is_bit_repeatable(which):
    step, rec, _ = _recorded(which)
    runs = [_activated_pass(step, rec) for _ in range(C.REPEATS)]
    assert all(float(runs[0][k].abs().max()) > 0 for k in runs[0])
    _fail(C.bit_failures(f"{which} ops.preprocess", runs))


# ---- 3. the raster backward: order-bounded -----------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["old", "new"])
def test_step_raster_backward_is_order_bounded(which):
    """The step's own raster backward.  Prints the distribution of k at the flaky test's shape: the old docstring's premise
    ("ONE 16 x 16 tile gives every splat one job", so at most two addends) holds if and only if no row has k >= 3."""
    step, rec, outs = _recorded(which)
    k, bound = _step_count(which)
    print(f"step scene ({which}: log-scale mean {C.OLD_SCALE_MEAN if which == 'old' else C.SCALE_MEAN}), classic launch, 4 wavefronts "
          f"per tile: k census {C.census(k)}, histogram {torch.bincount(k).tolist()}, rows with k >= 3: {(k >= 3).nonzero().flatten().tolist()[:16]}")  # fmt: skip
    with C.knobs():
        runs = [outs["raster_backward"]["v_splats"]] + [step.raster_backward(rec)["v_splats"] for _ in range(C.REPEATS)]
    torch.cuda.synchronize()
    distinct = len({r.cpu().numpy().tobytes() for r in runs})
    print(f"step scene ({which}): {distinct} distinct outcome(s) of the raster backward in {len(runs)} runs")
    c = C.census(k)
    assert c["1"] > 0 and c["2"] > 0
    if which == "new":
        assert c[">=3"] == 0 and distinct == 1
    _fail(C.order_failures(f"{which} step raster_backward", runs, k, bound))


def _raster_runs(name, strips):
    """The small scene ``name`` through ``ops.rasterize_splats`` 8 times, forward and backward.
    -> (forward outputs per run, [N,16] record gradients per run, k, bound)"""
    sc = C.raster_scene(name)
    nt, n = C.n_tiles_of(sc), sc.means2d.shape[0]
    ctx = ops.RasterContext()
    if strips:
        ctx.seg_ckpt_budget_bytes = 0  # no checkpoints: the backward's jobs are pixel strips
    rec, offs, ids = C.pack_records(sc).to(DEV), sc.offsets.to(DEV), sc.flatten_ids.to(DEV)
    vr = C.raster_cotangent(sc).float().to(DEV)
    fwds, grads, groups = [], [], None
    with ops.use(ctx):
        words = int(_lib.load().fg_raster_jobs_words(sc.width, sc.height, C.TILE, ctx.cfg()))
        assert (words > 0) == (C.RASTER_SCENES[name][4] == "jobs")
        for _ in range(C.REPEATS):
            splats, m2 = rec.clone().requires_grad_(True), rec[:, 0:2].clone().unsqueeze(0).requires_grad_(True)
            render, alphas, last = ops.rasterize_splats(splats, m2, 3, sc.width, sc.height, C.TILE, offs, ids, absgrad=True)
            node = render.grad_fn
            if groups is None:
                if words == 0:
                    assert node.jobs_bwd is None
                    groups = C.groups_classic(nt)
                else:
                    shares = node.saved_tensors[7] is not None  # (the forward's checkpoints: list shares in the backward)
                    assert shares == (not strips)
                    groups = C.groups_from_jobs(node.jobs_bwd, nt, shares, sc.offsets)
            fwds.append(dict(render=render.detach().clone(), alphas=alphas.detach().clone(), last_ids=last.clone()))
            (g,) = torch.autograd.grad(render, splats, vr)
            grads.append(g.clone())
    torch.cuda.synchronize()
    k = C.scene_addends(sc, groups, fwds[0]["last_ids"].cpu())
    f64 = R.composite(sc, 3, torch.float64)
    _, accum = R.backward(sc, 3, C.raster_cotangent(sc), torch.zeros(sc.height, sc.width, dtype=torch.float64), f64["alpha"], torch.float64)
    return fwds, grads, k, C.order_bound(k, C.accum_slots(accum)), groups


@pytest.mark.parametrize("name,strips", [("one_tile", False), ("two_tiles", False), ("job_lists", False), ("job_lists", True)])
def test_raster_stage_alone(name, strips):
    """Forward: bit-repeatable on the launch taken.  Backward: order-bounded, with every class of k populated."""
    fwds, grads, k, bound, groups = _raster_runs(name, strips)
    c = C.census(k)
    waves = sorted({tuple(g for g in row if g) for row in groups.tolist()})
    print(f"{name} ({'pixel strips' if strips else C.RASTER_SCENES[name][4]}): wavefront strip sets per tile {waves[:6]}, k census {c}, "
          f"{len({g.cpu().numpy().tobytes() for g in grads})} distinct backward outcomes in {len(grads)} runs")  # fmt: skip
    assert min(c["1"], c["2"], c[">=3"]) >= 20, c
    assert float(grads[0].abs().max()) > 0 and bool((grads[0][k == 0] == 0).all())
    _fail(C.bit_failures(f"{name} forward", fwds) + C.order_failures(f"{name} backward", grads, k, bound))


def test_job_lists_start_where_the_small_scene_is():
    """320 x 160 = 200 tiles is the smallest image with job lists: one tile row or column less has none."""
    words = lambda w, h: int(_lib.load().fg_raster_jobs_words(w, h, C.TILE, ops.current().cfg()))  # noqa: E731
    assert words(320, 160) > 0 and words(304, 160) == 0 and words(320, 144) == 0 and words(16 * 199, 16) == 0 and words(16, 16) == 0


# ---- 4. the chain ------------------------------------------------------------------------------------------------------
def _first_split(step, chains, reference):
    """(first stage whose outputs differ from ``reference`` in some chain, {stage: {tensor: most elements differing}})."""
    report = {}
    for outs in chains:
        for stage in step.STAGES:
            for name, cnt in C.differing(reference[stage], outs[stage]).items():
                report.setdefault(stage, {})[name] = max(cnt, report.get(stage, {}).get(name, 0))
    first = next((s for s in step.STAGES if s in report), None)
    return first, report


@pytest.mark.parametrize("which", ["old", "new"])
def test_chain_on_recorded_inputs_names_the_stage_that_splits(which):
    """Every stage 8 times on the FIRST run's records.  Only the raster backward may differ, only where k >= 3 allows it,
    and the stages behind it -- fed the recorded ``v_splats`` -- may not."""
    step, rec, outs = _recorded(which)
    k, bound = _step_count(which)
    with C.knobs():
        chains = [step.chain(rec) for _ in range(C.REPEATS)]
    first, report = _first_split(step, chains, outs)
    print(f"chain on recorded inputs ({which}): first stage that splits: {first}; differing elements {report}")
    assert first in (None, "raster_backward") and set(report) <= {"raster_backward"}, report
    if int(k.max()) <= 2:
        assert first is None
    _fail(C.order_failures(f"{which} chain raster_backward", [outs["raster_backward"]["v_splats"]] + [c["raster_backward"]["v_splats"] for c in chains], k, bound))  # fmt: skip


@pytest.mark.parametrize("which", ["old", "new"])
def test_chain_with_its_own_outputs_flowing(which):
    """The step 8 times from its inputs.  Everything in front of the raster backward repeats; with no row of k >= 3 so does
    everything behind it, to the last parameter gradient; with such rows the first difference is the raster backward's
    and the number of distinct outcomes is printed."""
    step, rec, outs = _recorded(which)
    k, _ = _step_count(which)
    with C.knobs():
        chains = [step.chain() for _ in range(C.REPEATS)]
    first, report = _first_split(step, chains, outs)
    finals = {tuple(sorted((n, t.cpu().numpy().tobytes()) for n, t in step.final_gradients(step.flat(c)).items())) for c in chains + [outs]}
    print(f"chain flowing ({which}): first stage that splits: {first}; {len(finals)} distinct outcome(s) of the final gradients in "
          f"{len(chains) + 1} runs; differing elements {report}")  # fmt: skip
    assert first in (None, "raster_backward"), report
    if int(k.max()) <= 2:
        assert first is None and len(finals) == 1
    else:
        rows = (k >= 3).nonzero().flatten()
        moved = torch.stack([(c["raster_backward"]["v_splats"] != outs["raster_backward"]["v_splats"]).any(dim=1).cpu() for c in chains]).any(dim=0)
        assert set(moved.nonzero().flatten().tolist()) <= set(rows.tolist())
        for n in ("v_means", "v_opacities", "loss"):  # (what the old write-up saw repeat is not asserted: printed)
            print(f"  {n}: differs in some run: {any(not torch.equal(step.flat(c)[n], rec[n]) for c in chains)}")
