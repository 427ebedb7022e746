#!/usr/bin/env python3
"""Deformation-MLP training call (forward + backward to the parameter gradients): the fused path (``FG_FUSED_MLP_TRAIN=1``:
``ops.mlp_train`` through the module's dispatch) against the torch path of the same module (the variable unset), which is
what runs without this knob.  Writes profiles/mlp_train.md.

    python scripts/mlp_train_bench.py [--trace] [--parity FILE] [--out DIR] [--md profiles/mlp_train.md]
    python scripts/mlp_train_bench.py --blender [--trace] [--parity FILE]     (writes profiles/mlp_train_inputs.md)

runs the steps below as child processes, each under its own ``timeout -k 10``, stopping at the first that fails (a
fault or a time limit in one step starts nothing more on the GPU):

    --step time    N = 33 000, 240 000, 1 000 000: the two paths ALTERNATE call by call in one process, 10 warm-up and
                   50 timed calls each between device events; median, p10, p90; FLOPs per row from the layer shapes
    --step error   both paths at N = 40 000 against a float64 run of the same module on the CPU (default init, one time
                   per row): outputs and parameter gradients, the fused path's margin beside the torch fp32 path's own,
                   over all rows and over the rows clear of the ReLU's kink (the tests' filter)
    --step model   ``get_outputs`` + ``get_loss_dict`` + backward of a ``FreeGaussianModel`` in training mode behind
                   ``warm_up``, knob on and off alternating: 240 000 random Gaussians at 960 x 540 (the half resolution
                   of the reference's deform phase), the non-blender net (the blender net keeps the torch path)
    --step trace   three fused calls at N = 240 000 for ``rocprofv3 --kernel-trace --stats`` (with --trace; a run of its own)
    --step report  profiles/mlp_train.md from these; --parity: a ``FG_PARITY_REPORT`` file of tests/test_mlp_train_gpu.py,
                   whose margins are quoted

``--blender`` is the same protocol for the blender net (a 30-wide learned time code: ``timenet`` in front of the trunk)
under ``FG_FUSED_MLP_TRAIN=2``, whose backward also forms the gradient of the input row (``fg_mlp_bwd_inputs``): the steps
time, model (the default ``FreeGaussianModel``, which builds that net) and trace -- not error: the row filter it needs knows
the non-blender net only, and tests/test_mlp_inputs_gpu.py holds this path to float64, whose margins --parity quotes -- and

    --step kernel  ``fg_mlp_bwd`` and ``fg_mlp_bwd_inputs`` on the same saved activations and head cotangents at N = 240 000,
                   alternating call by call between device events (each call: its weight re-ordering launches and the
                   kernel); the trace step runs both as well, so that the kernel table holds each kernel's own time

``--wgrad`` measures the fused parameter-gradient call (``fg_mlp_param_grads``; knob ``FG_FUSED_MLP_WGRAD=1`` on top of
``FG_FUSED_MLP_TRAIN``) against the library products it replaces (``deform.mlp_param_grads``: the knob unset, the same
build) and writes profiles/mlp_wgrad.md.  Its steps, each a child process as above:

    --step wcall   the call alone against ``deform.mlp_param_grads`` on the same random arrays (the tests' generators) at
                   N = 33 000, 240 000, 1 000 000 for aux widths 21 and 30, alternating call by call
    --step werror  both at N = 33 000 against ``deform.mlp_param_grads`` of the same arrays in float64 on the CPU
    --step wtrain  the whole ``ops.mlp_train`` forward + backward through the module, ``FG_FUSED_MLP_WGRAD`` set and unset,
                   under ``FG_FUSED_MLP_TRAIN=1`` (and, with --blender, the blender net under ``=2``)
    --step wmodel  the model training step of --step model, the knob set and unset (with --blender: the default model)
    --step wtrace  three calls of each side at N = 240 000, both aux widths, for ``rocprofv3 --kernel-trace --stats``
    --step wreport profiles/mlp_wgrad.md; --parity: a ``FG_PARITY_REPORT`` file of tests/test_mlp_wgrad_gpu.py

``--chunked`` measures the backward in row chunks (``fg_mlp_train_bwd``; knob ``FG_FUSED_MLP_CHUNKED=1`` on top of the two
above) against the two calls it combines, ``fg_mlp_bwd_inputs`` + ``fg_mlp_param_grads`` of the same build, and writes
profiles/mlp_chunked_bwd.md.  Its steps, each a child process as above:

    --step ccall   the backward alone on one real forward's activations at N = 33 000, 240 000, 1 000 000 for aux widths 21
                   and 30: ``chunk_slabs`` 16, 21, 32, 42 and all the slabs (one chunk), each alternating call by call with
                   the two calls; launches per call; the candidate the rule of the report picks
    --step ctrain  the whole ``ops.mlp_train`` forward + backward through the module, the knob set and unset (with --blender:
                   the blender net under ``FG_FUSED_MLP_TRAIN=2``)
    --step cmodel  the model training step of --step model for the default (blender) model, the knob set and unset
    --step cmem    peak allocated bytes per row of one forward + backward of the blender net above the level before it: the
                   torch path, the fused path with a whole ``G`` and the chunked path, at 240 000 and 1 000 000 rows
    --step ctrace  three calls of each side at N = 240 000, both aux widths, for ``rocprofv3 --kernel-trace --stats``
    --step creport profiles/mlp_chunked_bwd.md; --parity: a ``FG_PARITY_REPORT`` file of tests/test_mlp_chunked_gpu.py
With ``--parent-lib FILE`` (the library built from the parent commit) it also runs ``--step wcall`` and ``--step kernel
--blender`` once on each build (``--lib``: the library a step loads), for the table that shows what the kernels' new
arguments cost the existing entry points.

With ``--precision`` it compares the opt-in split-bf16 mode (``FG_FUSED_MLP_PRECISION=bf16x3``; include/fgraster.h has the
contract) with the fp32 path OF THE SAME BUILD, the two sides alternating call by call, and writes
profiles/mlp_split_bf16.md from these and from what ``scripts/mlp_forward_bench.py --precision`` left in the same directory
(results/mlp_split):

    --step ptrain  the whole fused training call (``ops.mlp_train`` forward + backward through the module,
                   ``FG_FUSED_MLP_WGRAD=1``), the deformation net and with --blender the blender net, at the three sizes
    --step pmodel  one model training step at 240 000 Gaussians, 960 x 540 (with --blender: the blender model)
    --step perror  every stored array and the gradients at N = 33 000 against float64 on the CPU, split beside fp32, over
                   all rows and over the rows clear of the ReLU's kink by 1e-4
    --step ptrace  three training calls of either precision at N = 240 000 for ``rocprofv3`` (with --trace)
    --step preport profiles/mlp_split_bf16.md

With ``--wgrad-precision`` it compares the opt-in split-bf16 mode of the fused parameter-gradient products
(``FG_FUSED_MLP_WGRAD_PRECISION=bf16x3`` on top of ``FG_FUSED_MLP_WGRAD=1``; ``fg_mlp_param_grads_p``) with the fp32 entry
point OF THE SAME BUILD, the sides alternating call by call, and writes profiles/mlp_wgrad_split.md:

    --step scall     ``ops.mlp_param_grads`` alone, precision "bf16x3" against "fp32", at the three sizes, aux widths 21 and 30
    --step serror    both at N = 33 000 against ``deform.mlp_param_grads`` of the same arrays in float64 on the CPU
    --step strain    the whole fused training call for both chain precisions x both values of the new knob, the four
                     alternating call by call (with --blender: the blender net)
    --step smodel    one model training step at 240 000 Gaussians, 960 x 540, the same four settings
    --step strace    three training calls of each setting at N = 240 000 for ``rocprofv3 --kernel-trace --stats`` (with --trace)
    --step scounters three calls of the split products alone for ``rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE``
                     (with --trace; a run of its own, no tracing beside the counters)
    --step sreport   profiles/mlp_wgrad_split.md (its hand-written ``## Notes`` section is kept)
"""
import argparse
import copy
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SIZES = (33_000, 240_000, 1_000_000)
WARM, TIMED = 10, 50
PEAK_TF = 157.0  # fp32 matrix peak of an MI355X
KNOB = "FG_FUSED_MLP_TRAIN"
BLENDER = False  # --blender: the blender net under KNOB=2 (the backward with input-row gradients)


def flops_per_row(m):
    """Forward: 2 x in x out over every linear.  Backward: the same again for each weight gradient, and once more for the
    data gradient of every linear whose input is an activation (not layer 0, not the input columns of layer 5; the
    blender net: those two as well -- its input row wants a gradient; ``timenet`` runs on one row and is not counted)."""
    fwd = data = 0
    for i, layer in enumerate(m.linear):
        fwd += 2 * layer.in_features * layer.out_features
        data += 0 if i == 0 else 2 * m.W * layer.out_features
        if m.is_blender and i in (0, m.skip_at + 1):
            data += 2 * m.input_ch * layer.out_features
    for head in (m.branch_w, m.branch_v, m.gaussian_rotation, m.gaussian_scaling):
        fwd += 2 * head.in_features * head.out_features
        data += 2 * head.in_features * head.out_features
    return 2 * fwd + data


def _quantiles(ms):
    s = sorted(ms)
    q = lambda p: s[min(len(s) - 1, int(round(p * (len(s) - 1))))]  # noqa: E731
    return {"median": q(0.5), "p10": q(0.1), "p90": q(0.9)}


def _timed_pair(run_fused, run_torch, warm=WARM, timed=TIMED):
    """Alternate the two callables; -> (fused ms list, torch ms list) from device events."""
    out = {"fused": [], "torch": []}
    for i in range(warm + timed):
        for name, fn in (("fused", run_fused), ("torch", run_torch)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warm:
                out[name].append(a.elapsed_time(b))
    return out["fused"], out["torch"]


def _module():
    from freegaussian_amd.deform import FreeGaussianDeformableModel

    torch.manual_seed(0)
    return FreeGaussianDeformableModel(is_blender=BLENDER)


def _knob(on):
    if on:
        os.environ[KNOB] = "2" if BLENDER else "1"
    else:
        os.environ.pop(KNOB, None)


def _count_fused_calls():
    from freegaussian_amd import ops

    calls = []
    real = ops.mlp_train
    ops.mlp_train = lambda *a, **k: calls.append(1) or real(*a, **k)
    return calls


def _train_call(m, x, t, cots):
    m.zero_grad(set_to_none=True)
    torch.autograd.backward(m(x, t), cots)


def step_time(out):
    m = _module().cuda()
    fl = flops_per_row(m)
    res = {"flops_per_row": fl, "sizes": {}}
    calls = _count_fused_calls()
    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        x = (torch.rand(n, 3, generator=g) * 2 - 1).cuda()
        t = torch.full((1, 1), 0.4, device="cuda").expand(n, -1)
        cots = [torch.randn(n, *s, generator=g).cuda() for s in ((4, 4), (4,), (3,))]

        def run_fused():
            _knob(True)
            _train_call(m, x, t, cots)

        def run_torch():
            _knob(False)
            _train_call(m, x, t, cots)

        before = len(calls)
        f, p = _timed_pair(run_fused, run_torch)
        assert len(calls) - before == WARM + TIMED  # the fused path ran the kernels, the torch path never did
        qf, qp = _quantiles(f), _quantiles(p)
        res["sizes"][str(n)] = {"fused_ms": qf, "torch_ms": qp, "ratio": qf["median"] / qp["median"],
                                "fused_tflops": fl * n / qf["median"] / 1e9, "torch_tflops": fl * n / qp["median"] / 1e9,
                                "peak_alloc_gb": torch.cuda.max_memory_allocated() / 1e9}  # fmt: skip
        print(n, res["sizes"][str(n)], flush=True)
    json.dump(res, open(os.path.join(out, "time.json"), "w"), indent=1)


def step_error(out):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from mlp_train_common import rows_clear_of_the_kink  # (the row filter of tests/test_mlp_train_gpu.py)

    from freegaussian_amd.deform import FUSED_MIN_ROWS

    n = 40_000  # (enough for the clear rows alone to reach the dispatch threshold)
    m = _module()
    g = torch.Generator().manual_seed(1)
    x, t = torch.rand(n, 3, generator=g) * 2 - 1, torch.rand(n, 1, generator=g)
    cots = [torch.randn(n, *s, generator=g, dtype=torch.float64) for s in ((4, 4), (4,), (3,))]
    clear = rows_clear_of_the_kink(m, x, t)
    assert int(clear.sum()) >= FUSED_MIN_ROWS
    md = copy.deepcopy(m).cuda()
    calls = _count_fused_calls()

    def rel(a, b):
        return float((a.detach().double().cpu() - b).abs().max() / b.abs().max())

    res = {"rows": {"all rows": n, "rows clear of the ReLU kink": int(clear.sum())}}
    for label, rows in (("all rows", torch.ones(n, dtype=torch.bool)), ("rows clear of the ReLU kink", clear)):
        xr, tr, cr = x[rows], t[rows], [c[rows] for c in cots]
        m64 = copy.deepcopy(m).double()
        want_out = m64(xr.double(), tr.double())
        torch.autograd.backward(want_out, cr)
        want = {k: p.grad for k, p in m64.named_parameters()}
        xd, td, cd = xr.cuda(), tr.cuda(), [c.float().cuda() for c in cr]
        for name, on in (("fused", True), ("torch_fp32", False)):
            _knob(on)
            md.zero_grad(set_to_none=True)
            outs = md(xd, td)
            torch.autograd.backward(outs, cd)
            worst = {}
            for k, o, w in zip(("d_xyz", "d_rot", "d_scale"), outs, want_out):
                worst[k] = rel(o, w.detach())
            for k, p in md.named_parameters():
                kind = "weight gradients" if k.endswith("weight") else "bias gradients"
                worst[kind] = max(worst.get(kind, 0.0), rel(p.grad, want[k]))
            for k, v in worst.items():
                res.setdefault(f"{k}, {label}", {})[name] = v
    assert len(calls) == 2
    print(res, flush=True)
    json.dump(res, open(os.path.join(out, "error.json"), "w"), indent=1)


def step_model(out):
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    n, W, H = 240_000, 960, 540
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-4.5, is_blender=BLENDER)
    with torch.no_grad():
        for q in model.deform.parameters():
            q.mul_(0.3)
    model.step = 4000
    model = model.cuda().train()
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1  # OpenCV -> OpenGL camera axes (utils.get_viewmat flips them back)
    cam = Camera(c2w[None, :3], 750.0, 750.0, W / 2, H / 2, W, H, times=torch.tensor([[0.4]]))
    gt = torch.rand(H, W, 3, device="cuda")
    calls = _count_fused_calls()

    def step(on):
        def run():
            _knob(on)
            model.zero_grad(set_to_none=True)
            model.get_loss_dict(model.get_outputs(cam), {"image": gt})["main_loss"].backward()
        return run

    warm, timed = 5, 30
    f, p = _timed_pair(step(True), step(False), warm=warm, timed=timed)
    assert len(calls) == warm + timed
    res = {"n": n, "width": W, "height": H, "fused_ms": _quantiles(f), "torch_ms": _quantiles(p)}
    print(res, flush=True)
    json.dump(res, open(os.path.join(out, "model.json"), "w"), indent=1)


def step_trace(out):
    m = _module().cuda()
    n = 240_000
    x = (torch.rand(n, 3) * 2 - 1).cuda()
    t = torch.full((1, 1), 0.4, device="cuda").expand(n, -1)
    cots = [torch.randn(n, *s).cuda() for s in ((4, 4), (4,), (3,))]
    _knob(True)
    for _ in range(3):
        _train_call(m, x, t, cots)
    torch.cuda.synchronize()
    if BLENDER:  # both backward kernels on the same inputs, for the table
        run_plain, run_inputs = _backward_calls(m, n)
        for _ in range(3):
            run_plain()
            run_inputs()
        torch.cuda.synchronize()


def _backward_calls(m, n):
    """(fg_mlp_bwd, fg_mlp_bwd_inputs) as callables on the activations of one training forward of ``m`` over n rows."""
    import ctypes

    from freegaussian_amd import _lib, ops

    g = torch.Generator().manual_seed(n)
    x = (torch.rand(n, 3, generator=g) * 2 - 1).cuda()
    aux = torch.randn(1, m.input_ch - 63, generator=g).cuda()
    heads = (m.branch_w, m.branch_v, m.gaussian_rotation, m.gaussian_scaling)
    d, _, rows, keep = ops._mlp_desc("bench", x, aux, m.linear, heads, _lib.MLP_PLAIN)
    lib = _lib.load()
    raw = torch.empty(n, sum(rows), device="cuda")
    enc = torch.empty(n, _lib.mlp_enc_width(d.aux_width), device="cuda")
    H, G = torch.empty(8, n, 256, device="cuda"), torch.empty(8, n, 256, device="cuda")
    g_enc, g_heads = torch.empty_like(enc), torch.randn(n, sum(rows), generator=g).cuda()
    ws = torch.empty(int(lib.fg_mlp_bwd_inputs_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    small = int(lib.fg_mlp_train_workspace_bytes(n))
    ptr, st = ctypes.addressof(d), ops._stream()
    ops._call("fg_mlp_train_fwd", n, ptr, raw.data_ptr(), enc.data_ptr(), H.data_ptr(), ws.data_ptr(), small, st)
    torch.cuda.synchronize()
    hold = (d, keep, raw, enc, H, G, g_enc, g_heads, ws)

    def run_plain(hold=hold):
        ops._call("fg_mlp_bwd", n, ptr, g_heads.data_ptr(), H.data_ptr(), G.data_ptr(), ws.data_ptr(), small, st)

    def run_inputs(hold=hold):
        ops._call("fg_mlp_bwd_inputs", n, ptr, g_heads.data_ptr(), H.data_ptr(), G.data_ptr(), g_enc.data_ptr(), ws.data_ptr(),
                  ws.numel(), st)  # fmt: skip

    return run_plain, run_inputs


def step_kernel(out):
    m = _module().cuda()
    n = 240_000
    run_plain, run_inputs = _backward_calls(m, n)
    f, p = _timed_pair(run_inputs, run_plain)
    qf, qp = _quantiles(f), _quantiles(p)
    res = {"n": n, "aux_width": m.input_ch - 63, "inputs_ms": qf, "plain_ms": qp, "ratio": qf["median"] / qp["median"]}
    print(res, flush=True)
    json.dump(res, open(os.path.join(out, "kernel.json"), "w"), indent=1)


def _ms(q):
    return f"{q['median']:.3f} ({q['p10']:.3f} .. {q['p90']:.3f})"


# ---- --wgrad: the fused parameter-gradient call ---------------------------------------------------------------------------
WGRAD_KNOB = "FG_FUSED_MLP_WGRAD"
WGRAD_ROWS = (3, 3, 4, 3)
WGRAD_FLOP_PER_ROW = 2 * 256 * (7 * 256 + 16)  # + 2 x 2 x 256 x in_ch for the two input products


def _wgrad_arrays(n, A, seed=0):
    """The generators of tests/test_mlp_wgrad_gpu.py, on the device: (enc, H, G, g_heads)."""
    from freegaussian_amd import _lib

    g = torch.Generator(device="cuda").manual_seed(1000 * A + seed)
    enc = torch.rand(n, _lib.mlp_enc_width(A), generator=g, device="cuda") * 2 - 1
    enc[:, 63 + A :] = 0.0
    H = torch.randn(8, n, 256, generator=g, device="cuda").relu_()
    G = torch.randn(8, n, 256, generator=g, device="cuda")
    for l in range(8):  # (layer by layer: no second [8, N, 256] temporary at a million rows)
        G[l] *= (torch.rand(n, 256, generator=g, device="cuda") < 0.5) * 1e-3
    return enc, H, G, torch.randn(n, sum(WGRAD_ROWS), generator=g, device="cuda") * 1e-3


def _wgrad_pair(enc, H, G, gh, A):
    from freegaussian_amd import deform, ops

    def run_fused():
        return ops.mlp_param_grads(enc, H, G, gh, A, WGRAD_ROWS)

    def run_lib():  # what _MlpTrain.backward does with the knob unset, the column copy of enc included
        return deform.mlp_param_grads(enc[:, : 63 + A], H, G, gh, WGRAD_ROWS)

    return run_fused, run_lib


def wstep_call(out):
    from freegaussian_amd import _lib, ops

    res = {}
    for A in (21, 30):
        for n in SIZES:
            arrays = _wgrad_arrays(n, A)
            run_fused, run_lib = _wgrad_pair(*arrays, A)
            f, p = _timed_pair(run_fused, run_lib)
            qf, qp = _quantiles(f), _quantiles(p)
            fl = (WGRAD_FLOP_PER_ROW + 4 * 256 * (63 + A)) * n
            res[f"{A},{n}"] = {"aux_width": A, "n": n, "fused_ms": qf, "lib_ms": qp, "ratio": qf["median"] / qp["median"],
                               "fused_tflops": fl / qf["median"] / 1e9, "lib_tflops": fl / qp["median"] / 1e9,
                               "slab_rows": ops.mlp_wgrad_slab_rows(n), "slabs": -(-n // ops.mlp_wgrad_slab_rows(n)),
                               "workspace_mb": int(_lib.load().fg_mlp_param_grads_workspace_bytes(n)) / 1e6}  # fmt: skip
            print(res[f"{A},{n}"], flush=True)
            del arrays, run_fused, run_lib
            torch.cuda.empty_cache()
    json.dump(res, open(os.path.join(out, "wcall.json"), "w"), indent=1)


def wstep_error(out):
    from freegaussian_amd import deform

    n, res = 33_000, {}

    def rel(a, b):
        return float((a.double().cpu() - b).abs().max() / b.abs().max())

    for A in (21, 30):
        enc, H, G, gh = _wgrad_arrays(n, A)
        run_fused, run_lib = _wgrad_pair(enc, H, G, gh, A)
        want = deform.mlp_param_grads(enc[:, : 63 + A].double().cpu(), H.double().cpu(), G.double().cpu(), gh.double().cpu(), WGRAD_ROWS)
        for name, got in (("fused", run_fused()), ("library", run_lib())):
            for kind, gs, ws in zip(("trunk weights", "trunk biases", "head weights", "head biases"), got, want):
                res.setdefault(f"{kind}, aux width {A}", {})[name] = max(rel(g, w) for g, w in zip(gs, ws))
    print(res, flush=True)
    json.dump(res, open(os.path.join(out, "werror.json"), "w"), indent=1)


def _wgrad_knob(on):
    if on:
        os.environ[WGRAD_KNOB] = "1"
    else:
        os.environ.pop(WGRAD_KNOB, None)


def _count_wgrad_calls():
    from freegaussian_amd import ops

    calls = []
    real = ops.mlp_param_grads
    ops.mlp_param_grads = lambda *a, **k: calls.append(1) or real(*a, **k)
    return calls


def wstep_train(out):
    m = _module().cuda()
    _knob(True)
    calls, res = _count_wgrad_calls(), {}
    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        x = (torch.rand(n, 3, generator=g) * 2 - 1).cuda()
        t = torch.full((1, 1), 0.4, device="cuda").expand(n, -1)
        cots = [torch.randn(n, *s, generator=g).cuda() for s in ((4, 4), (4,), (3,))]

        def run(on):
            def go():
                _wgrad_knob(on)
                _train_call(m, x, t, cots)
            return go

        before = len(calls)
        f, p = _timed_pair(run(True), run(False))
        assert len(calls) - before == WARM + TIMED  # the knob's side made the fused call, the other never
        qf, qp = _quantiles(f), _quantiles(p)
        res[str(n)] = {"on_ms": qf, "off_ms": qp, "ratio": qf["median"] / qp["median"]}
        print(n, res[str(n)], flush=True)
    json.dump(res, open(os.path.join(out, "wtrain_blender.json" if BLENDER else "wtrain.json"), "w"), indent=1)


def wstep_model(out):
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    n, W, H = 240_000, 960, 540
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-4.5, is_blender=BLENDER)
    with torch.no_grad():
        for q in model.deform.parameters():
            q.mul_(0.3)
    model.step = 4000
    model = model.cuda().train()
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1
    cam = Camera(c2w[None, :3], 750.0, 750.0, W / 2, H / 2, W, H, times=torch.tensor([[0.4]]))
    gt = torch.rand(H, W, 3, device="cuda")
    _knob(True)
    calls = _count_wgrad_calls()

    def step(on):
        def run():
            _wgrad_knob(on)
            model.zero_grad(set_to_none=True)
            model.get_loss_dict(model.get_outputs(cam), {"image": gt})["main_loss"].backward()
        return run

    warm, timed = 5, 30
    f, p = _timed_pair(step(True), step(False), warm=warm, timed=timed)
    assert len(calls) == warm + timed
    res = {"n": n, "width": W, "height": H, "on_ms": _quantiles(f), "off_ms": _quantiles(p)}
    print(res, flush=True)
    json.dump(res, open(os.path.join(out, "wmodel_blender.json" if BLENDER else "wmodel.json"), "w"), indent=1)


def wstep_trace(out):
    for A in (21, 30):
        arrays = _wgrad_arrays(240_000, A)
        run_fused, run_lib = _wgrad_pair(*arrays, A)
        for _ in range(3):
            run_fused()
            run_lib()
        torch.cuda.synchronize()


def wstep_report(out, md, parity):
    from freegaussian_amd.deform import FUSED_MIN_ROWS

    call = json.load(open(os.path.join(out, "wcall.json")))
    L = ["# Fused parameter-gradient call (`fg_mlp_param_grads`, `FG_FUSED_MLP_WGRAD=1`) against the library products", "",
         "Written by `scripts/mlp_train_bench.py --wgrad` on an MI355X.  The baseline of every table is the knob-unset path of the",
         "same build (`deform.mlp_param_grads`: the chunked library products and their reductions), never an earlier figure.",
         f"One process per table, {WARM} warm-up and {TIMED} timed calls each between device events, the two sides alternating call by call.", "",
         "## (a) The call alone, on the same arrays (the generators of tests/test_mlp_wgrad_gpu.py; head rows (3, 3, 4, 3))", "",
         "TFLOP/s: the products' 2 x 256 x (7 x 256 + 2 x in_ch + 16) FLOP per row over the call's time (of the "
         f"{PEAK_TF:.0f} TFLOP/s fp32 matrix peak).", "",
         "| aux width | N | slabs x rows | workspace MB | fused ms median (p10 .. p90) | library ms median (p10 .. p90) | fused / library | "
         "fused TFLOP/s | library TFLOP/s |", "|---|---|---|---|---|---|---|---|---|"]  # fmt: skip
    for r in call.values():
        L.append(f"| {r['aux_width']} | {r['n']:,} | {r['slabs']} x {r['slab_rows']} | {r['workspace_mb']:.0f} | {_ms(r['fused_ms'])} | "
                 f"{_ms(r['lib_ms'])} | {r['ratio']:.2f} | {r['fused_tflops']:.1f} | {r['lib_tflops']:.1f} |")  # fmt: skip
    at = [r for r in call.values() if r["n"] == 240_000]
    gain = all(r["fused_ms"]["median"] < r["lib_ms"]["median"] and r["fused_ms"]["p90"] < r["lib_ms"]["p10"] for r in at)
    wins = sorted({r["n"] for r in call.values()
                   if all(q["fused_ms"]["p90"] < q["lib_ms"]["p10"] for q in call.values() if q["n"] == r["n"])})
    L += ["", "**Outcome by the rule set for this call** (at 240 000 rows: the fused median below the library's with non-overlapping p10 .. p90, both "
          "aux widths): " + ("a gain." if gain else "NO gain is claimed; the call stays (it is correct and deterministic).")
          + f"  Sizes at which the fused call wins by that rule for both widths: {', '.join(f'{n:,}' for n in wins) or 'none'}."
          + f"  The knob stays opt-in either way; a fused training call sees at least `deform.FUSED_MIN_ROWS` = {FUSED_MIN_ROWS:,} rows."]  # fmt: skip
    for name, title in (("wtrain.json", "deformation net, `FG_FUSED_MLP_TRAIN=1`"), ("wtrain_blender.json", "blender net, `FG_FUSED_MLP_TRAIN=2`")):
        if os.path.exists(os.path.join(out, name)):
            tr = json.load(open(os.path.join(out, name)))
            L += ["", f"## (b) The whole `ops.mlp_train` forward + backward through the module ({title})", "",
                  f"| N | `{WGRAD_KNOB}=1` ms median (p10 .. p90) | unset ms median (p10 .. p90) | set / unset |", "|---|---|---|---|"]
            L += [f"| {int(n):,} | {_ms(r['on_ms'])} | {_ms(r['off_ms'])} | {r['ratio']:.2f} |" for n, r in tr.items()]
    for name, title in (("wmodel.json", "non-blender net, `FG_FUSED_MLP_TRAIN=1`"), ("wmodel_blender.json", "the default model -- the blender net -- `FG_FUSED_MLP_TRAIN=2`")):
        if os.path.exists(os.path.join(out, name)):
            fr = json.load(open(os.path.join(out, name)))
            L += ["", f"## (c) Model training step (`get_outputs` + `get_loss_dict` + backward; {fr['n']:,} random Gaussians behind `warm_up`, "
                  f"{fr['width']} x {fr['height']}; {title})", "", "| knob | ms per step median (p10 .. p90) |", "|---|---|",
                  f"| `{WGRAD_KNOB}` unset | {_ms(fr['off_ms'])} |", f"| `{WGRAD_KNOB}=1` | {_ms(fr['on_ms'])} |"]  # fmt: skip
    stats = sorted(glob.glob(os.path.join(out, "wtrace", "**", "*kernel_stats.csv"), recursive=True))
    if stats:
        L += ["", "## (d) Kernels of three calls of each side at N = 240 000, aux widths 21 and 30 (`rocprofv3 --kernel-trace --stats`, a run "
              "of its own; no counters)", "", "| kernel | calls | average us | share % |", "|---|---|---|---|"]  # fmt: skip
        for r in list(csv.DictReader(open(stats[0])))[:14]:
            L.append(f"| `{r['Name'][:80]}` | {r['Calls']} | {float(r['AverageNs']) / 1e3:.1f} | {float(r['Percentage']):.1f} |")
    if os.path.exists(os.path.join(out, "werror.json")):
        er = json.load(open(os.path.join(out, "werror.json")))
        L += ["", "## (e) Error against float64 at N = 33 000 (`deform.mlp_param_grads` of the same arrays in float64 on the CPU; "
              "max |a - b| / max |b|, worst array; the bar is 1e-4)", "", "| | fused call | library products (fp32) |", "|---|---|---|"]  # fmt: skip
        L += [f"| {k} | {v['fused']:.2e} | {v['library']:.2e} |" for k, v in er.items()]
    if parity and os.path.exists(parity):
        worst = {}
        for line in open(parity):
            r = json.loads(line)
            if "test_mlp_wgrad_gpu.py" in r["test"] and r["kind"] == "rel_err":
                name = r["test"].split("::")[1].split("[")[0]
                worst[name] = max(worst.get(name, 0.0), r["value"])
        L += ["", "## Margins of tests/test_mlp_wgrad_gpu.py (`FG_PARITY_REPORT`: the largest `rel_err` each test saw; the bar is 1e-4)", "",
              "| test | largest rel_err |", "|---|---|"]  # fmt: skip
        L += [f"| `{k}` | {v:.2e} |" for k, v in sorted(worst.items())]
    if os.path.exists(md) and "\n## Notes" in open(md).read():
        L += ["", "## Notes" + open(md).read().split("\n## Notes", 1)[1].rstrip()]
    open(md, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


# ---- --chunked: the backward in row chunks ----------------------------------------------------------------------------------
CHUNK_KNOB = "FG_FUSED_MLP_CHUNKED"
CHUNK_CANDIDATES = (16, 21, 32, 42)


def _use_library(path):
    """Load another build of the library (the parent commit's): the symbols it lacks are not bound."""
    import ctypes

    from freegaussian_amd import _lib

    os.environ["FG_RASTER_LIB"] = path
    lib = ctypes.CDLL(path)
    for name in [n for n in _lib.SIGNATURES if not hasattr(lib, n)]:
        del _lib.SIGNATURES[name]
    if "fg_abi_minor" not in _lib.SIGNATURES:
        _lib.ABI_MINOR = 0


def _chunk_knob(on):
    if on:
        os.environ[CHUNK_KNOB] = "1"
    else:
        os.environ.pop(CHUNK_KNOB, None)


def _count_chunked_calls():
    from freegaussian_amd import ops

    calls = []
    real = ops.mlp_train_backward
    ops.mlp_train_backward = lambda *a, **k: calls.append(1) or real(*a, **k)
    return calls


def _chunked_pair(n, A):
    """(run_chunked(chunk_slabs), run_two_calls) on the activations of one training forward over n rows of the net with an
    aux of width A (21: the deformation net, 30: the blender net)."""
    import ctypes

    from freegaussian_amd import _lib, ops
    from freegaussian_amd.deform import FreeGaussianDeformableModel

    torch.manual_seed(0)
    m = FreeGaussianDeformableModel(is_blender=A == 30).cuda()
    assert m.input_ch - 63 == A
    g = torch.Generator().manual_seed(n)
    x = (torch.rand(n, 3, generator=g) * 2 - 1).cuda()
    aux = torch.randn(1, A, generator=g).cuda()
    heads = (m.branch_w, m.branch_v, m.gaussian_rotation, m.gaussian_scaling)
    d, _, rows, keep = ops._mlp_desc("bench", x, aux, m.linear, heads, _lib.MLP_PLAIN)
    lib = _lib.load()
    raw = torch.empty(n, sum(rows), device="cuda")
    enc = torch.empty(n, _lib.mlp_enc_width(A), device="cuda")
    H = torch.empty(8, n, 256, device="cuda")
    g_heads = (torch.randn(n, sum(rows), generator=g) * 1e-3).cuda()
    ws = torch.empty(int(lib.fg_mlp_bwd_inputs_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    ptr, st = ctypes.addressof(d), ops._stream()
    ops._call("fg_mlp_train_fwd", n, ptr, raw.data_ptr(), enc.data_ptr(), H.data_ptr(), ws.data_ptr(), int(lib.fg_mlp_train_workspace_bytes(n)), st)
    torch.cuda.synchronize()
    hold = (m, d, keep, raw, x, aux)

    def run_two(hold=hold):  # what _MlpTrain.backward does with the knob unset: G and g_enc from the allocator, the two calls
        G, g_enc = torch.empty_like(H), torch.empty_like(enc)
        ops._call("fg_mlp_bwd_inputs", n, ptr, g_heads.data_ptr(), H.data_ptr(), G.data_ptr(), g_enc.data_ptr(), ws.data_ptr(), ws.numel(), st)
        return ops.mlp_param_grads(enc, H, G, g_heads, A, rows), g_enc

    def run_chunked(c, hold=hold):
        return ops.mlp_train_backward(enc, H, g_heads, m.linear, heads, A, rows, want_g_enc=True, chunk_slabs=c)

    return run_chunked, run_two


def cstep_call(out):
    from freegaussian_amd import _lib, ops

    res = {}
    for A in (21, 30):
        for n in SIZES:
            run_chunked, run_two = _chunked_pair(n, A)
            slabs = -(-n // ops.mlp_wgrad_slab_rows(n))
            a, b = run_chunked(3), run_two()  # the same bits, whatever the chunks
            torch.cuda.synchronize()
            same = all(torch.equal(p, q) for ga, gb in zip(a[:4], b[0]) for p, q in zip(ga, gb)) and torch.equal(a[4], b[1])
            assert same
            del a, b
            for c in CHUNK_CANDIDATES + (slabs,):
                f, p = _timed_pair(lambda: run_chunked(c), run_two)
                qf, qp = _quantiles(f), _quantiles(p)
                chunks = -(-slabs // min(c, slabs))
                res[f"{A},{n},{c}"] = {"aux_width": A, "n": n, "chunk_slabs": c, "one_chunk": c >= slabs, "slabs": slabs, "chunks": chunks,
                                       "launches": 2 + 2 * chunks + 1, "two_call_launches": 3 + 2, "chunked_ms": qf, "two_ms": qp,
                                       "ratio": qf["median"] / qp["median"],
                                       "workspace_mb": int(_lib.load().fg_mlp_train_bwd_workspace_bytes(n, c, 1)) / 1e6}  # fmt: skip
                print(res[f"{A},{n},{c}"], flush=True)
            del run_chunked, run_two
            torch.cuda.empty_cache()
    json.dump(res, open(os.path.join(out, "ccall.json"), "w"), indent=1)


def _pick_chunk_slabs(call, A=30, n=240_000):
    """The rule: the candidate with the lowest median at 240 000 rows (the default model's net); where its p10 .. p90 overlaps a
    smaller candidate's, the smaller."""
    rows = sorted((r for r in call.values() if r["aux_width"] == A and r["n"] == n and r["chunk_slabs"] in CHUNK_CANDIDATES),
                  key=lambda r: r["chunk_slabs"])  # fmt: skip
    best = min(rows, key=lambda r: r["chunked_ms"]["median"])
    for r in rows:
        if r["chunk_slabs"] < best["chunk_slabs"] and r["chunked_ms"]["p10"] <= best["chunked_ms"]["p90"] and best["chunked_ms"]["p10"] <= r["chunked_ms"]["p90"]:
            return r["chunk_slabs"], best["chunk_slabs"]
    return best["chunk_slabs"], best["chunk_slabs"]


def cstep_train(out):
    m = _module().cuda()
    _knob(True)
    _wgrad_knob(True)
    calls, res = _count_chunked_calls(), {}
    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        x = (torch.rand(n, 3, generator=g) * 2 - 1).cuda()
        t = torch.full((1, 1), 0.4, device="cuda").expand(n, -1)
        cots = [torch.randn(n, *s, generator=g).cuda() for s in ((4, 4), (4,), (3,))]

        def run(on):
            def go():
                _chunk_knob(on)
                _train_call(m, x, t, cots)
            return go

        before = len(calls)
        f, p = _timed_pair(run(True), run(False))
        assert len(calls) - before == WARM + TIMED  # the knob's side made the chunked call, the other never
        qf, qp = _quantiles(f), _quantiles(p)
        res[str(n)] = {"on_ms": qf, "off_ms": qp, "ratio": qf["median"] / qp["median"]}
        print(n, res[str(n)], flush=True)
    json.dump(res, open(os.path.join(out, "ctrain_blender.json" if BLENDER else "ctrain.json"), "w"), indent=1)


def cstep_model(out):
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    n, W, H = 240_000, 960, 540
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-4.5, is_blender=True)
    with torch.no_grad():
        for q in model.deform.parameters():
            q.mul_(0.3)
    model.step = 4000
    model = model.cuda().train()
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1
    cam = Camera(c2w[None, :3], 750.0, 750.0, W / 2, H / 2, W, H, times=torch.tensor([[0.4]]))
    gt = torch.rand(H, W, 3, device="cuda")
    os.environ[KNOB] = "2"
    _wgrad_knob(True)
    calls = _count_chunked_calls()

    def step(on):
        def run():
            _chunk_knob(on)
            model.zero_grad(set_to_none=True)
            model.get_loss_dict(model.get_outputs(cam), {"image": gt})["main_loss"].backward()
        return run

    warm, timed = 5, 30
    f, p = _timed_pair(step(True), step(False), warm=warm, timed=timed)
    assert len(calls) == warm + timed
    res = {"n": n, "width": W, "height": H, "on_ms": _quantiles(f), "off_ms": _quantiles(p)}
    print(res, flush=True)
    json.dump(res, open(os.path.join(out, "cmodel.json"), "w"), indent=1)


def cstep_mem(out):
    from freegaussian_amd.deform import FreeGaussianDeformableModel

    torch.manual_seed(0)
    m = FreeGaussianDeformableModel(is_blender=True).cuda()
    res = {}
    paths = (("torch path (no knob)", {}), ("fused, whole G (`FG_FUSED_MLP_TRAIN=2`, `FG_FUSED_MLP_WGRAD=1`)", {KNOB: "2", WGRAD_KNOB: "1"}),
             ("chunked (`FG_FUSED_MLP_CHUNKED=1` on top)", {KNOB: "2", WGRAD_KNOB: "1", CHUNK_KNOB: "1"}))  # fmt: skip
    for n in (240_000, 1_000_000):
        g = torch.Generator().manual_seed(n)
        x = (torch.rand(n, 3, generator=g) * 2 - 1).cuda()
        t = torch.full((1, 1), 0.4, device="cuda").expand(n, -1)
        cots = [torch.randn(n, *s, generator=g).cuda() for s in ((4, 4), (4,), (3,))]
        for name, env in paths:
            for k in (KNOB, WGRAD_KNOB, CHUNK_KNOB):
                os.environ.pop(k, None)
            os.environ.update(env)
            for _ in range(2):  # (the second call: the library loaded, nothing of the first alive)
                m.zero_grad(set_to_none=True)
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                outs = m(x, t)
                torch.cuda.synchronize()
                after_fwd = torch.cuda.memory_allocated() - before
                torch.autograd.backward(outs, cots)
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated() - before
                del outs
            res[f"{name}|{n}"] = {"path": name, "n": n, "kept_after_forward_per_row": after_fwd / n, "peak_per_row": peak / n, "peak_gb": peak / 1e9}
            print(res[f"{name}|{n}"], flush=True)
    json.dump(res, open(os.path.join(out, "cmem.json"), "w"), indent=1)


def cstep_trace(out):
    for A in (21, 30):
        run_chunked, run_two = _chunked_pair(240_000, A)
        for _ in range(3):
            run_chunked(0)
            run_two()
        torch.cuda.synchronize()


def cstep_report(out, md, parity):
    from freegaussian_amd import _lib
    from freegaussian_amd.deform import FUSED_MIN_ROWS

    call = json.load(open(os.path.join(out, "ccall.json")))
    pick, fastest = _pick_chunk_slabs(call)
    const = _lib.MLP_TRAIN_BWD_CHUNK_SLABS
    L = ["# Fused MLP backward in row chunks (`fg_mlp_train_bwd`, `FG_FUSED_MLP_CHUNKED=1`) against the two calls it combines", "",
         "Written by `scripts/mlp_train_bench.py --chunked` on an MI355X.  The baseline of every table is the knob-unset path of the same",
         "build (`fg_mlp_bwd_inputs` into a whole `G` [8, N, 256], then `fg_mlp_param_grads`), never an earlier figure.  One process per",
         f"table, {WARM} warm-up and {TIMED} timed calls each between device events, the two sides alternating call by call.  The results of",
         "the two sides are the same bits (checked at the start of every case of table (a), and by tests/test_mlp_chunked_gpu.py).", "",
         "## (a) The backward alone, on one real forward's activations (head rows (3, 3, 4, 3), `g_enc` wanted)", "",
         "Launches per call: the weight re-ordering (2), the chain and the slab kernel per chunk, the reduction; the two calls make 5.", "",
         "| aux width | N | slabs | chunk_slabs | chunks | launches | workspace MB | chunked ms median (p10 .. p90) | two calls ms median (p10 .. p90) | "
         "chunked / two calls |", "|---|---|---|---|---|---|---|---|---|---|"]  # fmt: skip
    for r in call.values():
        c = f"{r['chunk_slabs']} (all: one chunk)" if r["chunk_slabs"] == r["slabs"] else (f"{r['chunk_slabs']} (capped: one chunk)" if r["one_chunk"] else str(r["chunk_slabs"]))
        L.append(f"| {r['aux_width']} | {r['n']:,} | {r['slabs']} | {c} | {r['chunks']} | {r['launches']} | {r['workspace_mb']:.0f} | "
                 f"{_ms(r['chunked_ms'])} | {_ms(r['two_ms'])} | {r['ratio']:.3f} |")  # fmt: skip
    L += ["", f"**The library's constant.**  Rule: the candidate of {CHUNK_CANDIDATES} with the lowest median at 240 000 rows (aux width 30, the default "
          f"model's net); where its p10 .. p90 overlaps a smaller candidate's, the smaller.  Lowest median: {fastest}; by the rule: **{pick}**.  "
          f"`FG_MLP_TRAIN_BWD_CHUNK_SLABS` of the build that ran tables (b) to (e): {const}" + ("." if const == pick else " -- NOT the rule's pick.")]  # fmt: skip
    L += ["", "Chunked / two calls with the library's constant, as measured (above 1: the chunked call is slower by that factor):", ""]
    for r in call.values():
        if r["chunk_slabs"] == const:
            L.append(f"- aux width {r['aux_width']}, N = {r['n']:,}: {r['ratio']:.3f}")
    for name, title in (("ctrain.json", "deformation net, `FG_FUSED_MLP_TRAIN=1`"), ("ctrain_blender.json", "blender net, `FG_FUSED_MLP_TRAIN=2`")):
        if os.path.exists(os.path.join(out, name)):
            tr = json.load(open(os.path.join(out, name)))
            L += ["", f"## (b) The whole `ops.mlp_train` forward + backward through the module ({title}, `{WGRAD_KNOB}=1`)", "",
                  f"| N | `{CHUNK_KNOB}=1` ms median (p10 .. p90) | unset ms median (p10 .. p90) | set / unset |", "|---|---|---|---|"]
            L += [f"| {int(n):,} | {_ms(r['on_ms'])} | {_ms(r['off_ms'])} | {r['ratio']:.3f} |" for n, r in tr.items()]
    if os.path.exists(os.path.join(out, "cmodel.json")):
        fr = json.load(open(os.path.join(out, "cmodel.json")))
        L += ["", f"## (c) Model training step (`get_outputs` + `get_loss_dict` + backward; the default model -- the blender net -- {fr['n']:,} random "
              f"Gaussians behind `warm_up`, {fr['width']} x {fr['height']}; `FG_FUSED_MLP_TRAIN=2`, `{WGRAD_KNOB}=1`)", "",
              "| knob | ms per step median (p10 .. p90) |", "|---|---|",
              f"| `{CHUNK_KNOB}` unset | {_ms(fr['off_ms'])} |", f"| `{CHUNK_KNOB}=1` | {_ms(fr['on_ms'])} |"]  # fmt: skip
    if os.path.exists(os.path.join(out, "cmem.json")):
        mem = json.load(open(os.path.join(out, "cmem.json")))
        L += ["", "## (d) Peak allocated bytes per row (`torch.cuda.max_memory_allocated` over one forward + backward of the blender net through the "
              "module, above the level before the call: inputs, cotangents and parameters are not counted)", "",
              "| path | N | kept after the forward, bytes per row | peak, bytes per row | peak GB |", "|---|---|---|---|---|"]  # fmt: skip
        L += [f"| {r['path']} | {r['n']:,} | {r['kept_after_forward_per_row']:,.0f} | {r['peak_per_row']:,.0f} | {r['peak_gb']:.2f} |" for r in mem.values()]
    stats = sorted(glob.glob(os.path.join(out, "ctrace", "**", "*kernel_stats.csv"), recursive=True))
    if stats:
        L += ["", "## (e) Kernels of three calls of each side at N = 240 000, aux widths 21 and 30 (`rocprofv3 --kernel-trace --stats`, a run "
              "of its own; no counters)", "", "| kernel | calls | average us | share % |", "|---|---|---|---|"]  # fmt: skip
        for r in list(csv.DictReader(open(stats[0])))[:12]:
            L.append(f"| `{r['Name'][:80]}` | {r['Calls']} | {float(r['AverageNs']) / 1e3:.1f} | {float(r['Percentage']):.1f} |")
    base = {tag: os.path.join(out, f"base_{tag}") for tag in ("this", "parent")}
    if all(os.path.exists(os.path.join(d, "wcall.json")) and os.path.exists(os.path.join(d, "kernel.json")) for d in base.values()):
        w = {tag: json.load(open(os.path.join(d, "wcall.json"))) for tag, d in base.items()}
        k = {tag: json.load(open(os.path.join(d, "kernel.json"))) for tag, d in base.items()}
        L += ["", "## (f) The existing entry points on this build and on the parent commit's (the same GPU visit, a process each): what the "
              "kernels' new arguments cost them", "", "| call | N | aux width | this build ms median (p10 .. p90) | parent build ms median (p10 .. p90) | "
              "this / parent |", "|---|---|---|---|---|---|"]  # fmt: skip
        for key, r in w["this"].items():
            q = w["parent"][key]
            L.append(f"| `fg_mlp_param_grads` | {r['n']:,} | {r['aux_width']} | {_ms(r['fused_ms'])} | {_ms(q['fused_ms'])} | "
                     f"{r['fused_ms']['median'] / q['fused_ms']['median']:.3f} |")  # fmt: skip
        for name, field in (("fg_mlp_bwd_inputs", "inputs_ms"), ("fg_mlp_bwd", "plain_ms")):
            r, q = k["this"], k["parent"]
            L.append(f"| `{name}` | {r['n']:,} | {r['aux_width']} | {_ms(r[field])} | {_ms(q[field])} | {r[field]['median'] / q[field]['median']:.3f} |")
    if parity and os.path.exists(parity):
        worst = {}
        for line in open(parity):
            r = json.loads(line)
            if "test_mlp_chunked_gpu.py" in r["test"] and r["kind"] == "rel_err":
                name = r["test"].split("::")[1].split("[")[0]
                worst[name] = max(worst.get(name, 0.0), r["value"])
        L += ["", "## Margins of tests/test_mlp_chunked_gpu.py (`FG_PARITY_REPORT`: the largest `rel_err` each test saw; the bar is 1e-4; every other "
              "comparison of that file is bit for bit)", "", "| test | largest rel_err |", "|---|---|"]  # fmt: skip
        L += [f"| `{k_}` | {v:.2e} |" for k_, v in sorted(worst.items())]
    L += ["", f"The knob is off unless set; a fused training call sees at least `deform.FUSED_MIN_ROWS` = {FUSED_MIN_ROWS:,} rows."]
    if os.path.exists(md) and "\n## Notes" in open(md).read():
        L += ["", "## Notes" + open(md).read().split("\n## Notes", 1)[1].rstrip()]
    open(md, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


def step_report_inputs(out, md, parity):
    """profiles/mlp_train_inputs.md (--blender)."""
    from freegaussian_amd.deform import FUSED_MIN_ROWS

    tm = json.load(open(os.path.join(out, "time.json")))
    L = ["# Fused fp32 MLP training call with input-row gradients (`FG_FUSED_MLP_TRAIN=2`) against the torch path", "",
         "Written by `scripts/mlp_train_bench.py --blender` on an MI355X.  Blender deformation net (D = 8, W = 256, multires 10, a",
         "30-wide learned time code from `timenet`, one time for all rows), forward + backward to the 28 parameter gradients from",
         f"fixed output cotangents; {tm['flops_per_row']} FLOP per row from the layer shapes (forward, weight gradients, the data",
         f"gradients of the hidden activations and of the input row).  `{KNOB}=2` against the variable unset, alternating call by",
         f"call in one process, {WARM} warm-up and {TIMED} timed calls each between device events.  TFLOP/s: that count over the",
         f"call's time, a whole-call rate (of the {PEAK_TF:.0f} TFLOP/s fp32 matrix peak), not a kernel's.", "",
         "| N | fused ms median (p10 .. p90) | torch ms median (p10 .. p90) | fused / torch | fused TFLOP/s | torch TFLOP/s | peak allocated GB |",
         "|---|---|---|---|---|---|---|"]  # fmt: skip
    for n, r in tm["sizes"].items():
        L.append(f"| {int(n):,} | {_ms(r['fused_ms'])} | {_ms(r['torch_ms'])} | {r['ratio']:.2f} | {r['fused_tflops']:.1f} | "
                 f"{r['torch_tflops']:.1f} | {r['peak_alloc_gb']:.1f} |")  # fmt: skip
    L += ["", f"The knob is off unless set; dispatch from `deform.FUSED_MIN_ROWS` = {FUSED_MIN_ROWS:,} rows.  (Peak allocated: of the",
          "process up to that size, both paths.)"]
    stats = sorted(glob.glob(os.path.join(out, "trace", "**", "*kernel_stats.csv"), recursive=True))
    rows = list(csv.DictReader(open(stats[0]))) if stats else []
    if os.path.exists(os.path.join(out, "kernel.json")):
        kr = json.load(open(os.path.join(out, "kernel.json")))
        L += ["", f"## The backward with input-row gradients against the one without (N = {kr['n']:,}, aux {kr['aux_width']} wide, the same "
              "activations and cotangents)", "",
              "`fg_mlp_bwd`'s kernel is the previous commit's, instruction for instruction (its disassembly was compared), so this is",
              "the new kernel against that one.  By matrix-instruction count the new kernel does 8/7 = 1.14 of the old one's products.", "",
              "| | `fg_mlp_bwd_inputs` | `fg_mlp_bwd` | ratio |", "|---|---|---|---|",
              f"| whole call, ms median (p10 .. p90), device events, alternating | {_ms(kr['inputs_ms'])} | {_ms(kr['plain_ms'])} | "
              f"{kr['ratio']:.2f} |"]  # fmt: skip
        avg = {}
        for r in rows:
            if "mlp_bwd_kernel" in r["Name"]:
                avg["inputs" if ("true" in r["Name"] or "Lb1" in r["Name"]) else "plain"] = float(r["AverageNs"]) / 1e6
        if len(avg) == 2:
            L.append(f"| the kernel alone, average ms (`rocprofv3`, the table below) | {avg['inputs']:.3f} | {avg['plain']:.3f} | "
                     f"{avg['inputs'] / avg['plain']:.2f} |")  # fmt: skip
    if os.path.exists(os.path.join(out, "model.json")):
        fr = json.load(open(os.path.join(out, "model.json")))
        L += ["", f"## Model training step (`get_outputs` + `get_loss_dict` + backward; the default `FreeGaussianModel` -- the blender net "
              f"-- {fr['n']:,} random Gaussians behind `warm_up`, {fr['width']} x {fr['height']})", "",
              "| knob | ms per step median (p10 .. p90) |", "|---|---|",
              f"| unset (the torch path) | {_ms(fr['torch_ms'])} |", f"| `{KNOB}=2` | {_ms(fr['fused_ms'])} |"]  # fmt: skip
    if rows:
        L += ["", "## Kernels of three fused calls, then three calls of each backward entry point, at N = 240 000 "
              "(`rocprofv3 --kernel-trace --stats`, a run of its own)", "",
              "| kernel | calls | average us | share % |", "|---|---|---|---|"]  # fmt: skip
        for r in rows[:14]:
            L.append(f"| `{r['Name'][:80]}` | {r['Calls']} | {float(r['AverageNs']) / 1e3:.1f} | {float(r['Percentage']):.1f} |")
    if parity and os.path.exists(parity):
        worst = {}
        for line in open(parity):
            r = json.loads(line)
            if "test_mlp_inputs_gpu.py" in r["test"] and r["kind"] == "rel_err":
                name = r["test"].split("::")[1].split("[")[0]
                worst[name] = max(worst.get(name, 0.0), r["value"])
        L += ["", "## Margins of tests/test_mlp_inputs_gpu.py (`FG_PARITY_REPORT`: the largest `rel_err` each test saw; the bar is 1e-4)", "",
              "| test | largest rel_err |", "|---|---|"]  # fmt: skip
        L += [f"| `{k}` | {v:.2e} |" for k, v in sorted(worst.items())]
    if os.path.exists(md) and "\n## Notes" in open(md).read():
        L += ["", "## Notes" + open(md).read().split("\n## Notes", 1)[1].rstrip()]
    open(md, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


def step_report(out, md, parity):
    from freegaussian_amd.deform import FUSED_MIN_ROWS

    if BLENDER:
        return step_report_inputs(out, md, parity)
    tm = json.load(open(os.path.join(out, "time.json")))
    L = ["# Fused fp32 MLP training call (`ops.mlp_train`) against the torch path", "",
         "Written by `scripts/mlp_train_bench.py` on an MI355X.  Deformation net (D = 8, W = 256, multires 10, 21-wide time",
         "encoding, one time for all rows), forward + backward to the 24 parameter gradients from fixed output cotangents;",
         f"{tm['flops_per_row']} FLOP per row from the layer shapes (forward, weight gradients, and the data gradients of the hidden",
         f"activations).  `{KNOB}=1` against the variable unset, alternating call by call in one process, {WARM} warm-up and {TIMED}",
         f"timed calls each between device events.  TFLOP/s: that count over the call's time, a whole-call rate (of the {PEAK_TF:.0f}",
         "TFLOP/s fp32 matrix peak), not a kernel's.", "",
         "| N | fused ms median (p10 .. p90) | torch ms median (p10 .. p90) | fused / torch | fused TFLOP/s | torch TFLOP/s | peak allocated GB |",
         "|---|---|---|---|---|---|---|"]  # fmt: skip
    for n, r in tm["sizes"].items():
        L.append(f"| {int(n):,} | {_ms(r['fused_ms'])} | {_ms(r['torch_ms'])} | {r['ratio']:.2f} | {r['fused_tflops']:.1f} | "
                 f"{r['torch_tflops']:.1f} | {r['peak_alloc_gb']:.1f} |")  # fmt: skip
    L += ["", f"The knob is off unless set; dispatch from `deform.FUSED_MIN_ROWS` = {FUSED_MIN_ROWS:,} rows.  (Peak allocated: of the",
          "process up to that size, both paths.)"]
    if os.path.exists(os.path.join(out, "error.json")):
        er = json.load(open(os.path.join(out, "error.json")))
        rows = er.pop("rows")
        L += ["", "## Error against float64 (default init, a time per row; max |a - b| / max |b|, worst array; the bar is 1e-4)", "",
              f"Over {' and over '.join(f'{v:,} {k}' for k, v in rows.items())} (`rows_clear_of_the_kink` of tests/mlp_train_common.py:",
              "no float64 pre-activation within 1e-5 of its layer's largest from zero).  Within fp32 rounding of zero a unit's mask is",
              "either path's to choose, and one flipped unit moves a sum over N rows by about 1 / sqrt(N) of its scale.", "",
              "| | fused path | torch fp32 on the GPU |", "|---|---|---|"]  # fmt: skip
        L += [f"| {k} | {v['fused']:.2e} | {v['torch_fp32']:.2e} |" for k, v in er.items()]
    if parity and os.path.exists(parity):
        worst = {}
        for line in open(parity):
            r = json.loads(line)
            if "test_mlp_train_gpu.py" in r["test"] and r["kind"] == "rel_err":
                name = r["test"].split("::")[1].split("[")[0]
                worst[name] = max(worst.get(name, 0.0), r["value"])
        L += ["", "## Margins of tests/test_mlp_train_gpu.py (`FG_PARITY_REPORT`: the largest `rel_err` each test saw; the bar is 1e-4)", "",
              "| test | largest rel_err |", "|---|---|"]  # fmt: skip
        L += [f"| `{k}` | {v:.2e} |" for k, v in sorted(worst.items())]
    if os.path.exists(os.path.join(out, "model.json")):
        fr = json.load(open(os.path.join(out, "model.json")))
        L += ["", f"## Model training step (`get_outputs` + `get_loss_dict` + backward; {fr['n']:,} random Gaussians behind `warm_up`, "
              f"{fr['width']} x {fr['height']}, non-blender net)", "",
              "| knob | ms per step median (p10 .. p90) |", "|---|---|",
              f"| unset (the torch path) | {_ms(fr['torch_ms'])} |", f"| `{KNOB}=1` | {_ms(fr['fused_ms'])} |"]  # fmt: skip
    stats = sorted(glob.glob(os.path.join(out, "trace", "**", "*kernel_stats.csv"), recursive=True))
    if stats:
        L += ["", "## Kernels of three fused calls at N = 240 000 (`rocprofv3 --kernel-trace --stats`, a run of its own)", "",
              "| kernel | calls | average us | share % |", "|---|---|---|---|"]  # fmt: skip
        for r in list(csv.DictReader(open(stats[0])))[:12]:
            L.append(f"| `{r['Name'][:80]}` | {r['Calls']} | {float(r['AverageNs']) / 1e3:.1f} | {float(r['Percentage']):.1f} |")
    # (hand-written sections of the file -- everything from the first "## Notes" heading on -- are kept)
    if os.path.exists(md) and "\n## Notes" in open(md).read():
        L += ["", "## Notes" + open(md).read().split("\n## Notes", 1)[1].rstrip()]
    open(md, "w").write("\n".join(L) + "\n")
    print("\n".join(L))

# ---- --precision: the split-bf16 mode against fp32 (profiles/mlp_split_bf16.md) -------------------------------------------
PRECISION_KNOB = "FG_FUSED_MLP_PRECISION"


def _precision_knob(value):
    if value == "fp32":
        os.environ.pop(PRECISION_KNOB, None)
    else:
        os.environ[PRECISION_KNOB] = value


def _count_precisions():
    from freegaussian_amd import ops

    seen = []
    real = ops.mlp_train
    ops.mlp_train = lambda *a, **k: seen.append(k.get("precision", "fp32")) or real(*a, **k)
    return seen


def pstep_train(out):
    m = _module().cuda()
    _knob(True)
    _wgrad_knob(True)
    seen, res = _count_precisions(), {"flops_per_row": flops_per_row(m)}
    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        x = (torch.rand(n, 3, generator=g) * 2 - 1).cuda()
        t = torch.full((1, 1), 0.4, device="cuda").expand(n, -1)
        cots = [torch.randn(n, *s, generator=g).cuda() for s in ((4, 4), (4,), (3,))]

        def run(value):
            def go():
                _precision_knob(value)
                _train_call(m, x, t, cots)
            return go

        before = len(seen)
        s_, f = _timed_pair(run("bf16x3"), run("fp32"))
        assert seen[before:] == ["bf16x3", "fp32"] * (WARM + TIMED)  # both sides took the fused call, each in its own mode
        qs, qf = _quantiles(s_), _quantiles(f)
        res[str(n)] = {"split_ms": qs, "fp32_ms": qf, "ratio": qs["median"] / qf["median"]}
        print(n, res[str(n)], flush=True)
    json.dump(res, open(os.path.join(out, "ptrain_blender.json" if BLENDER else "ptrain.json"), "w"), indent=1)


def pstep_model(out):
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    n, W, H = 240_000, 960, 540
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-4.5, is_blender=BLENDER)
    with torch.no_grad():
        for q in model.deform.parameters():
            q.mul_(0.3)
    model.step = 4000
    model = model.cuda().train()
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1
    cam = Camera(c2w[None, :3], 750.0, 750.0, W / 2, H / 2, W, H, times=torch.tensor([[0.4]]))
    gt = torch.rand(H, W, 3, device="cuda")
    _knob(True)
    _wgrad_knob(True)
    seen = _count_precisions()

    def step(value):
        def run():
            _precision_knob(value)
            model.zero_grad(set_to_none=True)
            model.get_loss_dict(model.get_outputs(cam), {"image": gt})["main_loss"].backward()
        return run

    warm, timed = 5, 30
    s_, f = _timed_pair(step("bf16x3"), step("fp32"), warm=warm, timed=timed)
    assert seen == ["bf16x3", "fp32"] * (warm + timed)
    res = {"n": n, "width": W, "height": H, "split_ms": _quantiles(s_), "fp32_ms": _quantiles(f)}
    print(res, flush=True)
    json.dump(res, open(os.path.join(out, "pmodel_blender.json" if BLENDER else "pmodel.json"), "w"), indent=1)


def pstep_error(out):
    import ctypes

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from mlp_inputs_common import float64_with_input_row, rows_clear_of_the_kink_aux  # (the references of the tests)
    from mlp_split_common import MARGIN, float64_acts
    from mlp_train_common import head_rows, heads_of

    from freegaussian_amd import _lib, ops
    from freegaussian_amd.utils import positional_encoding

    n = 33_000
    m = _module()
    g = torch.Generator().manual_seed(1)
    x, t = torch.rand(n, 3, generator=g) * 2 - 1, torch.rand(n, 1, generator=g)
    with torch.no_grad():
        aux = positional_encoding(t, m.t_multires)
        aux = m.timenet(aux) if BLENDER else aux
    gh = torch.randn(n, sum(head_rows(m)), generator=g)
    clear = rows_clear_of_the_kink_aux(m, x, aux, margin=MARGIN)
    ref = float64_with_input_row(m, x, aux, gh)
    ref["H"] = float64_acts(m, x, aux)
    md = copy.deepcopy(m).cuda().requires_grad_(False)
    xd, ad, gd = x.cuda(), aux.cuda(), gh.cuda()
    A, in_ch, lib = aux.shape[1], 63 + aux.shape[1], _lib.load()

    def arrays(precision):
        d, _, rows, keep = ops._mlp_desc("bench", xd, ad, md.linear, heads_of(md), _lib.MLP_PLAIN)
        d.precision = precision
        raw, enc, H = torch.empty(n, sum(rows), device="cuda"), torch.empty(n, _lib.mlp_enc_width(A), device="cuda"), torch.empty(8, n, 256, device="cuda")
        G, ge = torch.empty_like(H), torch.empty_like(enc)
        ws = torch.empty(int(lib.fg_mlp_bwd_inputs_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
        ops._call("fg_mlp_train_fwd", n, ctypes.addressof(d), raw.data_ptr(), enc.data_ptr(), H.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        ops._call("fg_mlp_bwd_inputs", n, ctypes.addressof(d), gd.data_ptr(), H.data_ptr(), G.data_ptr(), ge.data_ptr(), ws.data_ptr(),
                  ws.numel(), ops._stream())  # fmt: skip
        torch.cuda.synchronize()
        return {"heads": raw, "acts": H.transpose(0, 1), "g_pre": G.transpose(0, 1), "g_enc": ge[:, :in_ch]}

    def rel(a, b):
        return float((a.detach().double().cpu() - b).abs().max() / b.abs().max())

    want = {"heads": ref["raw"], "acts": ref["H"].transpose(0, 1), "g_pre": ref["G"].transpose(0, 1), "g_enc": ref["g_enc"]}
    got = {"split": arrays(_lib.MLP_BF16X3), "fp32": arrays(_lib.MLP_FP32)}
    res = {"rows": {"all rows": n, "rows clear of the ReLU kink": int(clear.sum())}, "margin": MARGIN, "arrays": {}}
    for label, rows in (("all rows", torch.ones(n, dtype=torch.bool)), ("rows clear of the ReLU kink", clear)):
        for k, w in want.items():
            res["arrays"][f"{k}, {label}"] = {side: rel(got[side][k][rows.cuda()], w[rows]) for side in got}
    # the masks: rows whose ReLU mask differs from float64's in any unit
    for side in got:
        flipped = ((got[side]["acts"].cpu() > 0) != (ref["H"].transpose(0, 1) > 0)).flatten(1).any(1)
        res.setdefault("rows with a flipped mask", {})[side] = {"all rows": int(flipped.sum()), "rows clear of the ReLU kink": int((flipped & clear).sum())}
    print(res, flush=True)
    json.dump(res, open(os.path.join(out, "perror_blender.json" if BLENDER else "perror.json"), "w"), indent=1)


def pstep_trace(out):
    m = _module().cuda()
    n = 240_000
    x = (torch.rand(n, 3) * 2 - 1).cuda()
    t = torch.full((1, 1), 0.4, device="cuda").expand(n, -1)
    cots = [torch.randn(n, *s).cuda() for s in ((4, 4), (4,), (3,))]
    _knob(True)
    _wgrad_knob(True)
    for value in ("bf16x3", "fp32"):
        _precision_knob(value)
        for _ in range(3):
            _train_call(m, x, t, cots)
    torch.cuda.synchronize()


def _gain(s, f):
    """The outcome rule: a gain = the split median below the fp32 median with p10 .. p90 that do not overlap."""
    if s["median"] < f["median"] and s["p90"] < f["p10"]:
        return "gain"
    if s["median"] > f["median"] and s["p10"] > f["p90"]:
        return "loss"
    return "no difference (the p10 .. p90 ranges overlap)"


def pstep_report(out, md):
    def load(name):
        path = os.path.join(out, name)
        return json.load(open(path)) if os.path.exists(path) else None

    def span(q, digits=3):
        return f"{q['median']:.{digits}f} ({q['p10']:.{digits}f} .. {q['p90']:.{digits}f})"

    L = ["# Split-bf16 (3-product) mode of the fused MLP kernels against their fp32 mode", "",
         "Written by `scripts/mlp_forward_bench.py --precision` and `scripts/mlp_train_bench.py --precision` on an MI355X.  The",
         "baseline is always the fp32 path of the same build; the two sides alternate call by call in one process per table,",
         f"{WARM} warm-up and {TIMED} timed calls each between device events (5 and 30 for the model step and the frame); median (p10 .. p90).",
         "Outcome rule: a gain = the split median below the fp32 median with p10 .. p90 ranges that do not overlap, at 240 000 rows,",
         "for (a) and for (b)."]  # fmt: skip
    verdicts = {}
    pt = load("ptime.json")
    if pt:
        L += ["", "## (a) `fg_mlp_fwd` alone (`ops.mlp_forward`: points, rotations, scalings; one time for all rows)", "",
              "| N | bf16x3 ms | fp32 ms | bf16x3 / fp32 | bf16x3 TFLOP/s | fp32 TFLOP/s | by the rule |", "|---|---|---|---|---|---|---|"]  # fmt: skip
        for n, r in pt["sizes"].items():
            L.append(f"| {int(n):,} | {span(r['split_ms'])} | {span(r['fp32_ms'])} | {r['ratio']:.2f} | {r['split_tflops']:.1f} | "
                     f"{r['fp32_tflops']:.1f} | {_gain(r['split_ms'], r['fp32_ms'])} |")  # fmt: skip
        verdicts["(a)"] = _gain(pt["sizes"]["240000"]["split_ms"], pt["sizes"]["240000"]["fp32_ms"])
    for name, title in (("ptrain.json", "deformation net, `FG_FUSED_MLP_TRAIN=1`"), ("ptrain_blender.json", "blender net, `FG_FUSED_MLP_TRAIN=2`")):
        tr = load(name)
        if tr:
            L += ["", f"## (b) The whole `ops.mlp_train` forward + backward, `FG_FUSED_MLP_WGRAD=1`: {title}", "",
                  "| N | bf16x3 ms | fp32 ms | bf16x3 / fp32 | by the rule |", "|---|---|---|---|---|"]  # fmt: skip
            for n in (str(v) for v in SIZES):
                if n in tr:
                    L.append(f"| {int(n):,} | {span(tr[n]['split_ms'])} | {span(tr[n]['fp32_ms'])} | {tr[n]['ratio']:.2f} | {_gain(tr[n]['split_ms'], tr[n]['fp32_ms'])} |")
            verdicts[f"(b) {title.split(',')[0]}"] = _gain(tr["240000"]["split_ms"], tr["240000"]["fp32_ms"])
    rows = [(load("pmodel.json"), "model training step, deformation net"), (load("pmodel_blender.json"), "model training step, blender net")]
    if any(r for r, _ in rows):
        L += ["", "## (c) One model training step at 240 000 Gaussians, 960 x 540, behind `warm_up` (`FG_FUSED_MLP_TRAIN` and `_WGRAD` set)", "",
              "| model | bf16x3 ms | fp32 ms | bf16x3 / fp32 |", "|---|---|---|---|"]  # fmt: skip
        L += [f"| {title} | {span(r['split_ms'], 2)} | {span(r['fp32_ms'], 2)} | {r['split_ms']['median'] / r['fp32_ms']['median']:.2f} |" for r, title in rows if r]
    fr = load("pframe.json")
    if fr:
        L += ["", f"## (d) `get_outputs_for_camera` per frame ({fr['source']}: {fr['n']:,} Gaussians, {fr['width']} x {fr['height']}, eval)", "",
              "| bf16x3 ms | fp32 ms | bf16x3 / fp32 |", "|---|---|---|",
              f"| {span(fr['split_ms'], 2)} | {span(fr['fp32_ms'], 2)} | {fr['split_ms']['median'] / fr['fp32_ms']['median']:.2f} |"]  # fmt: skip
    for sub, title in (("ptrace_fwd", "three `ops.mlp_forward` calls of either precision"), ("ptrace", "three training calls of either precision, `FG_FUSED_MLP_WGRAD=1`")):
        stats = sorted(glob.glob(os.path.join(out, sub, "**", "*kernel_stats.csv"), recursive=True))
        if stats:
            L += ["", f"## (e) Kernels of {title} at N = 240 000 (`rocprofv3 --kernel-trace --stats`, a run of its own)", "",
                  "| kernel | calls | average us | share % |", "|---|---|---|---|"]  # fmt: skip
            for r in list(csv.DictReader(open(stats[0])))[:14]:
                L.append(f"| `{r['Name'][:90]}` | {r['Calls']} | {float(r['AverageNs']) / 1e3:.1f} | {float(r['Percentage']):.1f} |")
    for name, title in (("perror.json", "deformation net"), ("perror_blender.json", "blender net")):
        er = load(name)
        if er:
            L += ["", f"## (f) Error against float64 at N = 33 000 ({title}, default init, a time per row; max |a - b| / max |b|; the bar is 1e-4)", "",
                  f"Rows clear of the ReLU's kink by {er['margin']:g} of the layer's largest pre-activation: {er['rows']['rows clear of the ReLU kink']:,} of "
                  f"{er['rows']['all rows']:,}.  Rows with a ReLU mask other than float64's in any unit -- bf16x3: {er['rows with a flipped mask']['split']['all rows']} of all "
                  f"rows, {er['rows with a flipped mask']['split']['rows clear of the ReLU kink']} of the clear ones; fp32: {er['rows with a flipped mask']['fp32']['all rows']} and "
                  f"{er['rows with a flipped mask']['fp32']['rows clear of the ReLU kink']}.  A row with a flipped mask has another gradient, whatever computed it.", "",
                  "| array, rows | bf16x3 | fp32 |", "|---|---|---|"]  # fmt: skip
            L += [f"| {k} | {v['split']:.2e} | {v['fp32']:.2e} |" for k, v in er["arrays"].items()]
    if verdicts:
        L += ["", "## Outcome by the rule (240 000 rows)", ""] + [f"- {k}: **{v}**" for k, v in verdicts.items()]
    # (hand-written sections of the file -- everything from the first "## Notes" heading on -- are kept)
    if os.path.exists(md) and "\n## Notes" in open(md).read():
        L += ["", "## Notes" + open(md).read().split("\n## Notes", 1)[1].rstrip()]
    open(md, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


# ---- --wgrad-precision: the split-bf16 mode of the fused parameter-gradient products ---------------------------------------
WGRAD_PRECISION_KNOB = "FG_FUSED_MLP_WGRAD_PRECISION"


def _wgrad_precision_knob(value):
    if value == "fp32":
        os.environ.pop(WGRAD_PRECISION_KNOB, None)
    else:
        os.environ[WGRAD_PRECISION_KNOB] = value


def sstep_call(out):
    """``ops.mlp_param_grads`` alone, precision="bf16x3" against "fp32" of the same build, alternating call by call."""
    from freegaussian_amd import ops

    res = {}
    for A in (21, 30):
        for n in SIZES:
            enc, H, G, gh = _wgrad_arrays(n, A)
            s_, f = _timed_pair(lambda: ops.mlp_param_grads(enc, H, G, gh, A, WGRAD_ROWS, precision="bf16x3"),
                                lambda: ops.mlp_param_grads(enc, H, G, gh, A, WGRAD_ROWS))  # fmt: skip
            qs, qf = _quantiles(s_), _quantiles(f)
            fl = (WGRAD_FLOP_PER_ROW + 4 * 256 * (63 + A)) * n
            res[f"{A},{n}"] = {"aux_width": A, "n": n, "split_ms": qs, "fp32_ms": qf, "ratio": qs["median"] / qf["median"],
                               "split_tflops": fl / qs["median"] / 1e9, "fp32_tflops": fl / qf["median"] / 1e9,
                               "operand_gb_per_s": 16384.0 * n / qs["median"] / 1e6}  # fmt: skip
            print(res[f"{A},{n}"], flush=True)
            del enc, H, G, gh
            torch.cuda.empty_cache()
    json.dump(res, open(os.path.join(out, "scall.json"), "w"), indent=1)


def sstep_error(out):
    from freegaussian_amd import deform, ops

    n, res = 33_000, {}

    def rel(a, b):
        return float((a.double().cpu() - b).abs().max() / b.abs().max())

    for A in (21, 30):
        enc, H, G, gh = _wgrad_arrays(n, A)
        want = deform.mlp_param_grads(enc[:, : 63 + A].double().cpu(), H.double().cpu(), G.double().cpu(), gh.double().cpu(), WGRAD_ROWS)
        for name in ("bf16x3", "fp32"):
            got = ops.mlp_param_grads(enc, H, G, gh, A, WGRAD_ROWS, precision=name)
            for kind, gs, ws in zip(("trunk weights", "trunk biases", "head weights", "head biases"), got, want):
                res.setdefault(f"{kind}, aux width {A}", {})[name] = max(rel(g, w) for g, w in zip(gs, ws))
    print(res, flush=True)
    json.dump(res, open(os.path.join(out, "serror.json"), "w"), indent=1)


_COMBOS = [(chain, wgrad) for chain in ("fp32", "bf16x3") for wgrad in ("fp32", "bf16x3")]


def _timed_combos(run, warm=WARM, timed=TIMED):
    """The four (chain precision, weight-gradient precision) settings alternating call by call: name -> ms list."""
    ms = {c: [] for c in _COMBOS}
    for i in range(warm + timed):
        for c in _COMBOS:
            _precision_knob(c[0])
            _wgrad_precision_knob(c[1])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            if i >= warm:
                ms[c].append(a.elapsed_time(b))
    return {f"{c[0]},{c[1]}": _quantiles(v) for c, v in ms.items()}


def _count_wgrad_precisions():
    from freegaussian_amd import ops

    seen = []
    real = ops.mlp_train
    ops.mlp_train = lambda *a, **k: seen.append((k.get("precision", "fp32"), k.get("param_grads_precision", "fp32"))) or real(*a, **k)
    return seen


def sstep_train(out):
    m = _module().cuda()
    _knob(True)
    _wgrad_knob(True)
    seen, res = _count_wgrad_precisions(), {}
    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        x = (torch.rand(n, 3, generator=g) * 2 - 1).cuda()
        t = torch.full((1, 1), 0.4, device="cuda").expand(n, -1)
        cots = [torch.randn(n, *s, generator=g).cuda() for s in ((4, 4), (4,), (3,))]
        before = len(seen)
        res[str(n)] = _timed_combos(lambda: _train_call(m, x, t, cots))
        assert seen[before:] == _COMBOS * (WARM + TIMED)  # every side took the fused call, each in its own setting
        print(n, res[str(n)], flush=True)
    json.dump(res, open(os.path.join(out, "strain_blender.json" if BLENDER else "strain.json"), "w"), indent=1)


def sstep_model(out):
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    n, W, H = 240_000, 960, 540
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-4.5, is_blender=BLENDER)
    with torch.no_grad():
        for q in model.deform.parameters():
            q.mul_(0.3)
    model.step = 4000
    model = model.cuda().train()
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1
    cam = Camera(c2w[None, :3], 750.0, 750.0, W / 2, H / 2, W, H, times=torch.tensor([[0.4]]))
    gt = torch.rand(H, W, 3, device="cuda")
    _knob(True)
    _wgrad_knob(True)
    seen = _count_wgrad_precisions()

    def step():
        model.zero_grad(set_to_none=True)
        model.get_loss_dict(model.get_outputs(cam), {"image": gt})["main_loss"].backward()

    warm, timed = 5, 30
    res = {"n": n, "width": W, "height": H, "ms": _timed_combos(step, warm=warm, timed=timed)}
    assert seen == _COMBOS * (warm + timed)
    print(res, flush=True)
    json.dump(res, open(os.path.join(out, "smodel_blender.json" if BLENDER else "smodel.json"), "w"), indent=1)


def sstep_trace(out):
    """Three training calls of each of the four settings at N = 240 000, then three calls alone: for ``rocprofv3``."""
    from freegaussian_amd import ops

    m = _module().cuda()
    n = 240_000
    x = (torch.rand(n, 3) * 2 - 1).cuda()
    t = torch.full((1, 1), 0.4, device="cuda").expand(n, -1)
    cots = [torch.randn(n, *s).cuda() for s in ((4, 4), (4,), (3,))]
    _knob(True)
    _wgrad_knob(True)
    for chain, wgrad in _COMBOS:
        _precision_knob(chain)
        _wgrad_precision_knob(wgrad)
        for _ in range(3):
            _train_call(m, x, t, cots)
    torch.cuda.synchronize()


def sstep_counters(out):
    """Three calls of the split products alone at N = 240 000: for a ``rocprofv3 --pmc`` run of its own."""
    from freegaussian_amd import ops

    enc, H, G, gh = _wgrad_arrays(240_000, 21)
    for _ in range(3):
        ops.mlp_param_grads(enc, H, G, gh, 21, WGRAD_ROWS, precision="bf16x3")
    torch.cuda.synchronize()


def sstep_report(out, md):
    def load(name):
        path = os.path.join(out, name)
        return json.load(open(path)) if os.path.exists(path) else None

    L = ["# Split-bf16 (3-product) mode of the fused parameter-gradient products against their fp32 mode", "",
         "Written by `scripts/mlp_train_bench.py --wgrad-precision` on an MI355X.  The baseline is the fp32 entry point of the same",
         "build; the sides alternate call by call in one process per table, "
         f"{WARM} warm-up and {TIMED} timed calls each between device events (5 and 30 for the model step); median (p10 .. p90).",
         "Outcome rule: a gain = the split median below the fp32 median with p10 .. p90 ranges that do not overlap, at 240 000 rows."]  # fmt: skip
    verdicts = {}
    sc = load("scall.json")
    if sc:
        L += ["", "## (a) `fg_mlp_param_grads_p` alone (`ops.mlp_param_grads(precision=...)`, the tests' random arrays)", "",
              "| aux width | N | bf16x3 ms | fp32 ms | bf16x3 / fp32 | bf16x3 TFLOP/s | fp32 TFLOP/s | operand bytes / bf16x3 time, GB/s | by the rule |",
              "|---|---|---|---|---|---|---|---|---|"]  # fmt: skip
        for r in sc.values():
            L.append(f"| {r['aux_width']} | {r['n']:,} | {_ms(r['split_ms'])} | {_ms(r['fp32_ms'])} | {r['ratio']:.2f} | {r['split_tflops']:.1f} | "
                     f"{r['fp32_tflops']:.1f} | {r['operand_gb_per_s']:.0f} | {_gain(r['split_ms'], r['fp32_ms'])} |")  # fmt: skip
        verdicts["(a) the call alone, aux width 21"] = _gain(sc["21,240000"]["split_ms"], sc["21,240000"]["fp32_ms"])
    for name, title in (("strain.json", "deformation net, `FG_FUSED_MLP_TRAIN=1`"), ("strain_blender.json", "blender net, `FG_FUSED_MLP_TRAIN=2`")):
        tr = load(name)
        if tr:
            L += ["", f"## (b) The whole `ops.mlp_train` forward + backward, `FG_FUSED_MLP_WGRAD=1`: {title}", "",
                  "Columns: `FG_FUSED_MLP_PRECISION`, `FG_FUSED_MLP_WGRAD_PRECISION`.", "",
                  "| N | fp32, fp32 ms | fp32, bf16x3 ms | ratio | bf16x3, fp32 ms | bf16x3, bf16x3 ms | ratio | by the rule (chain fp32 / bf16x3) |",
                  "|---|---|---|---|---|---|---|---|"]  # fmt: skip
            for n in (str(v) for v in SIZES):
                if n in tr:
                    r = tr[n]
                    L.append(f"| {int(n):,} | {_ms(r['fp32,fp32'])} | {_ms(r['fp32,bf16x3'])} | {r['fp32,bf16x3']['median'] / r['fp32,fp32']['median']:.2f} | "
                             f"{_ms(r['bf16x3,fp32'])} | {_ms(r['bf16x3,bf16x3'])} | {r['bf16x3,bf16x3']['median'] / r['bf16x3,fp32']['median']:.2f} | "
                             f"{_gain(r['fp32,bf16x3'], r['fp32,fp32'])} / {_gain(r['bf16x3,bf16x3'], r['bf16x3,fp32'])} |")  # fmt: skip
            r = tr["240000"]
            verdicts[f"(b) {title.split(',')[0]}, chain fp32"] = _gain(r["fp32,bf16x3"], r["fp32,fp32"])
            verdicts[f"(b) {title.split(',')[0]}, chain bf16x3"] = _gain(r["bf16x3,bf16x3"], r["bf16x3,fp32"])
    rows = [(load("smodel.json"), "deformation net"), (load("smodel_blender.json"), "blender net")]
    if any(r for r, _ in rows):
        L += ["", "## (c) One model training step at 240 000 Gaussians, 960 x 540, behind `warm_up` (`FG_FUSED_MLP_TRAIN` and `_WGRAD` set)", "",
              "| model | fp32, fp32 ms | fp32, bf16x3 ms | bf16x3, fp32 ms | bf16x3, bf16x3 ms |", "|---|---|---|---|---|"]  # fmt: skip
        for r, title in rows:
            if r:
                q = r["ms"]
                L.append(f"| {title} | " + " | ".join(f"{q[k]['median']:.2f} ({q[k]['p10']:.2f} .. {q[k]['p90']:.2f})" for k in ("fp32,fp32", "fp32,bf16x3", "bf16x3,fp32", "bf16x3,bf16x3")) + " |")
    stats = sorted(glob.glob(os.path.join(out, "strace", "**", "*kernel_stats.csv"), recursive=True))
    if stats:
        L += ["", "## (d) Kernels of three training calls of each of the four settings at N = 240 000 (`rocprofv3 --kernel-trace --stats`, a run of its own)", "",
              "| kernel | calls | average us | share % |", "|---|---|---|---|"]  # fmt: skip
        for r in list(csv.DictReader(open(stats[0])))[:16]:
            L.append(f"| `{r['Name'][:90]}` | {r['Calls']} | {float(r['AverageNs']) / 1e3:.1f} | {float(r['Percentage']):.1f} |")
    er = load("serror.json")
    if er:
        L += ["", "## (e) Error against float64 of the same arrays at N = 33 000 (max |a - b| / max |b|; the bar is 1e-4)", "",
              "| gradients | bf16x3 | fp32 |", "|---|---|---|"]  # fmt: skip
        L += [f"| {k} | {v['bf16x3']:.2e} | {v['fp32']:.2e} |" for k, v in er.items()]
    if verdicts:
        L += ["", "## Outcome by the rule (240 000 rows)", ""] + [f"- {k}: **{v}**" for k, v in verdicts.items()]
    # (hand-written sections of the file -- everything from the first "## Notes" heading on -- are kept)
    if os.path.exists(md) and "\n## Notes" in open(md).read():
        L += ["", "## Notes" + open(md).read().split("\n## Notes", 1)[1].rstrip()]
    open(md, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["time", "error", "model", "trace", "kernel", "report", "wcall", "werror", "wtrain", "wmodel",
                                       "wtrace", "wreport", "ccall", "ctrain", "cmodel", "cmem", "ctrace", "creport", "ptrain", "pmodel", "perror",
                                       "ptrace", "preport", "scall", "serror", "strain", "smodel", "strace", "scounters", "sreport"])  # fmt: skip
    ap.add_argument("--wgrad-precision", action="store_true",
                    help="the split-bf16 mode of the parameter-gradient products, FG_FUSED_MLP_WGRAD_PRECISION, against fp32 (profiles/mlp_wgrad_split.md)")
    ap.add_argument("--precision", action="store_true", help="the split-bf16 mode, FG_FUSED_MLP_PRECISION, against fp32 (profiles/mlp_split_bf16.md)")
    ap.add_argument("--chunked", action="store_true", help="the backward in row chunks, FG_FUSED_MLP_CHUNKED (profiles/mlp_chunked_bwd.md)")
    ap.add_argument("--only", default=None, help="with --chunked: a comma-separated subset of its steps (ccall,base,ctrain,cmodel,cmem,ctrace,creport)")
    ap.add_argument("--parent-lib", default=None, help="with --chunked: the parent commit's build of the library, for the side-by-side table")
    ap.add_argument("--lib", default=None, help="with --step: load this build of the library in place of the package's")
    ap.add_argument("--wgrad", action="store_true", help="the fused parameter-gradient call, FG_FUSED_MLP_WGRAD (profiles/mlp_wgrad.md)")
    ap.add_argument("--blender", action="store_true", help="the blender net under FG_FUSED_MLP_TRAIN=2 (profiles/mlp_train_inputs.md)")
    ap.add_argument("--trace", action="store_true", help="also one rocprofv3 --kernel-trace --stats run of the fused calls")
    ap.add_argument("--parity", default=None, help="FG_PARITY_REPORT file to quote: of tests/test_mlp_train_gpu.py, with --blender of tests/test_mlp_inputs_gpu.py")
    ap.add_argument("--out", default=None, help="default: results/mlp_train, results/mlp_train_inputs with --blender")
    ap.add_argument("--md", default=None, help="default: profiles/mlp_train.md, profiles/mlp_train_inputs.md with --blender")
    a = ap.parse_args()
    global BLENDER
    BLENDER = a.blender
    name = "mlp_train_inputs" if BLENDER else "mlp_train"
    if a.wgrad or (a.step or "").startswith("w"):
        name = "mlp_wgrad"
    if a.chunked or (a.step or "").startswith("c"):
        name = "mlp_chunked_bwd"
    if a.precision or (a.step or "").startswith("p"):
        name = "mlp_split"
    if a.wgrad_precision or (a.step or "").startswith("s"):
        name = "mlp_wgrad_split"
    if a.lib:
        _use_library(a.lib)
    a.out = a.out or os.path.join(ROOT, "results", name)
    a.md = a.md or os.path.join(ROOT, "profiles", "mlp_split_bf16.md" if name == "mlp_split" else name + ".md")
    os.makedirs(a.out, exist_ok=True)
    if a.step:
        if a.step == "sreport":
            return sstep_report(a.out, a.md)
        if a.step.startswith("s"):
            return {"scall": sstep_call, "serror": sstep_error, "strain": sstep_train, "smodel": sstep_model, "strace": sstep_trace,
                    "scounters": sstep_counters}[a.step](a.out)  # fmt: skip
        if a.step == "preport":
            return pstep_report(a.out, a.md)
        if a.step.startswith("p"):
            return {"ptrain": pstep_train, "pmodel": pstep_model, "perror": pstep_error, "ptrace": pstep_trace}[a.step](a.out)
        if a.step == "report":
            return step_report(a.out, a.md, a.parity)
        if a.step == "wreport":
            return wstep_report(a.out, a.md, a.parity)
        if a.step == "creport":
            return cstep_report(a.out, a.md, a.parity)
        if a.step.startswith("c"):
            return {"ccall": cstep_call, "ctrain": cstep_train, "cmodel": cstep_model, "cmem": cstep_mem, "ctrace": cstep_trace}[a.step](a.out)
        if a.step.startswith("w"):
            return {"wcall": wstep_call, "werror": wstep_error, "wtrain": wstep_train, "wmodel": wstep_model, "wtrace": wstep_trace}[a.step](a.out)
        return {"time": step_time, "error": step_error, "model": step_model, "trace": step_trace, "kernel": step_kernel}[a.step](a.out)
    me = [sys.executable, os.path.abspath(__file__), "--out", a.out, "--md", a.md] + (["--blender"] if BLENDER else []) + ["--step"]
    steps = [(300, me + ["time"]), (180, me + ["error"]), (240, me + ["model"])]
    if BLENDER:
        steps = [(300, me + ["time"]), (120, me + ["kernel"]), (240, me + ["model"])]
    if a.wgrad:
        me = [sys.executable, os.path.abspath(__file__), "--out", a.out, "--md", a.md, "--step"]
        steps = [(240, me + ["wcall"]), (120, me + ["werror"]), (180, me + ["wtrain"]), (180, me + ["wtrain", "--blender"]),
                 (240, me + ["wmodel"]), (240, me + ["wmodel", "--blender"])]  # fmt: skip
        if a.trace:
            steps.append((180, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(a.out, "wtrace"),
                                "-o", "mlp", "--"] + me + ["wtrace"]))  # fmt: skip
        steps.append((60, me + ["wreport"] + (["--parity", a.parity] if a.parity else [])))
    elif a.trace:
        steps.append((180, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(a.out, "trace"),
                            "-o", "mlp", "--"] + me + ["trace"]))  # fmt: skip
    if a.chunked:
        me = [sys.executable, os.path.abspath(__file__), "--md", a.md]
        here = me + ["--out", a.out, "--step"]
        groups = {"ccall": [(300, here + ["ccall"])], "ctrain": [(180, here + ["ctrain"]), (180, here + ["ctrain", "--blender"])],
                  "cmodel": [(240, here + ["cmodel"])], "cmem": [(180, here + ["cmem"])], "base": [], "ctrace": [],
                  "creport": [(60, here + ["creport"] + (["--parity", a.parity] if a.parity else []))]}  # fmt: skip
        if a.parent_lib:
            from freegaussian_amd import _lib

            for tag, lib in (("this", _lib.LIB_PATH), ("parent", os.path.abspath(a.parent_lib))):
                base = me + ["--out", os.path.join(a.out, f"base_{tag}"), "--lib", lib, "--step"]
                os.makedirs(os.path.join(a.out, f"base_{tag}"), exist_ok=True)
                groups["base"] += [(300, base + ["wcall"]), (120, base + ["kernel", "--blender"])]
        if a.trace:
            groups["ctrace"] = [(180, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(a.out, "ctrace"),
                                       "-o", "mlp", "--"] + here + ["ctrace"])]  # fmt: skip
        order = ("ccall", "base", "ctrain", "cmodel", "cmem", "ctrace", "creport")
        steps = [s for name in order if not a.only or name in a.only.split(",") for s in groups[name]]
    elif not a.wgrad:
        steps.append((60, me + ["report"] + (["--parity", a.parity] if a.parity else [])))
    if a.precision:
        me = [sys.executable, os.path.abspath(__file__), "--out", a.out, "--md", a.md, "--step"]
        steps = [(240, me + ["ptrain"]), (240, me + ["ptrain", "--blender"]), (240, me + ["pmodel"]), (240, me + ["pmodel", "--blender"]),
                 (300, me + ["perror"])]  # fmt: skip
        if a.trace:
            steps.append((180, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(a.out, "ptrace"),
                                "-o", "mlp", "--"] + me + ["ptrace"]))  # fmt: skip
        steps.append((60, me + ["preport"]))
    if a.wgrad_precision:
        me = [sys.executable, os.path.abspath(__file__), "--out", a.out, "--md", a.md, "--step"]
        steps = [(300, me + ["scall"]), (120, me + ["serror"]), (300, me + ["strain"]), (300, me + ["strain", "--blender"]), (300, me + ["smodel"])]
        if a.trace:  # the kernel trace, then the LDS counters: a run each, the counters with no tracing beside them
            steps.append((180, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(a.out, "strace"),
                                "-o", "mlp", "--"] + me + ["strace"]))  # fmt: skip
            steps.append((180, ["rocprofv3", "--pmc", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "--output-format", "csv", "-d",
                                os.path.join(a.out, "scounters"), "-o", "mlp", "--"] + me + ["scounters"]))  # fmt: skip
        steps.append((60, me + ["sreport"]))
    for limit, cmd in steps:  # chained like &&: the first failure ends the job
        rc = subprocess.call(["timeout", "-k", "10", str(limit)] + cmd)
        if rc != 0:
            sys.exit(f"step failed ({rc}): {' '.join(cmd[-2:])}")


if __name__ == "__main__":
    main()
