"""The Adam kernels (csrc/adam.hip) in isolation, one update at a time, every element of p', m' and v' compared with the
float64 restatement of tests/adam_restatement.py on its regime tensor:

    |x_hip - x64| / denominator  <=  F * E32(regime, output)

E32 over the regime's elements of the same tensor.  tests/parity_common.py has the protocol (E32, the floor, F); F, FLOOR and
the three denominators are adam_restatement's, the recorded table is in profiles/loss_adam_flow_parity.md.

    FusedAdam.step()    -> fg_adam_step_multi, at sizes around the float4 boundary and at and past the 2048-workgroup cap of
                        one tensor (2 097 152 floats: beyond it the grid-stride loop runs, and the tail under a capped grid),
                        crossed with step in {1, 2, 1000, 30000} and lr in {1.6e-4, 1.6e-6}
    step_all            batches of 16, 17 and 33 single-tensor optimizers in one call: zero-sized tensors, tensors without
                        a gradient, a learning rate per optimizer, two different step counts in one launch
    fg_adam_step        the single-tensor entry through ``_lib``, past its own 8192-workgroup cap; bit for bit
                        fg_adam_step_multi on equal inputs, as include/fgraster.h promises

``PYTHONPATH=. python tests/test_adam_elements_gpu.py REPORT.jsonl`` turns the records of a run under FG_PARITY_REPORT into the table of
profiles/loss_adam_flow_parity.md.
"""
import ctypes
import functools
import sys

import pytest
import torch

import adam_restatement as A
import parity_common as P
from freegaussian_amd import _lib
from freegaussian_amd.optim import FusedAdam, _AdamTensor, step_all
from parity_common import need_gpu  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAP = 2048 * 256 * 4  # floats one tensor's 2048 workgroups cover in one pass of fg_adam_step_multi
SIZES = [1, 2, 3, 4, 5, 1023, 1024 * 4 + 3, CAP - 1, CAP, CAP + 5, 3 * CAP + 7]


@functools.lru_cache(maxsize=2)
def _tensor(n, seed=0):
    return A.regime_tensor(n, seed)


def _check(tag, pre, regime, lr, step, out, failures):
    """One tensor's three outputs against float64, per element.  Every ratio is recorded before anything is asserted."""
    p, g, m, v = pre
    out64, den, e32 = A.reference(p, g, m, v, regime, lr, step)
    masks = P.masks_of_index(regime, A.REGIMES)
    for k, x, x64 in zip(A.OUTPUTS, out, out64):
        P.check(f"{tag}|{k}|{{regime}}", masks, P.distance(x.reshape(-1), x64, den[k]), e32[k], A.F, failures)
    # fresh state, zero gradient: exactly p, m' = v' = 0
    z = regime == A.REGIMES.index("fresh_zero_grad")
    if not (torch.equal(out[0].cpu().reshape(-1)[z], p[z]) and bool((out[1].cpu().reshape(-1)[z] == 0).all())
            and bool((out[2].cpu().reshape(-1)[z] == 0).all())):  # fmt: skip
        failures.append(f"{tag}: a fresh element with a zero gradient moved")


def _optimizer(p, g, m, v, lr, step):
    """A FusedAdam about to take update number ``step`` of one parameter, moments as given."""
    x = p.clone().to(DEV).requires_grad_(True)
    x.grad = g.clone().to(DEV)
    opt = FusedAdam([x], lr=lr, eps=A.EPS)
    opt.state[x] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone().to(DEV), exp_avg_sq=v.clone().to(DEV))
    return opt, x


# (a size's cases are neighbours: its regime tensor is made once)
@pytest.mark.parametrize("n,step,lr", [(n, t, lr) for n in SIZES for t in A.STEPS for lr in A.LRS])
def test_every_element_through_step(n, step, lr):
    p, g, m, v, regime = _tensor(n)
    opt, x = _optimizer(p, g, m, v, lr, step)
    grad_before = x.grad.clone()
    opt.step()
    torch.cuda.synchronize()
    st = opt.state[x]
    assert float(st["step"]) == step and torch.equal(x.grad, grad_before)
    failures = []
    _check(f"step-n{n}-t{step}-lr{lr:g}", (p, g, m, v), regime, lr, step, (x.detach(), st["exp_avg"], st["exp_avg_sq"]), failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("count", [16, 17, 33])
def test_every_element_through_step_all(count):
    """One ``step_all`` over ``count`` single-tensor optimizers (one launch for every 16 tensors): sizes cycling through
    1, 3, 64 * 3, 1000 and 0 (``torch.empty(0, 3)`` with an empty gradient), every seventh parameter without a gradient, a
    learning rate per optimizer, and every other optimizer stepped once before, so that one launch carries two step counts."""
    shapes = [(1,), (3,), (64, 3), (1000,), (0, 3)]
    opts, xs, lrs = [], [], []
    for i in range(count):
        shape = shapes[i % len(shapes)]
        n = shape[0] * (shape[1] if len(shape) > 1 else 1)
        p, g, _, _, _ = A.regime_tensor(n, seed=100 + i)
        x = p.reshape(shape).clone().to(DEV).requires_grad_(True)
        lr = 1.6e-4 * (1 + i)
        opt = FusedAdam([x], lr=lr, eps=A.EPS)
        if i % 2 == 1:  # stepped once before, on its own
            x.grad = (0.5 * g).reshape(shape).to(DEV)
            opt.step()
        x.grad = None if i % 7 == 3 else g.reshape(shape).clone().to(DEV)
        opts.append(opt), xs.append(x), lrs.append(lr)
    torch.cuda.synchronize()
    pre = []
    for opt, x in zip(opts, xs):
        st = opt.state[x]
        zeros = torch.zeros(x.numel())
        pre.append((x.detach().cpu().reshape(-1).clone(), None if x.grad is None else x.grad.cpu().reshape(-1).clone(),
                    st["exp_avg"].cpu().reshape(-1).clone() if st else zeros, st["exp_avg_sq"].cpu().reshape(-1).clone() if st else zeros,
                    float(st["step"]) if st else 0.0))  # fmt: skip
    step_all(opts)
    torch.cuda.synchronize()
    failures = []
    for i, (opt, x, lr, (p, g, m, v, t)) in enumerate(zip(opts, xs, lrs, pre)):
        st = opt.state[x]
        if g is None:  # untouched: bit-identical, the step counter where it was
            same = torch.equal(x.detach().cpu().reshape(-1), p) and (
                (float(st["step"]) == t and torch.equal(st["exp_avg"].cpu().reshape(-1), m)
                 and torch.equal(st["exp_avg_sq"].cpu().reshape(-1), v)) if st else t == 0.0)  # fmt: skip
            if not same:
                failures.append(f"step_all-{count}-i{i}: a tensor without a gradient was touched")
            continue
        if not (float(st["step"]) == t + 1 == (2 if i % 2 == 1 else 1)):
            failures.append(f"step_all-{count}-i{i}: step is {float(st['step'])} after {t}")
        if not (st["exp_avg"].shape == x.shape and st["exp_avg_sq"].shape == x.shape):
            failures.append(f"step_all-{count}-i{i}: the moments' shapes are not the parameter's")
            continue
        regime = torch.arange(p.numel()) % len(A.REGIMES)
        if i % 2 == 1:  # (after a step the fresh elements are warm; those with a zero gradient still have m = v = 0)
            regime = torch.where(regime == A.REGIMES.index("fresh"), A.REGIMES.index("warm"), regime)
        if p.numel():
            _check(f"step_all-{count}-i{i}", (p, g, m, v), regime, lr, int(t) + 1, (x.detach(), st["exp_avg"], st["exp_avg_sq"]), failures)
    assert not failures, "\n".join(failures)


def _direct(name, arrays, lr, step):
    p, g, m, v = arrays
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    if name == "fg_adam_step":
        rc = lib.fg_adam_step(p.numel(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), lr, A.BETA1, A.BETA2, A.EPS, step, stream)
    else:
        t = (_AdamTensor * 1)()
        t[0].param, t[0].grad, t[0].exp_avg, t[0].exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
        t[0].n, t[0].lr, t[0].beta1, t[0].beta2, t[0].eps, t[0].step = p.numel(), lr, A.BETA1, A.BETA2, A.EPS, step
        rc = lib.fg_adam_step_multi(1, ctypes.cast(t, ctypes.c_void_p), stream)
    _lib.check(rc, name)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [100_003, 8192 * 256 * 4 + 1027])
def test_single_tensor_entry_point(n):
    """``fg_adam_step`` through ``_lib``: every element against float64, and bit for bit ``fg_adam_step_multi`` on equal
    inputs.  The larger size is past its own 8192-workgroup cap (8 388 608 floats in one pass)."""
    p, g, m, v, regime = _tensor(n, 1)
    lr, step = 1.6e-4, 2
    one = [t.clone().to(DEV) for t in (p, g, m, v)]
    multi = [t.clone().to(DEV) for t in (p, g, m, v)]
    _direct("fg_adam_step", one, lr, step)
    _direct("fg_adam_step_multi", multi, lr, step)
    assert torch.equal(one[1].cpu(), g)
    failures = []
    _check(f"fg_adam_step-n{n}", (p, g, m, v), regime, lr, step, (one[0], one[2], one[3]), failures)
    for name, a, b in zip(("p", "g", "m", "v"), one, multi):
        assert torch.equal(a, b), f"{name}: fg_adam_step and fg_adam_step_multi differ"
    assert not failures, "\n".join(failures)


def _report(path):
    """Markdown of a run's records (FG_PARITY_REPORT): per output and regime, the worst HIP ratio over all cases and (the
    smallest E32 met); then the worst ratio per output of every size (over its steps and learning rates) and of every
    ``step_all`` batch (over its tensors)."""
    ratio, e32, per_group = {}, {}, {}
    cell_ratio, cell_e32 = P.read_records(path, "test_adam_elements_gpu")
    for (tag, k, name), value in cell_ratio.items():
        ratio[(k, name)] = max(ratio.get((k, name), 0.0), value)
        parts = tag.split("-")  # step-n5-t1-lr..., step_all-16-i3, fg_adam_step-n100003
        group = f"{parts[0]} {parts[1].lstrip('n')}"
        per_group[(group, k)] = max(per_group.get((group, k), 0.0), value)
    for (tag, k, name), value in cell_e32.items():
        e32[(k, name)] = min(e32.get((k, name), float("inf")), value)
    worst = max(ratio, key=ratio.get)
    print(f"Adam: worst ratio {ratio[worst]:.2f} at {worst[0]}', {worst[1]}; {len(dict.fromkeys(g for g, _ in per_group))} sizes and batches.\n")
    print("| output | " + " | ".join(A.REGIMES) + " |\n|---|" + "---|" * len(A.REGIMES))
    for k in A.OUTPUTS:
        print(f"| {k}' | " + " | ".join(f"{ratio[(k, r)]:.2f} ({e32[(k, r)]:.1e})" if (k, r) in ratio else "" for r in A.REGIMES) + " |")
    print("\n| entry, size or batch | p' | m' | v' |\n|---|---|---|---|")
    for group in dict.fromkeys(g for g, _ in per_group):
        print(f"| {group} | " + " | ".join(f"{per_group.get((group, k), 0.0):.2f}" for k in A.OUTPUTS) + " |")


if __name__ == "__main__":
    _report(sys.argv[1])
