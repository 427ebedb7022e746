"""Plumbing shared by the tests/test_mlp_*.py files: the two structs of the fused MLP's C ABI filled in, guard-band
allocations, gradient snapshots, spies and stand-ins.  No float64 restatement lives here (mlp_train_common.py,
mlp_inputs_common.py and mlp_split_common.py hold those), and no call of ``helpers.rel_err``: that records its caller's line."""
import ctypes
import os

import torch

from freegaussian_amd import _lib
from freegaussian_amd import ops
from mlp_train_common import heads_of, loss_of

PTR = 4096  # an address nobody reads: the host tests' calls are all refused before a launch
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "fgraster.h")
GUARD = 1024  # floats of NaN on either side of an arena's array
NAN = float("nan")


def addr(struct):
    return ctypes.addressof(struct) if struct is not None else None


def header_text():
    with open(HEADER) as f:
        return f.read()


def desc(mode=_lib.MLP_PLAIN, A=21, rows=(3, 3, 4, 3), *, weights=True, inputs=False, outs=False, precision=0, ptr=PTR):
    """An ``fg_mlp_desc`` of the network's shape.  ``weights``: every parameter pointer set (the chain reads them; the
    parameter-gradient call alone takes a descriptor without); ``inputs``: ``x`` / ``aux`` and its row stride; ``outs``: one
    output per head.  Whatever is not asked for stays null."""
    d = _lib.MlpDesc()
    d.size, d.mode, d.depth, d.width, d.multires, d.aux_width = ctypes.sizeof(_lib.MlpDesc), mode, 8, 256, 10, A
    d.n_heads, d.precision = len(rows), precision
    for i, r in enumerate(rows):
        d.head_rows[i] = r
        if weights:
            d.head_weight[i], d.head_bias[i] = ptr, ptr
        if outs:
            d.out[i] = ptr
    for l in range(8 if weights else 0):
        d.weight[l], d.bias[l] = ptr, ptr
    if inputs:
        d.aux_stride, d.x, d.aux = A, ptr, ptr
    return d


def grads(weight=range(8), bias=range(8), head_weight=range(4), head_bias=range(4)):
    """An ``fg_mlp_grads`` that asks for the listed gradients."""
    g = _lib.MlpGrads()
    g.size = ctypes.sizeof(_lib.MlpGrads)
    for name, which in (("weight", weight), ("bias", bias), ("head_weight", head_weight), ("head_bias", head_bias)):
        for i in which:
            getattr(g, name)[i] = PTR
    return g


def arena(*shape, device="cuda"):
    """``(flat, view)``: an array of ``shape`` in an allocation of its own between two NaN bands of ``GUARD`` floats."""
    numel = 1
    for s in shape:
        numel *= s
    flat = torch.full((numel + 2 * GUARD,), NAN, device=device)
    return flat, flat[GUARD : GUARD + numel].view(*shape)


def out_shapes(A, rows):
    """The parameter gradients' shapes, restated (``ops`` has its own statement: the two are compared, not shared)."""
    in_ch = 63 + A
    return ([(256, in_ch if l == 0 else (in_ch + 256 if l == 5 else 256)) for l in range(8)] + [(256,)] * 8
            + [(r, 256) for r in rows] + [(r,) for r in rows])  # fmt: skip


def named_grads(module):
    """A copy of every parameter's gradient by name, ``None`` where there is none."""
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in module.named_parameters()}


def named_grads_or_zeros(module):
    """... with zeros where there is none: a parameter nothing reached compares as one whose gradient is zero."""
    return {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for k, p in module.named_parameters()}


def lib_calls(monkeypatch, names=None):
    """``ops._call`` wrapped: the list of the library calls' names as they are made (``names``: only those)."""
    seen = []
    real = ops._call

    def call(name, *a, **k):
        if names is None or name in names:
            seen.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(ops, "_call", call)
    return seen


def train_step(m_dev, x, aux, g_heads, **kw):
    """One taped ``ops.mlp_train`` + backward from the head cotangents: ``(raw, the parameter gradients there are, x.grad,
    aux.grad)``; ``x`` / ``aux`` want a gradient where ``input_grads`` is passed.  The module is left without gradients."""
    m_dev.requires_grad_(True).zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(kw.get("input_grads", False))
    aux = aux.detach().clone().requires_grad_(kw.get("input_grads", False))
    raw = ops.mlp_train(x, aux, m_dev.linear, heads_of(m_dev), **kw)
    raw.backward(g_heads)
    grads = {k: p.grad.detach().clone() for k, p in m_dev.named_parameters() if p.grad is not None}
    m_dev.requires_grad_(False).zero_grad(set_to_none=True)
    return raw.detach(), grads, x.grad, aux.grad


def stand_in_for_cuda(monkeypatch, is_cuda=True):
    """``ops.mlp_train`` replaced by a spy that returns zeros and, with ``is_cuda``, tensors that report CUDA: the dispatch
    alone, on the CPU.  Returns the list of the keywords of each call."""
    seen = []

    def fake(x, aux, trunk, heads, **kw):
        seen.append(kw)
        return torch.zeros(x.shape[0], sum(h.weight.shape[0] for h in heads)) + 0.0 * trunk[0].bias.sum()

    monkeypatch.setattr(ops, "mlp_train", fake)
    if is_cuda:
        monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    return seen


def grad_names(rows):
    """A label per parameter gradient, in the order of ``flat``."""
    k = len(rows)
    return [f"gW[{l}]" for l in range(8)] + [f"gb[{l}]" for l in range(8)] + [f"gWh[{h}]" for h in range(k)] + [f"gbh[{h}]" for h in range(k)]


def flat(grads4):
    """The four groups ``ops.mlp_param_grads`` returns as one list."""
    return [t for group in grads4 for t in group]


def module_inputs(kind, n, seed=1):
    """Points in [-1, 1) and what the module takes beside them: a control vector, else a time."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g) * 2 - 1
    return x, (torch.randn(n, 3, generator=g) * 0.1 if kind == "control" else torch.rand(n, 1, generator=g))


def module_step(m_dev, x, other, cots):
    """One forward and backward through the module itself: its parameter gradients by name."""
    m_dev.zero_grad(set_to_none=True)
    loss_of(m_dev(x, other), cots).backward()
    return named_grads(m_dev)
