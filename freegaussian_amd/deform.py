"""Deformation / control MLPs that feed the rasterizer.  Training runs the dense GEMMs on PyTorch-ROCm / hipBLASLt
(SURVEY.md §2 row 5); a forward that needs no gradient over at least ``FUSED_MIN_ROWS`` rows is one fused HIP call
(``ops.mlp_forward``: a weight re-ordering launch and the network's launch; ``FG_FUSED_MLP=0`` turns it off).
With ``FG_FUSED_MLP_TRAIN=1`` (opt-in; unset = off) a taped forward over as many rows runs as ``ops.mlp_train``: the fused
forward with saved activations, the fused backward data chain, and the weight gradients as chunked library products
(``mlp_param_grads``); ``FG_FUSED_MLP_TRAIN=2`` also takes the blender net and inputs that want a gradient
(``ops.mlp_train(..., input_grads=True)``: the backward that forms the gradient of the input row); with
``FG_FUSED_MLP_WGRAD=1`` (opt-in) on top of either, the weight gradients are one fused call too (``ops.mlp_param_grads``); with
``FG_FUSED_MLP_CHUNKED=1`` (opt-in) on top of both, the backward is one call that works through the rows in chunks and keeps no
``[8,N,256]`` gradient array (``ops.mlp_train_backward``); with ``FG_FUSED_MLP_PRECISION=bf16x3`` (opt-in) whichever of these
fused calls takes a call forms its trunk and data-chain products as split-bf16 products (``fused_precision``); with
``FG_FUSED_MLP_WGRAD_PRECISION=bf16x3`` (opt-in) on top of ``FG_FUSED_MLP_WGRAD=1`` the fused weight-gradient products are
split-bf16 products too (``fused_wgrad_precision``).  Behaviour and
``state_dict`` key names follow the reference's ``FreeGaussianDeformableModel`` / ``FreeGaussianControllableModel``
(freegaussian/freegaussian_model.py:1054-1145) so stage-1 checkpoints load unchanged; outputs are
checked against golden vectors produced by the reference classes (tests/golden/g_mlp.npz)."""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .utils import exp_se3, positional_encoding


def _trunk(in_ch: int, width: int, depth: int, skip_at: int) -> nn.ModuleList:
    """depth linears of `width`; the one AFTER index `skip_at` also takes the re-injected input."""
    layers = [nn.Linear(in_ch, width)]
    for i in range(depth - 1):
        layers.append(nn.Linear(width + in_ch if i == skip_at else width, width))
    return nn.ModuleList(layers)


def _tall_weight_grad(go: torch.Tensor, x: torch.Tensor, chunk: int = 8192) -> torch.Tensor:
    """go^T x ([N,out], [N,in] -> [out,in]) as a batched product over chunks of `chunk` rows, a sum of the partial
    matrices, and the product of the tail (see ``_TallLinear``)."""
    N = x.shape[0]
    B = N // chunk
    n0 = B * chunk
    gw = torch.bmm(go[:n0].view(B, chunk, go.shape[1]).transpose(1, 2), x[:n0].view(B, chunk, x.shape[1])).sum(0)
    if n0 < N:
        gw = gw + go[n0:].t() @ x[n0:]
    return gw


class _TallLinear(torch.autograd.Function):
    """x [N,in] -> x W^T + b for N in the hundreds of thousands.  Same library GEMMs forward and for the input
    gradient; the WEIGHT gradient go^T x is a [out, N] x [N, in] product -- 256 x 256 outputs, N-long dot products --
    which the BLAS runs as one small-tile kernel at a fraction of its rate (three quarters of the MLP's backward on an
    MI355X: 13.6 ms of 18 at 300k Gaussians).  Here it is a batched product over chunks of 8192 rows (shapes the library
    is good at) and a sum of the partial [out, in] matrices."""

    CHUNK = 8192

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return torch.addmm(bias, x, weight.t())

    @staticmethod
    def backward(ctx, go):
        x, weight = ctx.saved_tensors
        go = go.contiguous()
        gx = go @ weight if ctx.needs_input_grad[0] else None
        gw = None
        if ctx.needs_input_grad[1]:
            gw = _tall_weight_grad(go, x, _TallLinear.CHUNK)
        gb = go.sum(0) if ctx.needs_input_grad[2] else None
        return gx, gw, gb


def _linear(layer: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    if x.is_cuda and x.dim() == 2 and x.shape[0] >= 4 * _TallLinear.CHUNK and layer.bias is not None and x.is_contiguous():
        return _TallLinear.apply(x, layer.weight, layer.bias)
    return layer(x)


def _run_trunk(layers: nn.ModuleList, inp: torch.Tensor, skip_at: int) -> torch.Tensor:
    h = inp
    for i, layer in enumerate(layers):
        h = torch.relu(_linear(layer, h))
        if i == skip_at:
            h = torch.cat([inp, h], dim=-1)
    return h


# Rows from which a gradient-free forward takes the fused kernel: the threshold `_linear` uses, so every small scene keeps
# the torch path bit for bit.  Raised if the measured crossover lies above it, never lowered
# (profiles/mlp_forward.md: the fused forward takes 0.70 x the torch path's time at 33 000 rows, 0.61 x at 240 000 and 1M).
FUSED_MIN_ROWS = 4 * _TallLinear.CHUNK
# What an unset FG_FUSED_MLP means: "1" only where the measurement of profiles/mlp_forward.md meets the default-on rule
# (fused median <= 0.8 x the torch median from FUSED_MIN_ROWS rows on)
FUSED_DEFAULT = "1"


def fused_applies(module: nn.Module, x: torch.Tensor, other: torch.Tensor) -> bool:
    """Whether ``module(x, other)`` runs as one ``ops.mlp_forward`` call: CUDA fp32 inputs, nothing that wants a gradient,
    enough rows, the one network shape the kernel is built for, and ``FG_FUSED_MLP`` (read here, on the host; unset =
    ``FUSED_DEFAULT``) not "0".  Anything else: the torch ops."""
    if os.environ.get("FG_FUSED_MLP", FUSED_DEFAULT) == "0":
        return False
    if not (x.is_cuda and other.is_cuda and x.dtype == other.dtype == torch.float32 and x.dim() == other.dim() == 2):
        return False
    other_ch = 3 if isinstance(module, FreeGaussianControllableModel) else 1
    if x.shape[0] < FUSED_MIN_ROWS or other.shape[0] != x.shape[0] or x.shape[1] != 3 or other.shape[1] != other_ch:
        return False
    if (module.D, module.W, module.multires, module.skip_at) != (8, 256, 10, 4):
        return False
    taped = torch.is_grad_enabled()
    if taped and (x.requires_grad or other.requires_grad):
        return False
    for p in module.parameters():
        if not p.is_cuda or p.dtype != torch.float32 or (taped and p.requires_grad):
            return False
    return True


def fused_train_mode(module: nn.Module, x: torch.Tensor, other: torch.Tensor) -> str:
    """How a taped ``module(x, other)`` runs: "" = the torch ops, "1" or "2" = one ``ops.mlp_train`` call, the value being
    ``FG_FUSED_MLP_TRAIN`` (read here and nowhere else, on the host, on every call; unset = off).  Either wants grad mode on
    and a parameter that wants a gradient, CUDA fp32, enough rows and the one network shape the kernels are built for.
    "1" wants inputs that need no gradient and not the blender net (its ``timenet`` needs the gradient of the encoded time,
    which ``fg_mlp_bwd`` does not form); "2" takes those too, through ``ops.mlp_train(..., input_grads=True)``
    (``fg_mlp_bwd_inputs``)."""
    knob = os.environ.get("FG_FUSED_MLP_TRAIN", "0")
    if knob not in ("1", "2"):
        return ""
    if not torch.is_grad_enabled() or (knob == "1" and (x.requires_grad or other.requires_grad)):
        return ""
    if not (x.is_cuda and other.is_cuda and x.dtype == other.dtype == torch.float32 and x.dim() == other.dim() == 2):
        return ""
    other_ch = 3 if isinstance(module, FreeGaussianControllableModel) else 1
    if x.shape[0] < FUSED_MIN_ROWS or other.shape[0] != x.shape[0] or x.shape[1] != 3 or other.shape[1] != other_ch:
        return ""
    if (module.D, module.W, module.multires, module.skip_at) != (8, 256, 10, 4):
        return ""
    if knob == "1" and getattr(module, "is_blender", False):
        return ""
    params = list(module.parameters())
    ok = all(p.is_cuda and p.dtype == torch.float32 for p in params) and any(p.requires_grad for p in params)
    return knob if ok else ""


def fused_precision() -> str:
    """The ``precision`` of the fused calls: ``FG_FUSED_MLP_PRECISION`` (opt-in; read here and nowhere else, on the host, on
    every call) -- unset or "fp32": the exact-fp32 kernels; "bf16x3": the split-bf16 product of include/fgraster.h in the
    forward's trunk and the backward's data chain (the weight gradients stay fp32; profiles/mlp_split_bf16.md).  Anything
    else is a ``ValueError``: a typo must not train silently in fp32.  It has effect only where a fused path already takes
    the call (``fused_applies``, ``fused_train_mode``): no dispatch of its own."""
    knob = os.environ.get("FG_FUSED_MLP_PRECISION", "fp32")
    if knob not in ("fp32", "bf16x3"):
        raise ValueError(f"FG_FUSED_MLP_PRECISION wants fp32 or bf16x3, got {knob!r}")
    return knob


def _precision_keywords() -> dict:
    """``precision=`` for a fused call, only where the knob asks for something other than the default."""
    knob = fused_precision()
    return {} if knob == "fp32" else {"precision": knob}


def fused_wgrad_precision() -> str:
    """The precision of the fused parameter-gradient products: ``FG_FUSED_MLP_WGRAD_PRECISION`` (opt-in; read here and
    nowhere else, on the host, on every call) -- unset or "fp32": the exact-fp32 kernel; "bf16x3": the split-bf16 tile job
    of ``fg_mlp_param_grads_p`` (include/fgraster.h; profiles/mlp_wgrad_split.md).  Anything else is a ``ValueError``: a
    typo must not train silently in fp32.  It has effect only where ``FG_FUSED_MLP_WGRAD=1`` already asks for the fused
    products, and does not depend on ``FG_FUSED_MLP_PRECISION``."""
    knob = os.environ.get("FG_FUSED_MLP_WGRAD_PRECISION", "fp32")
    if knob not in ("fp32", "bf16x3"):
        raise ValueError(f"FG_FUSED_MLP_WGRAD_PRECISION wants fp32 or bf16x3, got {knob!r}")
    return knob


def fused_se3() -> bool:
    """Whether the means are moved by one ``ops.se3_apply`` call in place of ``_se3`` + ``utils.transform_points``:
    ``FG_FUSED_SE3`` (opt-in; read here and nowhere else, on the host, on every call) -- unset or "0": the torch ops; "1": the
    fused op, forward and backward (profiles/se3_apply_fused.md).  Anything else is a ``ValueError``: a typo must not train
    silently on the other path.  The callers (model.py) add their own conditions: CUDA float32 tensors, and a call that
    ``deformed_points`` has not already taken."""
    knob = os.environ.get("FG_FUSED_SE3", "0")
    if knob not in ("0", "1"):
        raise ValueError(f"FG_FUSED_SE3 wants 0 or 1, got {knob!r}")
    return knob == "1"


def fused_control() -> bool:
    """Whether stage 2's glue around the control MLP -- mask rows, attribute means, control values, the scatter into the full
    set -- runs on a cached plan of the mask through the ``ops.control_*`` calls in place of boolean indexing, a Python loop and
    ``index_put``: ``FG_FUSED_CONTROL`` (opt-in; read here and nowhere else, on the host, on every call) -- unset or "0": the
    torch ops; "1": the fused stage, with no host synchronisation per step (profiles/control_fused.md).  Anything else is a
    ``ValueError``: a typo must not train silently on the other path.  The caller (model.fused_control_applies) adds its own
    conditions: CUDA float32 tensors, no crop, 1 to 32 attributes, each with at least one row."""
    knob = os.environ.get("FG_FUSED_CONTROL", "0")
    if knob not in ("0", "1"):
        raise ValueError(f"FG_FUSED_CONTROL wants 0 or 1, got {knob!r}")
    return knob == "1"


def fused_train_applies(module: nn.Module, x: torch.Tensor, other: torch.Tensor) -> bool:
    """Whether a taped ``module(x, other)`` runs as one ``ops.mlp_train`` call (``fused_train_mode``)."""
    return fused_train_mode(module, x, other) != ""


def _train_keywords(mode: str) -> dict:
    """``ops.mlp_train``'s keywords for a ``fused_train_mode``: "2" = the call also returns the gradients of its inputs;
    ``FG_FUSED_MLP_WGRAD=1`` (opt-in; read here and nowhere else, on the host, on every call; unset = off) = its parameter
    gradients come from the fused call ``ops.mlp_param_grads`` in place of ``mlp_param_grads`` below.  The knob has no
    lower row bound of its own: it wins at every size measured (profiles/mlp_wgrad.md: 0.49 against 1.42 ms at 33 000 rows,
    the smallest, within 1 % of ``FUSED_MIN_ROWS``, the fewest rows a fused training call sees).
    ``FG_FUSED_MLP_CHUNKED=1`` (opt-in; read here and nowhere else, on the host, on every call; unset = off) on top of that
    knob -- without it it does nothing -- = the backward is one ``fg_mlp_train_bwd`` call over row chunks: the same gradients
    bit for bit, 8 KB per row less memory (profiles/mlp_chunked_bwd.md).
    ``FG_FUSED_MLP_WGRAD_PRECISION=bf16x3`` (opt-in; ``fused_wgrad_precision``) on top of ``FG_FUSED_MLP_WGRAD=1`` -- without it
    it does nothing -- = the fused parameter gradients' hidden and input products are split-bf16 products
    (profiles/mlp_wgrad_split.md); independent of ``FG_FUSED_MLP_PRECISION``."""
    kw = {"input_grads": True} if mode == "2" else {}
    kw.update(_precision_keywords())  # (FG_FUSED_MLP_PRECISION: fused_precision above)
    wgrad_precision = fused_wgrad_precision()  # (read, so validated, whether or not it has an effect)
    if os.environ.get("FG_FUSED_MLP_WGRAD", "0") == "1":
        kw["fused_param_grads"] = True
        if wgrad_precision != "fp32":
            kw["param_grads_precision"] = wgrad_precision
        if os.environ.get("FG_FUSED_MLP_CHUNKED", "0") == "1":
            kw["chunked_backward"] = True
    return kw


def mlp_param_grads(inp: torch.Tensor, H: torch.Tensor, G: torch.Tensor, g_heads: torch.Tensor, head_rows):
    """The parameter gradients of the trunk and the heads from what the fused training calls leave behind (any device,
    any float type): ``inp`` [N,in_ch] the encoded input rows, ``H`` [8,N,W] the post-ReLU activations, ``G`` [8,N,W] the
    gradients of the pre-activations (``P_l`` of include/fgraster.h), ``g_heads`` [N, rows_total] the head cotangents.
    Returns ``(gW x 8, gb x 8, gW_head per head, gb_head per head)``: ``gW_l = P_l^T in_l`` with ``in_l = h_{l-1}``,
    ``in_0 = inp`` and ``in_5 = [inp, h_4]`` (two products side by side), every product chunked as ``_TallLinear``'s."""
    C = _TallLinear.CHUNK
    gW = []
    for l in range(H.shape[0]):
        if l == 0:
            gW.append(_tall_weight_grad(G[0], inp, C))
        elif l == H.shape[0] // 2 + 1:
            gW.append(torch.cat([_tall_weight_grad(G[l], inp, C), _tall_weight_grad(G[l], H[l - 1], C)], dim=1))
        else:
            gW.append(_tall_weight_grad(G[l], H[l - 1], C))
    gb = G.sum(1).unbind(0)
    gWh = _tall_weight_grad(g_heads, H[-1], C).split(list(head_rows), dim=0)
    gbh = g_heads.sum(0).split(list(head_rows))
    return gW, gb, gWh, gbh


def _one_row_if_broadcast(t: torch.Tensor) -> torch.Tensor:
    """``times.expand(N, -1)`` has row stride 0: its encoding is computed on one row and broadcast by the kernel."""
    return t[:1] if t.stride(0) == 0 else t


class FreeGaussianDeformableModel(nn.Module):
    """(x [N,3], t [N,1]) -> (SE(3) per Gaussian [N,4,4], d_rotation [N,4], d_scaling [N,3])."""

    def __init__(self, D: int = 8, W: int = 256, multires: int = 10, is_blender: bool = False):
        super().__init__()
        self.D, self.W, self.is_blender = D, W, is_blender
        self.multires = multires
        self.t_multires = 6 if is_blender else 10
        self.skip_at = D // 2
        xyz_ch = 3 * (1 + 2 * multires)
        t_ch = 1 + 2 * self.t_multires
        if is_blender:
            self.time_out = 30
            self.timenet = nn.Sequential(nn.Linear(t_ch, 256), nn.ReLU(inplace=True), nn.Linear(256, self.time_out))
            t_ch = self.time_out
        self.input_ch = xyz_ch + t_ch
        self.linear = _trunk(self.input_ch, W, D, self.skip_at)
        self.branch_w = nn.Linear(W, 3)
        self.branch_v = nn.Linear(W, 3)
        self.gaussian_rotation = nn.Linear(W, 4)
        self.gaussian_scaling = nn.Linear(W, 3)

    def _fused(self, x: torch.Tensor, t: torch.Tensor, outs):
        from . import ops

        with torch.no_grad():
            aux = positional_encoding(_one_row_if_broadcast(t), self.t_multires)
            if self.is_blender:
                aux = self.timenet(aux)
            heads = (self.branch_w, self.branch_v, self.gaussian_rotation, self.gaussian_scaling)
            return ops.mlp_forward(x, aux, self.linear, heads, mode="se3", outs=outs, **_precision_keywords())

    def deformed_points(self, x: torch.Tensor, t: torch.Tensor):
        """(transform_points(d_xyz, x) [N,3], d_rotation, d_scaling) without the [N,4,4] transforms: what a render that
        needs no gradient reads.  Only where ``fused_applies(self, x, t)``."""
        _, rot, scale, pts = self._fused(x, t, (False, None, None, None))
        return pts, rot, scale

    def heads(self, x: torch.Tensor, t: torch.Tensor):
        """The raw heads ``(w [N,3], v [N,3], d_rotation [N,4], d_scaling [N,3])`` of a call that is NOT a fused gradient-free
        forward (``fused_applies``: that one goes from the positions to the transforms inside its kernel): through
        ``ops.mlp_train`` where ``fused_train_mode`` says so, else the torch ops."""
        mode = fused_train_mode(self, x, t)
        if mode:
            from . import ops

            # (taped: under "2" a time that wants a gradient, and the blender net's timenet, get theirs through aux)
            aux = positional_encoding(_one_row_if_broadcast(t), self.t_multires)
            if self.is_blender:
                aux = self.timenet(aux)
            heads = (self.branch_w, self.branch_v, self.gaussian_rotation, self.gaussian_scaling)
            return ops.mlp_train(x, aux, self.linear, heads, **_train_keywords(mode)).split((3, 3, 4, 3), dim=-1)
        t_emb = positional_encoding(t, self.t_multires)
        if self.is_blender:
            t_emb = self.timenet(t_emb)
        inp = torch.cat([positional_encoding(x, self.multires), t_emb], dim=-1)
        h = _run_trunk(self.linear, inp, self.skip_at)
        w, v = _linear(self.branch_w, h), _linear(self.branch_v, h)
        return w, v, _linear(self.gaussian_rotation, h), _linear(self.gaussian_scaling, h)

    def forward(self, x: torch.Tensor, t: torch.Tensor):
        if fused_applies(self, x, t):
            return tuple(self._fused(x, t, (None, None, None, False))[:3])
        w, v, rot, scale = self.heads(x, t)
        return self._se3(w, v), rot, scale

    @staticmethod
    def _se3(w: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        theta = w.norm(dim=-1, keepdim=True)
        # the reference adds 1e-5 AFTER the division (freegaussian_model.py:1106-1107)
        screw = torch.cat([w / theta + 1e-5, v / theta + 1e-5], dim=-1)
        return exp_se3(screw, theta)


class FreeGaussianControllableModel(nn.Module):
    """(control points [M,3], control value [M,3]) -> (d_xyz [M,3], d_rot [M,4], d_scale [M,3])."""

    def __init__(self, D: int = 8, W: int = 256, multires: int = 10):
        super().__init__()
        self.D, self.W, self.multires = D, W, multires
        self.skip_at = D // 2
        self.input_ch = 2 * 3 * (1 + 2 * multires)
        self.linear = _trunk(self.input_ch, W, D, self.skip_at)
        self.d_xyz = nn.Linear(W, 3)
        self.d_scale = nn.Linear(W, 3)
        self.d_rot = nn.Linear(W, 4)

    def forward(self, x: torch.Tensor, value: torch.Tensor):
        if fused_applies(self, x, value):
            from . import ops

            with torch.no_grad():
                aux = positional_encoding(_one_row_if_broadcast(value), self.multires)
                heads = (self.d_xyz, self.d_rot, self.d_scale)
                return tuple(ops.mlp_forward(x, aux, self.linear, heads, mode="plain", **_precision_keywords()))
        mode = fused_train_mode(self, x, value)
        if mode:
            from . import ops

            aux = positional_encoding(_one_row_if_broadcast(value), self.multires)
            heads = (self.d_xyz, self.d_rot, self.d_scale)
            return ops.mlp_train(x, aux, self.linear, heads, **_train_keywords(mode)).split((3, 4, 3), dim=-1)
        inp = torch.cat([positional_encoding(x, self.multires), positional_encoding(value, self.multires)], dim=-1)
        h = _run_trunk(self.linear, inp, self.skip_at)
        return _linear(self.d_xyz, h), _linear(self.d_rot, h), _linear(self.d_scale, h)
