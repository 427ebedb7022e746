"""Every refusal of the fused MLP's Python layer, pinned by its message: ``ops._mlp_precision``, ``ops._mlp_desc``,
``ops.mlp_forward``, ``ops.mlp_param_grads``, ``ops.mlp_train_backward`` and ``ops.mlp_train``.  Each row of the table is
one bad call and a fragment that only the refusal it meets prints; where a call trips two checks the row pins the one that
fires first -- that order is part of the behaviour.  On the CPU: tensors report CUDA through a stand-in, and ``ops._call``
is a recorder that must stay empty (nothing is launched)."""
import re

import pytest
import torch

from freegaussian_amd import deform as D
from freegaussian_amd import ops

N = 8
ROWS = (3, 3, 4, 3)
_M = D.FreeGaussianDeformableModel()
TRUNK = [(l.weight, l.bias) for l in _M.linear]
HEADS = [(l.weight, l.bias) for l in (_M.branch_w, _M.branch_v, _M.gaussian_rotation, _M.gaussian_scaling)]
X, AUX = torch.zeros(N, 3), torch.zeros(N, 21)
ENC, H, G, GH = torch.zeros(N, 88), torch.zeros(8, N, 256), torch.zeros(8, N, 256), torch.zeros(N, 13)
H_STRIDED = H.transpose(0, 1).contiguous().transpose(0, 1)  # the shape of H, not its layout
H_SHORT = torch.zeros(8, N - 1, 256)
NO_BIAS = TRUNK[:3] + [(TRUNK[3][0], None)] + TRUNK[4:]
LAYER5_SQUARE = TRUNK[:5] + [(torch.zeros(256, 256), torch.zeros(256))] + TRUNK[6:]
HEAD1_NARROW = HEADS[:1] + [(torch.zeros(3, 128), torch.zeros(3))] + HEADS[2:]


def pg(enc=ENC, h=H, g=G, gh=GH, A=21, rows=ROWS, **kw):
    return ops.mlp_param_grads(enc, h, g, gh, A, rows, **kw)


def tb(enc=ENC, h=H, gh=GH, trunk=TRUNK, heads=HEADS, A=21, rows=ROWS, **kw):
    return ops.mlp_train_backward(enc, h, gh, trunk, heads, A, rows, **kw)


def tr(x=X, aux=AUX, trunk=TRUNK, heads=HEADS, **kw):
    return ops.mlp_train(x, aux, trunk, heads, **kw)


def fw(x=X, aux=AUX, trunk=TRUNK, heads=HEADS, **kw):
    return ops.mlp_forward(x, aux, trunk, heads, **kw)


def _gradient_call_rows(f, who):
    """The refusals the two gradient calls share, in the order their checks stand."""
    tensors = f"{who} wants contiguous CUDA float32 tensors"
    double = dict(enc=ENC.double(), h=H.double(), gh=GH.double(), **({"g": G.double()} if f is pg else {}))
    return [
        (f"{who}-cpu-tensor", f, {}, tensors, False),
        (f"{who}-float64", f, double, tensors, True),
        (f"{who}-strided-H", f, dict(h=H_STRIDED), tensors, True),
        (f"{who}-aux-width-0", f, dict(A=0), f"{who}: aux width 0 / head rows [3, 3, 4, 3] outside", True),
        (f"{who}-aux-width-65", f, dict(A=65), f"{who}: aux width 65 / head rows", True),
        (f"{who}-no-heads", f, dict(rows=()), f"{who}: aux width 21 / head rows [] outside", True),
        (f"{who}-five-heads", f, dict(rows=(3, 3, 4, 3, 3)), f"{who}: aux width 21 / head rows [3, 3, 4, 3, 3] outside", True),
        (f"{who}-head-of-0-rows", f, dict(rows=(3, 0, 4, 3)), f"{who}: aux width 21 / head rows [3, 0, 4, 3] outside", True),
        (f"{who}-17-rows", f, dict(rows=(5, 5, 4, 3)), f"{who}: aux width 21 / head rows [5, 5, 4, 3] outside", True),
        # (63 + 26 pads to 96; 63 + 22 would pad to ENC's own 88 and meet no refusal here)
        (f"{who}-enc-of-another-width", f, dict(A=26), f"{who} wants enc [N, 96], got (8, 88)", True),
        (f"{who}-g_heads-of-another-width", f, dict(gh=torch.zeros(N, 12)), f"{who} wants g_heads [8, 13], got (8, 12)", True),
        (f"{who}-want-of-wrong-length", f, dict(want=[True] * 5), f"{who}: want has 5 entries for 24 gradients", True),
        (f"{who}-unknown-precision", f, dict(precision="fp16"), f"{who}: precision wants one of ['bf16x3', 'fp32'], got 'fp16'", True),
        # the order: the precision before the tensors, the tensors before the shapes, enc before H before g_heads before want
        (f"{who}-precision-before-tensors", f, dict(precision=None), f"{who}: precision wants one of", False),
        (f"{who}-tensors-before-aux-width", f, dict(h=H_STRIDED, A=0), tensors, True),
        (f"{who}-rows-before-enc", f, dict(A=26, rows=()), f"{who}: aux width 26 / head rows [] outside", True),
        (f"{who}-enc-before-H", f, dict(A=26, h=H_SHORT), f"{who} wants enc [N, 96]", True),
        (f"{who}-g_heads-before-want", f, dict(gh=torch.zeros(N, 12), want=[True] * 5), f"{who} wants g_heads [8, 13]", True),
    ]


TABLE = [
    *_gradient_call_rows(pg, "mlp_param_grads"),
    ("mlp_param_grads-H-of-another-N", pg, dict(h=H_SHORT), "mlp_param_grads wants H and G [8, 8, 256], got (8, 7, 256) and (8, 8, 256)", True),
    ("mlp_param_grads-G-unlike-H", pg, dict(g=torch.zeros(7, N, 256)), "mlp_param_grads wants H and G [8, 8, 256], got (8, 8, 256) and (7, 8, 256)", True),
    ("mlp_param_grads-H-before-g_heads", pg, dict(h=H_SHORT, gh=torch.zeros(N, 12)), "mlp_param_grads wants H and G [8, 8, 256]", True),
    *_gradient_call_rows(tb, "mlp_train_backward"),
    ("mlp_train_backward-H-of-another-N", tb, dict(h=H_SHORT), "mlp_train_backward wants H [8, 8, 256], got (8, 7, 256)", True),
    ("mlp_train_backward-H-before-g_heads", tb, dict(h=H_SHORT, gh=torch.zeros(N, 12)), "mlp_train_backward wants H [8, 8, 256]", True),
    ("mlp_train_backward-chunk_slabs--1", tb, dict(chunk_slabs=-1), "mlp_train_backward: chunk_slabs wants an int >= 0, got -1", True),
    ("mlp_train_backward-chunk_slabs-True", tb, dict(chunk_slabs=True), "mlp_train_backward: chunk_slabs wants an int >= 0, got True", True),
    ("mlp_train_backward-chunk_slabs-1.5", tb, dict(chunk_slabs=1.5), "mlp_train_backward: chunk_slabs wants an int >= 0, got 1.5", True),
    # chunk_slabs sits between the head rows and enc
    ("mlp_train_backward-rows-before-chunk_slabs", tb, dict(A=0, chunk_slabs=-1), "mlp_train_backward: aux width 0 / head rows", True),
    ("mlp_train_backward-chunk_slabs-before-enc", tb, dict(A=26, chunk_slabs=-1), "mlp_train_backward: chunk_slabs wants", True),
    ("mlp_train_backward-rows-not-the-heads", tb, dict(rows=(3, 4, 3, 3)), "mlp_train_backward: head rows [3, 4, 3, 3] are not the heads' [3, 3, 4, 3]", True),
    ("mlp_train_backward-unknown-param_grads_precision", tb, dict(param_grads_precision="tf32"),
     "mlp_train_backward: precision wants one of ['bf16x3', 'fp32'], got 'tf32'", True),
    ("mlp_train_backward-precision-before-param_grads_precision", tb, dict(precision="fp16", param_grads_precision="tf32"),
     "mlp_train_backward: precision wants one of ['bf16x3', 'fp32'], got 'fp16'", True),
    # ... and then the descriptor's own (the network is looked at last: a want of the wrong length comes first)
    ("mlp_train_backward-7-trunk-layers", tb, dict(trunk=TRUNK[:7]), "mlp_train_backward wants 8 trunk layers and 1..4 heads, got 7 and 4", True),
    ("mlp_train_backward-want-before-the-network", tb, dict(trunk=TRUNK[:7], want=[True] * 5), "mlp_train_backward: want has 5 entries", True),
    ("mlp_train_backward-trunk-of-another-aux-width", tb, dict(A=22),
     "mlp_train_backward: trunk layer 0 wants weight (256, 85) and a bias, got (256, 84)", True),
    ("mlp_train_backward-head-of-wrong-width", tb, dict(heads=HEAD1_NARROW),
     "mlp_train_backward: head 1 wants weight [rows, 256] and a bias, got (3, 128)", True),
    ("mlp_train-7-trunk-layers", tr, dict(trunk=TRUNK[:7]), "mlp_train wants 8 trunk layers and 1..4 heads, got 7 and 4", True),
    ("mlp_train-0-heads", tr, dict(heads=[]), "mlp_train wants 8 trunk layers and 1..4 heads, got 8 and 0", True),
    ("mlp_train-5-heads", tr, dict(heads=HEADS + HEADS[:1]), "mlp_train wants 8 trunk layers and 1..4 heads, got 8 and 5", True),
    ("mlp_train-layer-without-bias", tr, dict(trunk=NO_BIAS), "mlp_train wants CUDA float32 tensors (and a bias on every layer)", True),
    ("mlp_train-cpu-tensor", tr, {}, "mlp_train wants CUDA float32 tensors (and a bias on every layer)", False),
    ("mlp_train-float64", tr, dict(x=X.double()), "mlp_train wants CUDA float32 tensors (and a bias on every layer)", True),
    ("mlp_train-x-of-one-dimension", tr, dict(x=torch.zeros(N)), "mlp_train wants [N,3] points with N >= 1, got (8,)", True),
    ("mlp_train-N-0", tr, dict(x=torch.zeros(0, 3)), "mlp_train wants [N,3] points with N >= 1, got (0, 3)", True),
    ("mlp_train-chunked_backward-0", tr, dict(chunked_backward=0, fused_param_grads=True),
     "mlp_train: chunked_backward wants True or a positive int, got 0", True),
    ("mlp_train-chunked_backward--1", tr, dict(chunked_backward=-1, fused_param_grads=True),
     "mlp_train: chunked_backward wants True or a positive int, got -1", True),
    ("mlp_train-chunked_backward-yes", tr, dict(chunked_backward="yes", fused_param_grads=True),
     "mlp_train: chunked_backward wants True or a positive int, got 'yes'", True),
    ("mlp_train-chunked-without-fused", tr, dict(chunked_backward=True), "mlp_train: chunked_backward forms the fused parameter gradients", True),
    ("mlp_train-bf16x3-wgrad-without-fused", tr, dict(param_grads_precision="bf16x3"),
     "mlp_train: param_grads_precision='bf16x3' splits the fused parameter gradients", True),
    ("mlp_train-unknown-precision", tr, dict(precision="fp16"), "mlp_train: precision wants one of ['bf16x3', 'fp32'], got 'fp16'", True),
    ("mlp_train-unknown-param_grads_precision", tr, dict(param_grads_precision="tf32", fused_param_grads=True),
     "mlp_train: precision wants one of ['bf16x3', 'fp32'], got 'tf32'", True),
    # the order: the precisions, the chunks' value before their need of the fused gradients, the network before the tensors
    ("mlp_train-precision-before-chunked_backward", tr, dict(precision="fp16", chunked_backward=0), "mlp_train: precision wants one of", True),
    ("mlp_train-bf16x3-wgrad-before-chunked_backward", tr, dict(param_grads_precision="bf16x3", chunked_backward=0),
     "mlp_train: param_grads_precision='bf16x3' splits", True),
    ("mlp_train-chunked-value-before-fused", tr, dict(chunked_backward=-1), "mlp_train: chunked_backward wants True or a positive int", True),
    ("mlp_train-chunked-before-the-network", tr, dict(chunked_backward=True, trunk=TRUNK[:7]), "mlp_train: chunked_backward forms", True),
    ("mlp_train-network-before-tensors", tr, dict(trunk=TRUNK[:7]), "mlp_train wants 8 trunk layers", False),
    ("mlp_train-tensors-before-points", tr, dict(x=torch.zeros(N).double()), "mlp_train wants CUDA float32 tensors", True),
    # ... and what is left to the descriptor, met in the autograd function's forward
    ("mlp_train-x-not-N-by-3", tr, dict(x=torch.zeros(N, 2)), "mlp_train wants [N,3] points, got (8, 2)", True),
    ("mlp_train-aux-of-65-columns", tr, dict(aux=torch.zeros(N, 65)), "mlp_train wants aux [N or 1, 1..64], got (8, 65) for N = 8", True),
    ("mlp_train-trunk-layer-of-wrong-shape", tr, dict(trunk=LAYER5_SQUARE),
     "mlp_train: trunk layer 5 wants weight (256, 340) and a bias, got (256, 256)", True),
    ("mlp_train-head-of-wrong-width", tr, dict(heads=HEAD1_NARROW), "mlp_train: head 1 wants weight [rows, 256] and a bias, got (3, 128)", True),
    ("mlp_forward-unknown-mode", fw, dict(mode="quat"), "mlp_forward: unknown mode 'quat'", True),
    ("mlp_forward-unknown-precision", fw, dict(precision="fp16"), "mlp_forward: precision wants one of ['bf16x3', 'fp32'], got 'fp16'", True),
    ("mlp_forward-mode-before-precision", fw, dict(mode="quat", precision="fp16"), "mlp_forward: unknown mode", True),
    ("mlp_forward-precision-before-the-network", fw, dict(precision="fp16", trunk=TRUNK[:7]), "mlp_forward: precision wants one of", True),
    ("mlp_forward-7-trunk-layers", fw, dict(trunk=TRUNK[:7]), "mlp_forward wants 8 trunk layers and 1..4 heads, got 7 and 4", True),
    ("mlp_forward-5-heads", fw, dict(heads=HEADS + HEADS[:1]), "mlp_forward wants 8 trunk layers and 1..4 heads, got 8 and 5", True),
    ("mlp_forward-outs-of-wrong-length", fw, dict(outs=[None] * 3), "mlp_forward: mode 'se3' with 4 heads has 4 outputs, got 3", True),
    ("mlp_forward-plain-outs-of-wrong-length", fw, dict(mode="plain", heads=HEADS[:2], outs=[None] * 4),
     "mlp_forward: mode 'plain' with 2 heads has 2 outputs, got 4", True),
    ("mlp_forward-outs-entry-of-wrong-shape", fw, dict(outs=[torch.zeros(N, 4, 4), torch.zeros(N, 3), None, None]),
     "mlp_forward: output 1 wants a contiguous CUDA float32 (8, 4)", True),
    ("mlp_forward-outs-entry-float64", fw, dict(outs=[torch.zeros(N, 4, 4).double(), None, None, None]),
     "mlp_forward: output 0 wants a contiguous CUDA float32 (8, 4, 4)", True),
    ("mlp_forward-x-not-N-by-3", fw, dict(x=torch.zeros(N, 2)), "mlp_forward wants [N,3] points, got (8, 2)", True),
    ("mlp_forward-x-of-one-dimension", fw, dict(x=torch.zeros(N)), "mlp_forward wants [N,3] points, got (8,)", True),
    ("mlp_forward-aux-of-0-columns", fw, dict(aux=torch.zeros(N, 0)), "mlp_forward wants aux [N or 1, 1..64], got (8, 0) for N = 8", True),
    ("mlp_forward-aux-of-65-columns", fw, dict(aux=torch.zeros(N, 65)), "mlp_forward wants aux [N or 1, 1..64], got (8, 65) for N = 8", True),
    ("mlp_forward-aux-of-3-rows", fw, dict(aux=torch.zeros(3, 21)), "mlp_forward wants aux [N or 1, 1..64], got (3, 21) for N = 8", True),
    ("mlp_forward-points-before-aux", fw, dict(x=torch.zeros(N, 2), aux=torch.zeros(3, 21)), "mlp_forward wants [N,3] points", True),
    ("mlp_forward-network-before-points", fw, dict(x=torch.zeros(N, 2), trunk=TRUNK[:7]), "mlp_forward wants 8 trunk layers", True),
    ("mlp_forward-trunk-layer-of-wrong-shape", fw, dict(trunk=LAYER5_SQUARE),
     "mlp_forward: trunk layer 5 wants weight (256, 340) and a bias, got (256, 256)", True),
    ("mlp_forward-trunk-of-another-aux-width", fw, dict(aux=torch.zeros(N, 22)),
     "mlp_forward: trunk layer 0 wants weight (256, 85) and a bias, got (256, 84)", True),
    ("mlp_forward-trunk-layer-without-bias", fw, dict(trunk=NO_BIAS), "mlp_forward: trunk layer 3 wants weight (256, 256) and a bias", True),
    ("mlp_forward-head-of-wrong-width", fw, dict(heads=HEAD1_NARROW), "mlp_forward: head 1 wants weight [rows, 256] and a bias, got (3, 128)", True),
    ("mlp_forward-head-without-bias", fw, dict(heads=[(HEADS[0][0], None)] + HEADS[1:]), "mlp_forward: head 0 wants weight [rows, 256] and a bias", True),
    ("mlp_forward-aux-before-trunk", fw, dict(aux=torch.zeros(3, 21), trunk=LAYER5_SQUARE), "mlp_forward wants aux [N or 1, 1..64]", True),
    ("mlp_forward-trunk-before-heads", fw, dict(trunk=LAYER5_SQUARE, heads=HEAD1_NARROW), "mlp_forward: trunk layer 5 wants", True),
    ("mlp_forward-heads-before-outs", fw, dict(heads=HEAD1_NARROW, outs=[None] * 3), "mlp_forward: head 1 wants", True),
]


@pytest.mark.parametrize("call,kwargs,match,stand_in", [pytest.param(*row[1:], id=row[0]) for row in TABLE])
def test_refusal_is_the_one_named_and_nothing_is_launched(monkeypatch, call, kwargs, match, stand_in):
    if stand_in:  # everything but the device: tensors that report CUDA, so that each other refusal is seen to be its own
        monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    launched = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: launched.append(a))
    with pytest.raises(ValueError, match=re.escape(match)):
        call(**kwargs)
    assert not launched
