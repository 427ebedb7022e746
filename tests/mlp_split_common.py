"""Shared by tests/test_mlp_split_host.py and tests/test_mlp_split_gpu.py: the CPU emulation of the split-bf16 contract of
include/fgraster.h (``FG_MLP_BF16X3``) -- ``split`` by two roundings to bfloat16, a product as the three bf16-exact products
summed in float32 -- the network and the backward's data chain built on it, and row pools filtered for the ReLU's kink.

The emulation is no bit-for-bit model of the kernels (the order of the float32 sums differs); it restates the arithmetic, and
both it and the kernels are held to the project's one bar, 1e-4 of each array's largest magnitude against float64.

The kink margin: the split moves a pre-activation by about 5e-6 of its layer's scale, so a row with a pre-activation
nearer to zero than that may take the other ReLU branch, and its gradient is then simply another one.  Rows are drawn
clear of the kink by ``MARGIN`` = 1e-4 of the layer's largest pre-activation (20 x the shift): ``POOL`` = 4096 candidates for
``ROWS`` = 1024 wanted; about half of a pool survives (asserted: at least ``ROWS``)."""
import torch

from freegaussian_amd import deform as D
from freegaussian_amd.utils import positional_encoding, transform_points
from mlp_inputs_common import _raw_inputs, float64_with_input_row, make_net, rows_clear_of_the_kink_aux
from mlp_train_common import aux_of, head_rows, heads_of, outputs_from_raw, rows_clear_of_the_kink

MARGIN, POOL, ROWS = 1e-4, 4096, 1024


def split(v):
    """(hi, lo) of the contract as float32 tensors: hi = bf16(v) (round to nearest even), lo = bf16(v - hi)."""
    v = v.float()
    hi = v.bfloat16().float()
    return hi, (v - hi).bfloat16().float()


def product(a, b, terms=3):
    """``a @ b`` as A_hi B_hi + A_hi B_lo + A_lo B_hi (each product of two bfloat16 values is exact in float32; float32
    sums).  ``terms`` = 2 leaves the third out, 1 the second too: what the tests show to miss the bar."""
    ah, al = split(a)
    bh, bl = split(b)
    out = ah @ bh
    if terms >= 2:
        out = out + ah @ bl
    if terms >= 3:
        out = out + al @ bh
    return out


def emulate(m, x, aux, g_heads, terms=3):
    """The fused training forward and the backward's data chain under ``FG_MLP_BF16X3`` on the CPU, in the arrays the calls
    store (all float32): ``dict(enc [N,in_ch], H [8,N,256], raw, G [8,N,256], g_enc [N,in_ch], grads)`` -- ``grads`` the
    exact-fp32 parameter gradients of ``deform.mlp_param_grads`` over those arrays, as the contract leaves them."""
    with torch.no_grad():
        x, aux, g_heads = x.detach().cpu().float(), aux.detach().cpu().float(), g_heads.detach().cpu().float()
        n, in_ch = x.shape[0], m.input_ch
        W = [layer.weight.detach().cpu().float() for layer in m.linear]
        b = [layer.bias.detach().cpu().float() for layer in m.linear]
        enc = torch.cat([positional_encoding(x, 10), aux.expand(n, -1)], dim=-1)
        hs, h = [], enc
        for l in range(8):
            hs.append(torch.relu(product(h, W[l].t(), terms) + b[l]))
            h = torch.cat([enc, hs[-1]], dim=-1) if l == m.skip_at else hs[-1]
        Wh = torch.cat([hd.weight.detach().cpu().float() for hd in heads_of(m)])
        bh = torch.cat([hd.bias.detach().cpu().float() for hd in heads_of(m)])
        raw = hs[-1] @ Wh.t() + bh  # the forward's head product stays fp32
        g = product(g_heads, Wh, terms)
        G = [None] * 8
        for l in range(7, -1, -1):
            G[l] = torch.where(hs[l] > 0, g, torch.zeros_like(g))
            if l > 0:
                g = product(G[l], W[l][:, in_ch:] if l == m.skip_at + 1 else W[l], terms)
        g_enc = product(G[m.skip_at + 1], W[m.skip_at + 1][:, :in_ch], terms) + product(G[0], W[0], terms)
        H, G = torch.stack(hs), torch.stack(G)
        gW, gb, gWh, gbh = D.mlp_param_grads(enc, H, G, g_heads, head_rows(m))
    return dict(enc=enc, H=H, raw=raw, G=G, g_enc=g_enc, grads=(gW, gb, gWh, gbh))


def clear_rows(m, n=ROWS, pool=POOL, seed=1):
    """``n`` rows ``(x, aux)`` clear of the ReLU's kink by ``MARGIN`` from ``pool`` candidates: ``rows_clear_of_the_kink``
    for the modules it knows (the deformation and control nets), the same rule over the given ``aux`` for the others."""
    x, other, aux = _raw_inputs(m, pool, seed)
    if aux is None:
        ok, aux = rows_clear_of_the_kink(m, x, other, margin=MARGIN), aux_of(m, other)
    else:
        ok = rows_clear_of_the_kink_aux(m, x, aux, margin=MARGIN)
    assert int(ok.sum()) >= n, f"{int(ok.sum())} of {pool} rows clear of the kink, {n} wanted"
    return x[ok][:n].contiguous(), aux[ok][:n].contiguous()


def head_cotangents(m, n, seed=3):
    return torch.randn(n, sum(head_rows(m)), generator=torch.Generator().manual_seed(seed))


def float64_acts(m, x, aux):
    """The eight post-ReLU activations [8,N,256] in float64 on the CPU."""
    lin = [(layer.weight.detach().cpu().double(), layer.bias.detach().cpu().double()) for layer in m.linear]
    with torch.no_grad():
        x, aux = x.detach().cpu().double(), aux.detach().cpu().double()
        inp = torch.cat([positional_encoding(x, 10), aux.expand(x.shape[0], -1)], dim=-1)
        hs, h = [], inp
        for i, (w, b) in enumerate(lin):
            hs.append(torch.relu(h @ w.t() + b))
            h = torch.cat([inp, hs[-1]], dim=-1) if i == m.skip_at else hs[-1]
    return torch.stack(hs)


_CASES = {}


def case(kind, weights="default"):
    """One shared, read-only reference per network: ``dict(m, x, aux, g_heads, ref)`` -- ``ROWS`` filtered rows, fixed head
    cotangents and ``float64_with_input_row`` over them (``ref["H"]``: the activations; ``ref["outs"]``: the module's outputs from the float64 raw heads,
    for the deformation nets with the transformed points appended)."""
    key = (kind, weights)
    if key not in _CASES:
        m = make_net(kind, weights).requires_grad_(False)
        x, aux = clear_rows(m)
        g_heads = head_cotangents(m, x.shape[0])
        ref = float64_with_input_row(m.requires_grad_(True), x, aux, g_heads)
        m.requires_grad_(False)
        ref["H"] = float64_acts(m, x, aux)
        if not kind.startswith("A"):
            outs = tuple(o.detach() for o in outputs_from_raw(m, ref["raw"]))
            ref["outs"] = outs if kind == "control" else (*outs, transform_points(outs[0], x.double()))
        _CASES[key] = dict(m=m, x=x, aux=aux, g_heads=g_heads, ref=ref)
    return _CASES[key]


def trunk_weight_grads(m, grads_by_name):
    """The eight trunk weight gradients out of ``float64_with_input_row``'s ``grads`` (by parameter name)."""
    names = dict((id(p), k) for k, p in m.named_parameters())
    return [grads_by_name[names[id(layer.weight)]] for layer in m.linear]
