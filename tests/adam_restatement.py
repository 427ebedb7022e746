"""Plain-torch restatement of one Adam update (csrc/adam.hip: fg_adam_step, fg_adam_step_multi) as a map
(p, g, m, v, lr, beta1, beta2, eps, step) -> (p', m', v') in any dtype, on one tensor of labelled elements.  A helper, not a
test; nothing of the package under test is imported here.

    scalars(...)        the step-dependent scalars in Python doubles, exactly as ``adam_scalars`` and torch form them
    update(...)         the update; the fp32 variant rounds the scalars to float as the kernel does, the float64 variant
                        takes the fp32 inputs exactly and the scalars as doubles
    denominators(...)   per element, what each output's distance is relative to:
                            m'   |m| + w1 (|g| + |m|)
                            v'   v'64  (all terms are positive)
                            p'   |delta64| + 2^-24 |p|
    regime_tensor(n)    p, g, m, v [n] fp32 and the regime of every element (element i has regime i mod 7)
    MUTANTS             wrong restatements (float64, CPU only: they prove that the bound has teeth)

ELEMENT DISTANCE.  |x - x64| / denominator.  m' = m + w1 (g - m) cancels where g is close to m; p' is p plus an update that
is far below p's own rounding when the learning rate is small.  tests/parity_common.py has the protocol.
"""
import math
from typing import Dict, Optional, Tuple

import torch

import parity_common as P

# Floor of the fp32 yardstick E32.  The other suites floor theirs at 16 * 2^-24: their rows are sums of hundreds of terms.
# Here an output is an elementwise expression of two to ten roundings, the fp32 restatement is often exact to the last
# bit (E32 = 0), and what the kernel may do differently is contract a product into an fma, twice per output at the most
# (m' and v' are one fma each, p' is one more): each contraction removes one rounding of at most 2^-24 relative, and a
# second one may follow from the changed operand.  4 * 2^-24.
FLOOR = 4 * 2.0**-24
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15  # torch's betas; the eps the reference's method config attaches to every group
STEPS = (1, 2, 1000, 30000)
LRS = (1.6e-4, 1.6e-6)

# The GPU bound is F * E32(regime, output).  Set from the MI355X run recorded in profiles/loss_adam_flow_parity.md: 4 x the
# worst recorded ratio (HIP distance) / E32 = 4 x 1.00, a power of two already; capped by the host test's mutant assertion
# (F <= 13: w2 = 1 - float32(0.999) on the fresh regime).  None: record only (how the run F was set from was made).
F: Optional[float] = 4.0

REGIMES = ("fresh", "warm", "warm_zero_grad", "fresh_zero_grad", "tiny_grad", "huge_grad", "grad_near_m")
OUTPUTS = ("p", "m", "v")
MUTANTS = ("bias_corrections_at_step_minus_1", "eps_inside_sqrt", "w2_from_float_beta2", "m_weighted_by_beta1")


def scalars(lr: float, beta1: float, beta2: float, eps: float, step: int, mutant: Optional[str] = None) -> Dict[str, float]:
    t = step - 1 if mutant == "bias_corrections_at_step_minus_1" else step
    bc1, bc2 = 1.0 - beta1**t, 1.0 - beta2**t
    if t == 0:  # (the mutant at step 1: no correction at all)
        bc1 = bc2 = 1.0
    w2 = 1.0 - beta2
    if mutant == "w2_from_float_beta2":
        w2 = 1.0 - float(torch.tensor(beta2, dtype=torch.float32))
    return dict(neg_step=-(lr / bc1), bc2_sqrt=math.sqrt(bc2), w1=1.0 - beta1, w2=w2, beta2=beta2, eps=eps)


def update(p, g, m, v, lr, beta1, beta2, eps, step, dtype, mutant: Optional[str] = None):
    """-> (p', m', v') in ``dtype``; the operations and their order are the kernel's ``adam1``."""
    s = scalars(lr, beta1, beta2, eps, step, mutant)
    s = {k: torch.tensor(x, dtype=dtype) for k, x in s.items()}  # (fp32: rounded to float, as the kernel's arguments are)
    p, g, m, v = (t.detach().cpu().to(dtype) for t in (p, g, m, v))
    w1 = (1.0 - s["w1"]) if mutant == "m_weighted_by_beta1" else s["w1"]
    m = m + w1 * (g - m)
    v = v * s["beta2"] + (s["w2"] * g) * g
    if mutant == "eps_inside_sqrt":
        denom = torch.sqrt(v + s["eps"]) / s["bc2_sqrt"]
    else:
        denom = torch.sqrt(v) / s["bc2_sqrt"] + s["eps"]
    p = p + s["neg_step"] * (m / denom)
    return p, m, v


def denominators(p, g, m, v, out64, lr, beta1, beta2, eps, step) -> Dict[str, torch.Tensor]:
    p, g, m, v = (t.detach().cpu().double() for t in (p, g, m, v))
    w1 = 1.0 - beta1
    p64, m64, v64 = out64
    return dict(m=m.abs() + w1 * (g.abs() + m.abs()), v=v64, p=(p64 - p).abs() + 2.0**-24 * p.abs())


def regime_tensor(n: int, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> p, g, m, v [n] float32, regime [n] long (= i mod 7: every size from 7 elements on holds every regime)."""
    gen = torch.Generator().manual_seed(4000 + seed)
    U = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=gen)  # noqa: E731
    N = lambda: torch.randn(n, generator=gen)  # noqa: E731
    sign = lambda: torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)  # noqa: E731
    regime = torch.arange(n) % len(REGIMES)
    is_ = lambda name: regime == REGIMES.index(name)  # noqa: E731
    p = N()
    scale = 10.0 ** U(-6.0, 0.0)  # the scale of a warm element's gradients
    m, v = N() * scale, scale * scale * U(0.5, 2.0)
    g = N() * scale  # warm: a gradient of the moments' scale
    zero = torch.zeros(n)
    fresh = is_("fresh") | is_("fresh_zero_grad") | is_("tiny_grad") | is_("huge_grad")
    m, v = torch.where(fresh, zero, m), torch.where(fresh, zero, v)
    g = torch.where(is_("fresh"), sign() * 10.0 ** U(-8.0, 1.0), g)
    g = torch.where(is_("warm_zero_grad") | is_("fresh_zero_grad"), zero, g)
    g = torch.where(is_("tiny_grad"), sign() * 1e-20, g)
    # (the update eps decides there is lr * 1e-6 at the most: a parameter near zero, so that it is above p's own rounding)
    p = torch.where(is_("tiny_grad"), 1e-6 * p, p)
    g = torch.where(is_("huge_grad"), sign() * 1e15, g)
    up = torch.where(torch.rand(n, generator=gen) < 0.5, math.inf, -math.inf)
    g = torch.where(is_("grad_near_m"), torch.nextafter(m, up), g)  # one ulp from m: g - m is exact and tiny
    return p.contiguous(), g.contiguous(), m.contiguous(), v.contiguous(), regime


def reference(p, g, m, v, regime, lr, step, beta1=BETA1, beta2=BETA2, eps=EPS):
    """-> (out64, denominators, E32[output][regime]) of one update of the given pre-state."""
    out64 = update(p, g, m, v, lr, beta1, beta2, eps, step, torch.float64)
    out32 = update(p, g, m, v, lr, beta1, beta2, eps, step, torch.float32)
    den = denominators(p, g, m, v, out64, lr, beta1, beta2, eps, step)
    masks = P.masks_of_index(regime, REGIMES)
    d32 = {k: P.distance(x32, x64, den[k]) for k, x32, x64 in zip(OUTPUTS, out32, out64)}
    return out64, den, {k: P.yardstick(masks, d32[k], FLOOR) for k in OUTPUTS}
