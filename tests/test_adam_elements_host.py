"""The Adam restatement (tests/adam_restatement.py) and its regime tensor, checked on the CPU: the float64 restatement is
``torch.optim.Adam(foreach=False)`` in float64 over three steps, every regime is what it is named for, the fp32 yardstick
E32 is finite per (regime, output) at every (step, lr), and the per-element bound the GPU test applies (F x E32, relative
to the output's denominator; tests/parity_common.py has the protocol) catches each wrong restatement on some regime."""
import functools

import torch

import adam_restatement as A
import parity_common as P

N = 7 * 4096


@functools.lru_cache(maxsize=None)
def _tensor():
    return A.regime_tensor(N)


def test_float64_restatement_is_torch_adam_in_float64():
    p0, g, m, v, regime = _tensor()
    gen = torch.Generator().manual_seed(5)
    for lr in A.LRS:
        x = p0.double().clone().requires_grad_(True)
        opt = torch.optim.Adam([x], lr=lr, eps=A.EPS, foreach=False)
        p, m_, v_ = p0.double(), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
        for t in (1, 2, 3):
            grad = (g * (0.5 + torch.rand(N, generator=gen))).double()
            x.grad = grad.clone()
            opt.step()
            out = A.update(p, grad, m_, v_, lr, A.BETA1, A.BETA2, A.EPS, t, torch.float64)
            den = A.denominators(p, grad, m_, v_, out, lr, A.BETA1, A.BETA2, A.EPS, t)
            st = opt.state[x]
            # (p' is rounded once more, to a float64 ulp of p: 2^-52 |p| is 4e-9 of the 2^-24 |p| its denominator counts)
            den["p"] = den["p"] + 2.0**-52 * p.abs() / 1e-12
            for k, got, want in zip(A.OUTPUTS, (x.detach(), st["exp_avg"], st["exp_avg_sq"]), out):
                d = P.distance(got, want, den[k])
                assert float(d.max()) <= 1e-12, (lr, t, k, float(d.max()))
            p, m_, v_ = out


def test_census_every_regime_is_what_it_is_named_for():
    p, g, m, v, regime = _tensor()
    is_ = lambda name: regime == A.REGIMES.index(name)  # noqa: E731
    assert all(int(is_(name).sum()) == 4096 for name in A.REGIMES)
    for name in ("fresh", "fresh_zero_grad", "tiny_grad", "huge_grad"):
        assert bool((m[is_(name)] == 0).all()) and bool((v[is_(name)] == 0).all()), name
    for name in ("warm", "warm_zero_grad", "grad_near_m"):
        assert bool((v[is_(name)] > 0).all()) and bool((m[is_(name)] != 0).all()), name
    gf = g[is_("fresh")].abs()
    assert float(gf.min()) < 1e-7 and float(gf.max()) > 1.0 and bool((gf >= 1e-8).all()) and bool((gf <= 10).all())
    assert bool((g[is_("warm_zero_grad") | is_("fresh_zero_grad")] == 0).all())
    assert bool((g[is_("tiny_grad")].abs() == torch.tensor(1e-20)).all()) and bool((g[is_("huge_grad")].abs() == torch.tensor(1e15)).all())
    near = is_("grad_near_m")
    assert bool((g[near] != m[near]).all()) and bool(((g[near] - m[near]).abs() <= 1.2e-7 * m[near].abs()).all())
    ratio = (g[is_("warm")].abs() / v[is_("warm")].sqrt())
    assert 0.05 < float(ratio.median()) < 5  # a gradient of the moments' scale
    for step in A.STEPS:
        for lr in A.LRS:
            p64, m64, v64 = A.update(p, g, m, v, lr, A.BETA1, A.BETA2, A.EPS, step, torch.float64)
            p32, m32, v32 = A.update(p, g, m, v, lr, A.BETA1, A.BETA2, A.EPS, step, torch.float32)
            # fresh state, zero gradient: exactly p, m' = v' = 0, no NaN (0 / eps)
            z = is_("fresh_zero_grad")
            for pp, mm, vv in ((p64, m64, v64), (p32, m32, v32)):
                assert torch.equal(pp[z], p[z].to(pp.dtype)) and bool((mm[z] == 0).all()) and bool((vv[z] == 0).all())
                assert bool(torch.isfinite(pp).all()) and bool(torch.isfinite(vv).all())
            # the tiny gradient: v' is below the smallest normal float; the update is decided by eps, not by sqrt(v')
            t = is_("tiny_grad")
            assert bool((v64[t] < 2.0**-126).all()) and bool((v64[t] > 0).all())
            s = A.scalars(lr, A.BETA1, A.BETA2, A.EPS, step)
            assert bool((v64[t].sqrt() / s["bc2_sqrt"] < 1e-3 * A.EPS).all())
            assert bool(((p64 - p.double())[t].abs() > 0).all())


def test_yardsticks_are_floored_and_finite():
    p, g, m, v, regime = _tensor()
    for step in A.STEPS:
        for lr in A.LRS:
            _, den, e32 = A.reference(p, g, m, v, regime, lr, step)
            assert {(r, k) for k in e32 for r in e32[k]} == {(r, k) for r in A.REGIMES for k in A.OUTPUTS}
            assert all(bool((d >= 0).all()) for d in den.values())
            for name, k, e in ((name, k, e) for k in e32 for name, e in e32[k].items()):
                # p': the last rounding alone is up to half an ulp of p, which the denominator counts as 2^-24 |p|
                assert A.FLOOR <= e <= (1.0 if k == "p" else (0.02 if name == "tiny_grad" else 1e-6)), (step, lr, name, k, e)


# (mutant, regime, output, steps at which it shows)
MUTANT_CASES = [
    ("bias_corrections_at_step_minus_1", "warm", "p", (1, 2, 1000)),  # (at step 30000 both corrections are 1 to 1e-13)
    ("bias_corrections_at_step_minus_1", "fresh", "p", (1, 2, 1000)),
    ("eps_inside_sqrt", "tiny_grad", "p", A.STEPS),
    ("w2_from_float_beta2", "fresh", "v", A.STEPS),  # 1 - float32(0.999) is 1.3e-5 from 1 - 0.999
    ("m_weighted_by_beta1", "warm", "m", A.STEPS),
    ("m_weighted_by_beta1", "fresh", "m", A.STEPS),
]


def mutant_caps():
    """-> {(mutant, regime, output, step, lr): the largest F at which three quarters of the regime's elements are still
    caught, i.e. at least 4 * F * E32 from the true output}."""
    p, g, m, v, regime = _tensor()
    out = {}
    for mutant, name, k, steps in MUTANT_CASES:
        for step in steps:
            for lr in A.LRS:
                out64, den, e32 = A.reference(p, g, m, v, regime, lr, step)
                i = A.OUTPUTS.index(k)
                xm = A.update(p, g, m, v, lr, A.BETA1, A.BETA2, A.EPS, step, torch.float64, mutant)[i]
                ratios = P.distance(xm, out64[i], den[k])[regime == A.REGIMES.index(name)] / e32[k][name]
                out[(mutant, name, k, step, lr)] = P.three_quarter_cap(ratios)
    return out


def test_every_mutant_is_listed():
    assert {c[0] for c in MUTANT_CASES} == set(A.MUTANTS)


def test_mutants_are_caught_by_the_element_bound():
    """Each mutant is at least 4 * F * E32 away, on three quarters of the elements of some regime, at some (step, lr) the
    GPU test runs: the GPU bound F * E32 has teeth, and this caps F.  (Three quarters, not every element, as in
    tests/test_raster_rows_host.py: looser than "on the elements it concerns".)  Not at every (step, lr): the bias corrections are 1 to
    1e-13 at step 30000, and at the small learning rate an update is below the parameter's own rounding, which p' is
    measured against."""
    caps = mutant_caps()
    best = {}
    for (mutant, name, k, step, lr), c in caps.items():
        if mutant not in best or c > best[mutant][0]:
            best[mutant] = (c, name, k, step, lr)
    for mutant, (c, name, k, step, lr) in best.items():
        shown = sum(1 for key, v in caps.items() if key[0] == mutant and v >= (1.0 if A.F is None else A.F))
        print(f"{mutant}: caps F at {c:.1f} on ({name}, {k}') at step {step}, lr {lr:g}; caught in {shown} of its cells")
    cap = min(v[0] for v in best.values())
    print(f"the cap on F: {cap:.1f}")
    assert cap >= (1.0 if A.F is None else A.F), min(best, key=lambda k: best[k][0])
    # the fresh regime catches w2 = 1 - float32(0.999) at every step and learning rate
    w2 = [v for key, v in caps.items() if key[0] == "w2_from_float_beta2"]
    assert len(w2) == len(A.STEPS) * len(A.LRS) and min(w2) >= (1.0 if A.F is None else A.F)
