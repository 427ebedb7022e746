"""The float64 parity protocol of the per-element and per-row kernel tests (loss, Adam, bilateral-grid slice, raster,
per-Gaussian stage, flow), stated once.  A helper, not a test; plain functions over torch tensors or numpy arrays.

THE PROTOCOL.  A kernel's output x is compared, element by element or row by row, with a float64 restatement x64:

    distance        |x - x64| / den                 den = A64, the element's ABSOLUTE ACCUMULATION: the sum that forms x64 with
                                                    every term by magnitude.  A sum that cancels is wrong at the scale of its
                                                    terms, not of its result.  (The per-Gaussian family passes |g64|: its rows
                                                    do not cancel.)  Rows: the 2-norm of the difference over that of the row of
                                                    denominators.
    E32(regime)     the largest distance of the fp32 restatement (CPU) over the regime's elements -- what plain fp32 arithmetic
                    does there -- FLOORED: where the fp32 restatement happens to be exact, a kernel that contracts an fma or
                    sums in another order is still right.  The floor is the family's (16 * 2^-24; Adam 4 * 2^-24).
    the bound       distance <= F * E32(regime), on the worst element of every regime (``worst_ratios``, ``check``).
    F               4 x the worst ratio (kernel distance / E32) recorded on an MI355X, rounded up to a power of two.  A
                    RECORDING RUN sets it: with the family's F = None, ``bound`` passes everything, the GPU tests run under
                    FG_PARITY_REPORT=<file>, ``check`` records ``ratio|<key>`` and ``e32|<key>`` of every cell, and
                    ``python tests/test_<family>_gpu.py <file>`` prints the table F is read off (kept under profiles/).
    the mutant cap  F must not be so large that the bound has no teeth: the family's host test restates the kernel wrongly
                    on purpose (its MUTANTS) and shows each mutant at least 4 * F * E32 away on three quarters of the elements
                    it concerns.  ``three_quarter_cap``: the largest F at which that still holds; F <= the smallest cap.
    exact zeros     a row whose float64 value is exactly zero must be exactly zero (``exact_zero_rule``); such rows take no part
                    in a regime's maximum, on either side.

REGIMES are ``{name: bool mask}``; an element may lie in several, or in none.  ``masks_of_index`` and ``masks_of_labels`` make
them from an integer regime tensor and from a list of labels.  A mask may cover the leading or the trailing axes of the array
it selects from ([H,W] over [H,W,C] or [C,H,W]; [GL,GY,GX] over [12,GL,GY,GX]).
"""
import json
import math

import numpy as np
import pytest
import torch

import helpers


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    """For the GPU test files to import: there is no CPU fallback to fall back to."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (no CPU fallback exists)")
    from freegaussian_amd import _lib

    _lib.load()


def _f64(a) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().double()
    return torch.from_numpy(np.array(a, dtype=np.float64))  # (a copy: the families' shared arrays are read-only)


def _bool(m) -> torch.Tensor:
    return m if isinstance(m, torch.Tensor) else torch.from_numpy(np.array(m, dtype=bool))


def distance(x, x64, den, rows: bool = False):
    """|x - x64| / den per element -- ``rows``: per row of the first axis, |x - x64|_2 / |den|_2 -- in float64: 0 where the
    difference is exactly zero, inf where only the denominator is zero or x is not finite (x64 too or not).  Torch tensors
    give a tensor, numpy arrays an array."""
    as_numpy = not isinstance(x, torch.Tensor)
    x, x64, den = _f64(x), _f64(x64), _f64(den)
    diff, finite = x - x64, torch.isfinite(x)
    if rows:
        n = x.shape[0]
        diff, den, finite = diff.reshape(n, -1).norm(dim=1), den.reshape(n, -1).norm(dim=1), finite.reshape(n, -1).all(dim=1)
    else:
        diff = diff.abs()
    inf = torch.full_like(diff, math.inf)
    d = torch.where(diff == 0, torch.zeros_like(diff), torch.where(den > 0, diff / den, inf))
    d = torch.where(finite, d, inf)
    return d.numpy() if as_numpy else d


def zero_rows(g64: torch.Tensor) -> torch.Tensor:
    """[N] bool: the rows that are exactly zero (of either sign)."""
    return ~(g64.reshape(g64.shape[0], -1) != 0).any(dim=1)


def exact_zero_rule(x: torch.Tensor, x64: torch.Tensor) -> torch.Tensor:
    """[N] bool, the rows that break the rule: x64 is exactly zero there and x is not (NaN != 0).  ``live_row_masks`` leaves
    the zero rows of x64 out of the regimes."""
    return zero_rows(x64) & (x.reshape(x.shape[0], -1) != 0).any(dim=1)


def masks_of_index(regime: torch.Tensor, names) -> dict:
    """``regime`` holds, per element, an index into ``names``: the masks of the names that occur."""
    return {name: regime == i for i, name in enumerate(names) if bool((regime == i).any())}


def masks_of_labels(labels) -> dict:
    """``labels``: one name per row; the masks in the order of first appearance."""
    return {name: torch.tensor([l == name for l in labels]) for name in dict.fromkeys(labels)}


def restrict(masks: dict, keep) -> dict:
    return {name: m & keep for name, m in masks.items()}


def live_row_masks(labels, x64: torch.Tensor) -> dict:
    """The rows of each label, those whose float64 value is exactly zero left out (the exact-zero rule has them)."""
    return restrict(masks_of_labels(labels), ~zero_rows(x64))


def _select(d: torch.Tensor, mask) -> torch.Tensor:
    """-> (the elements of d under the mask, the mask at d's shape): the mask covers d's leading axes, else its trailing ones."""
    mask = _bool(mask)
    lead = tuple(d.shape[: mask.dim()]) == tuple(mask.shape)
    full = mask.reshape(mask.shape + (1,) * (d.dim() - mask.dim())) if lead else mask
    return (d[mask] if lead else d[..., mask]), full.expand(d.shape)


def yardstick(masks: dict, d32, floor: float) -> dict:
    """E32 per regime: the largest distance of the fp32 restatement over the regime's elements, floored.  A regime without
    elements has nothing above the floor: it is the floor."""
    d32 = _f64(d32)
    out = {}
    for name, mask in masks.items():
        v, _ = _select(d32, mask)
        out[name] = max(float(v.max()) if v.numel() else 0.0, floor)
    return out


def worst_ratios(masks: dict, d, e32: dict) -> dict:
    """Per regime that has elements: (largest d / E32, where) -- ``where`` an index of d (an int if d has one axis).  Anything
    not finite counts as inf."""
    d = _f64(d)
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, math.inf))
    out = {}
    for name, mask in masks.items():
        v, full = _select(d, mask)
        if not v.numel():
            continue
        at = int(torch.where(full, d, torch.full_like(d, -1.0)).argmax())
        where = tuple(int(i) for i in np.unravel_index(at, tuple(d.shape)))
        out[name] = (float(d.reshape(-1)[at]) / e32[name], where[0] if d.dim() == 1 else where)
    return out


def bound(ratio: float, F) -> bool:
    """The bound, or with F = None no bound: the recording run F is set from."""
    return F is None or ratio <= F


def check_cell(key: str, ratio: float, e32: float, F, failures: list, what: str = "", depth: int = 2) -> None:
    """One cell: ``ratio|key`` and ``e32|key`` are recorded first (against the line ``depth`` frames up: the caller's), then
    the bound is applied."""
    helpers._record(f"ratio|{key}", ratio, depth)
    helpers._record(f"e32|{key}", e32, depth)
    if not bound(ratio, F):
        failures.append(f"{key.replace('|', ' ')}: {what + ' ' if what else ''}is {ratio * e32:.3e} of its denominator from float64 = "
                        f"{ratio:.1f} x E32 ({e32:.3e}); the bound is {F:g} x")  # fmt: skip


def check(key: str, masks: dict, d, e32: dict, F, failures: list, depth: int = 2) -> None:
    """Every regime's worst element against F * E32: ``key`` is the cell's record key with ``{regime}`` where the regime's
    name goes."""
    for name, (ratio, at) in worst_ratios(masks, d, e32).items():
        check_cell(key.format(regime=name), ratio, e32[name], F, failures, f"element {at}", depth + 1)


def three_quarter_cap(ratios) -> float:
    """``ratios``: distance / E32 of the elements a mutant concerns.  The largest F at which three quarters of them (rounded
    up, at least one) are still 4 * F * E32 away; 0 without elements."""
    ratios = _f64(ratios).reshape(-1)
    if not ratios.numel():
        return 0.0
    k = max(-(-3 * ratios.numel() // 4), 1)
    return float(torch.sort(ratios, descending=True).values[k - 1]) / 4


def read_records(path: str, test_file: str):
    """-> (ratio, e32): the ``ratio|...`` and ``e32|...`` records that the tests of ``test_file`` left in an FG_PARITY_REPORT
    file, keyed by the tuple of the key's fields; the largest value where a key repeats."""
    ratio, e32 = {}, {}
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            kind, *key = r["kind"].split("|")
            if kind in ("ratio", "e32") and test_file in r.get("test", ""):
                d = ratio if kind == "ratio" else e32
                d[tuple(key)] = max(d.get(tuple(key), 0.0), r["value"])
    return ratio, e32
