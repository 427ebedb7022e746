"""The four operations of the fused stage-2 control stage (csrc/control.hip, include/fgraster.h section CT) restated on the CPU,
in float64 and in the kernels' own fp32 order, the cases the tests run them on, and the bounds.  A helper, not a test.

The bounds are derived, not measured:

    attribute mean   |x - x64| <= 2^-23 |x64| + n 2^-52 A64      x64: the float64 mean of the SAME fp32 differences, A64: the mean
                     of |difference| over the attribute.  The first term is the one rounding of the quotient to fp32 (2^-24,
                     doubled); the second is a float64 sum of at most n terms in any order ((n - 1) 2^-53 of the sum of
                     magnitudes, doubled, divided by the count), which also covers x64's own sum.
    value rows       |x - x64| <= (p + 1) 2^-24 S / p            p = popcount, S = the sum of |d_avg[m]| over the set bits: p - 1
                     fp32 additions of partial sums no larger than S, one division, and one unit to spare.
"""
import torch

M_MAX = 32


def mask_of_bits(bits: torch.Tensor, M: int) -> torch.Tensor:
    """bool [n,M] of integer words [n] (any integer type; bit m -> column m)."""
    words = bits.to(torch.int64) & 0xFFFFFFFF
    return ((words[:, None] >> torch.arange(M, dtype=torch.int64)) & 1).bool()


def plan_brute(mask: torch.Tensor):
    """The plan's four arrays by loops over the rows of a CPU bool mask [N,M]: (sel_index, bits, rank, counts) as lists."""
    N, M = mask.shape
    rows = mask.tolist()
    sel, bits, rank, counts = [], [], [-1] * N, [0] * M
    for r, row in enumerate(rows):
        word = 0
        for m, on in enumerate(row):
            if on:
                word |= 1 << m
                counts[m] += 1
        if word:
            rank[r] = len(sel)
            sel.append(r)
            bits.append(word)
    return sel, bits, rank, counts


def attr_mean64(a: torch.Tensor, b: torch.Tensor, pmask: torch.Tensor):
    """(x64 [M,3], A64 [M,3]) of fp32 ``a``, ``b`` [n,3] and bool ``pmask`` [n,M]: the difference in fp32, the rest in float64."""
    delta = (a.float() - b.float()).double()
    w = pmask.double()
    counts = w.sum(0)[:, None]
    return w.t() @ delta / counts, w.t() @ delta.abs() / counts


def attr_mean_bound(x64: torch.Tensor, A64: torch.Tensor, n: int) -> torch.Tensor:
    return 2.0**-23 * x64.abs() + n * 2.0**-52 * A64


def attr_mean_torch(a: torch.Tensor, b: torch.Tensor, pmask: torch.Tensor) -> torch.Tensor:
    """The torch statement (model.py, the unset path)."""
    delta = a - b
    return torch.stack([delta[pmask[:, i]].mean(0) for i in range(pmask.shape[1])])


def value_rows64(pmask: torch.Tensor, d_avg: torch.Tensor):
    """(x64 [n,3], S / p [n,3]) of fp32 ``d_avg`` [M,3]."""
    w, p = pmask.double(), pmask.sum(-1, keepdim=True).double()
    return w @ d_avg.double() / p, w @ d_avg.double().abs() / p


def value_rows_bound(pmask: torch.Tensor, s_over_p: torch.Tensor) -> torch.Tensor:
    return (pmask.sum(-1, keepdim=True).double() + 1) * 2.0**-24 * s_over_p


def value_rows32(pmask: torch.Tensor, d_avg: torch.Tensor) -> torch.Tensor:
    """The kernel's order in fp32: the set bits' rows of ``d_avg`` added in ascending m, then one division."""
    s = torch.zeros(pmask.shape[0], 3, dtype=torch.float32)
    for m in range(pmask.shape[1]):
        s = torch.where(pmask[:, m : m + 1], s + d_avg[m].float(), s)
    return s / pmask.sum(-1, keepdim=True).float()


def value_rows_torch(pmask: torch.Tensor, d_avg: torch.Tensor) -> torch.Tensor:
    """The torch statement."""
    return pmask.float() @ d_avg / pmask.sum(-1, keepdim=True)


def scatter_torch(sel_index64: torch.Tensor, means, d_xyz, d_rot, d_scale):
    """The torch statement: ``zeros_like().index_put`` of each head, and the means moved."""
    idx = (sel_index64,)
    N = means.shape[0]
    return (means + torch.zeros_like(means).index_put(idx, d_xyz), means.new_zeros(N, 4).index_put(idx, d_rot),
            means.new_zeros(N, 3).index_put(idx, d_scale))  # fmt: skip


# ---------------------------------------------------------------------------------------------------------------------
# cases

MEAN_ROWS = (1, 63, 64, 65, 257, 4097, 70_001)  # a wave, a workgroup's 1024 rows and 69 partial blocks are crossed
MEAN_ATTRS = (1, 3, 32)
SCATTER_ROWS = (1, 64, 65, 257, 4096)


def mean_case(n: int, M: int):
    """fp32 ``a``, ``b`` [n,3] and a bool ``pmask`` [n,M] in which every row has an attribute, attribute 0 has all rows, the
    last one (M > 1) a single row, and the ones between about 40 % of the rows (never none): rows lie in several."""
    g = torch.Generator().manual_seed(1000 * M + n)
    pmask = torch.zeros(n, M, dtype=torch.bool)
    pmask[:, 0] = True
    if M > 1:
        pmask[n // 2, M - 1] = True
    if M > 2:
        pmask[:, 1 : M - 1] = torch.rand(n, M - 2, generator=g) < 0.4
        pmask[0, 1 : M - 1] = True
    b = torch.rand(n, 3, generator=g) * 2 - 1
    # a displacement per attribute and a per-row part of both signs: the means cancel partly, as real ones do
    a = b + 0.05 * torch.randn(n, 3, generator=g) + 0.02 * (pmask.float() @ torch.randn(M, 3, generator=g))
    return a, b, pmask


def bits_of_mask(pmask: torch.Tensor) -> torch.Tensor:
    """uint32 words [n] of a bool [n,M]."""
    M = pmask.shape[1]
    words = (pmask.to(torch.int64) << torch.arange(M, dtype=torch.int64)).sum(-1)
    return torch.where(words >= 2**31, words - 2**32, words).to(torch.int32).view(torch.uint32)


def scatter_mask(N: int, sparse: bool) -> torch.Tensor:
    """bool [N,3]: every row selected, or (``sparse``) every seventh row and the last; each attribute has a row."""
    mask = torch.zeros(N, 3, dtype=torch.bool)
    rows = torch.arange(N)
    pick = (rows % 7 == 3) | (rows == N - 1) if sparse else torch.ones(N, dtype=torch.bool)
    mask[:, 0] = pick
    mask[:, 1] = pick & (rows % 2 == 0)
    mask[:, 2] = pick & (rows % 3 == 0)
    first = int(pick.nonzero()[0])
    mask[first] = True
    return mask


def scatter_case(N: int, sparse: bool):
    """(mask [N,3], means [N,3], heads [n,10], upstream gradients of the three outputs) in fp32, seeded."""
    g = torch.Generator().manual_seed(7 * N + int(sparse))
    mask = scatter_mask(N, sparse)
    n = int(mask.any(-1).sum())
    means, heads = torch.randn(N, 3, generator=g), torch.randn(n, 10, generator=g)
    ups = (torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g), torch.randn(N, 3, generator=g))
    return mask, means, heads, ups
