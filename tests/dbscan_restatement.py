"""The definition of ``fg_dbscan`` (include/fgraster.h, "DB") on the CPU: numpy fp32, brute force over all pairs in row
chunks, neighbour LISTS (never a dense [n,n] matrix).

    dx = x_i - x_j (y, z alike), d2 = (dx dx + dy dy) + dz dz in fp32, eps2 = eps * eps in fp32
    j neighbours i  iff  d2 <= eps2   (symmetric; a finite row neighbours itself; a non-finite row neighbours nobody)
    core(i)         iff  at least min_samples neighbours, the row itself counted
    clusters        =    connected components of the core rows, numbered by ascending lowest core row
    border row      =    non-core with a core neighbour: the lowest-numbered cluster among its core neighbours
    everything else =    -1

The neighbour lists depend on (x, eps) alone: ``neighbour_lists`` once, ``labels_from_lists`` per ``min_samples``."""
from __future__ import annotations

import numpy as np


def neighbour_lists(x, eps, want_gap: bool = False, chunk_pairs: int = 1 << 24):
    """-> (indptr int64 [n+1], indices int64 [nnz], gap): row i's neighbours are indices[indptr[i]:indptr[i+1]], ascending.
    gap (``want_gap``; else None) = the smallest | |x_i - x_j| - eps | / eps over all pairs i != j of finite rows, in float64
    (inf when there is no such pair): how far the data are from the rounding edge of eps."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    assert x.ndim == 2 and x.shape[1] == 3
    n = x.shape[0]
    e = np.float32(eps)
    eps2 = np.float32(e * e)
    x64 = x.astype(np.float64)
    finite = np.isfinite(x).all(axis=1)
    rows_per = max(1, chunk_pairs // max(n, 1))
    counts = np.zeros(n, dtype=np.int64)
    parts = []
    gap = np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, n, rows_per):
            b = min(n, a + rows_per)
            dx = x[a:b, None, 0] - x[None, :, 0]
            dy = x[a:b, None, 1] - x[None, :, 1]
            dz = x[a:b, None, 2] - x[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            near = d2 <= eps2  # (a NaN compares False)
            r, c = np.nonzero(near)
            counts[a:b] = np.bincount(r, minlength=b - a)
            parts.append(c.astype(np.int64))
            if want_gap:
                d = np.sqrt(((x64[a:b, None, :] - x64[None, :, :]) ** 2).sum(axis=2))
                g = np.abs(d - float(e)) / float(e)
                g[np.arange(b - a), np.arange(a, b)] = np.inf  # i == j
                g[~finite[a:b], :] = np.inf
                g[:, ~finite] = np.inf
                gap = min(gap, float(g.min()))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    indices = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return indptr, indices, (gap if want_gap else None)


def _segment_min(values, seg_len):
    """min of each of the consecutive NON-EMPTY segments of ``values`` (lengths ``seg_len`` > 0)."""
    starts = np.zeros(seg_len.shape[0], dtype=np.int64)
    np.cumsum(seg_len[:-1], out=starts[1:])
    return np.minimum.reduceat(values, starts)


def labels_from_lists(indptr, indices, min_samples: int):
    """-> (labels int32 [n], core bool [n], K)."""
    n = indptr.shape[0] - 1
    deg = np.diff(indptr)
    core = deg >= int(min_samples)
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    # components of the core rows: every core row's label -> the minimum over its core neighbours (itself among them),
    # then pointer jumping, until nothing moves; the fixed point is the lowest core row of the component
    lab = np.arange(n, dtype=np.int64)
    cc = core[src] & core[indices]
    cc_dst = indices[cc]
    cc_len = np.bincount(src[cc], minlength=n)[core]
    core_rows = np.nonzero(core)[0]
    while core_rows.size:
        new = lab.copy()
        new[core_rows] = _segment_min(lab[cc_dst], cc_len)
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, lab):
            break
        lab = new
    roots = np.unique(lab[core_rows])  # ascending lowest core row = the cluster numbers
    labels = np.full(n, -1, dtype=np.int32)
    labels[core_rows] = np.searchsorted(roots, lab[core_rows]).astype(np.int32)
    # border rows: the lowest-numbered cluster (= the lowest root) among the core neighbours
    bc = ~core[src] & core[indices]
    if bc.any():
        b_len = np.bincount(src[bc], minlength=n)
        b_rows = np.nonzero(b_len)[0]
        labels[b_rows] = np.searchsorted(roots, _segment_min(lab[indices[bc]], b_len[b_rows])).astype(np.int32)
    return labels, core, int(roots.size)


def dbscan(x, eps, min_samples: int = 4, want_gap: bool = False):
    """-> (labels int32 [n], core bool [n], K, gap or None)."""
    indptr, indices, gap = neighbour_lists(x, eps, want_gap=want_gap)
    labels, core, k = labels_from_lists(indptr, indices, min_samples)
    return labels, core, k, gap


def shared_border_case():
    """-> (x float32 [19,3], eps, min_samples, lone row): two 3 x 3 grids of spacing 0.1, the FAR one (x in 1.6 .. 1.8) in
    rows 0..8, the near one (x in 0 .. 0.2) in rows 9..17, and a lone point at (0.9, 0.1, 0) in row 18.  At eps 0.75 it has
    three neighbours in each grid (the column 0.7 away: 0.7, 0.707, 0.707) and itself: 7 < 8, a border row of both."""
    g = np.array([[i * 0.1, j * 0.1, 0.0] for i in range(3) for j in range(3)])
    x = np.concatenate([g + [1.6, 0.0, 0.0], g, [[0.9, 0.1, 0.0]]]).astype(np.float32)
    return x, 0.75, 8, 18


def permute_lists(indptr, indices, perm):
    """The neighbour lists of x[perm] from those of x (new row r is old row perm[r]): no second pass over the pairs."""
    n = indptr.shape[0] - 1
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n, dtype=np.int64)
    src = inv[np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))]
    order = np.argsort(src, kind="stable")
    new_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=new_ptr[1:])
    return new_ptr, inv[indices][order]


def renumber_by_lowest_core_row(labels, core):
    """The labels of the CORE rows with the clusters numbered anew by ascending lowest core row (-1 elsewhere): what a
    permutation of the rows does to the numbering.  (A border row between two clusters follows the numbering, so its
    cluster may change under a permutation: the core rows' partition is what is invariant.)"""
    labels, core = np.asarray(labels), np.asarray(core, dtype=bool)
    out = np.full(labels.shape, -1, dtype=np.int64)
    seen = {}
    for i in np.nonzero(core)[0].tolist():
        out[i] = seen.setdefault(int(labels[i]), len(seen))
    return out
