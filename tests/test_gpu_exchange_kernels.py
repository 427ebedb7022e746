"""The device kernels of the view-sharded gradient exchange, one process, no collectives: the gathered blocks are built
by hand and every output row is compared with a float64 statement of the same sum (tests/exchange_restatement.py).

    fg_sh_grad_accumulate / fg_sh_grad_accumulate_split   (csrc/sh.hip, one kernel)      test 1, test 2, test 3
    fg_preprocess_bwd_factored / fg_preprocess_raw_bwd_factored (csrc/preprocess.hip)     test 2
    fg_payload_compact / fg_payload_expand                (csrc/sh.hip)                   test 3

The kernels are called as viewdp.py calls them: ``_lib.load().fg_...`` with ``data_ptr()``s, wrapped in ``_lib.check``.

PARAMETER SET of test 1 -- the full cross product (2496 kernel calls, 20 pytest cases of 48-192 calls each):
    entry point   flat (fg_sh_grad_accumulate, [N,k_stored,3]) | split (features_dc [N,3] + features_rest [N,k_stored-1,3],
                  two allocations; k_stored = 1: v_features_rest = NULL)
    k_stored      1, 4, 9, 12, 16            degree   every 0..3 with (degree+1)^2 <= k_stored
    payload       3 (g | camera position) | 6 (g, carried direction)
    n_views       1, 3, 8                    scale    1, 1/n_views
    N             1, BLOCK-1, BLOCK, BLOCK+1, 255, 256, 257, 1000   (BLOCK = the workgroup's rows, read from the sources)
  and, cycled through inside the product so that every (N, k_stored, entry point, payload) meets each value:
    view_stride   minimum + 0 | 1 | 5 floats, the padding NaN
    output        at float offset 0 | 3 of its allocation (16-byte aligned: the float4 store paths of lds_to_slab_at;
                  not aligned: its scalar path -- FlatGaussianParams' colour block starts at float 11 N of the flat buffer)
"""
import functools
import os
import re

import pytest
import torch

import helpers
from exchange_restatement import compact, forward_magnitude64, rebuild, rebuild64, row_error_ratio
from freegaussian_amd import _lib, ops
from freegaussian_amd.scenes import synthetic_scene

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
GUARD = 64  # floats of NaN behind every output: nothing may be written past the end
SENTINEL = 0x5EA7BEEF  # the bit pattern blocks are pre-filled with in test 3 (a finite float, no row id, no count)

# Per-row bound:  || v_hip[i] - v64[i] ||  <=  TOL * |scale| * sum_v || basis(dir_v(i)) || || g_v[i] ||
# The same sum in float32 on the CPU in plain torch (exchange_restatement.rebuild(..., dtype=torch.float32)) against the
# float64 restatement, worst row over the whole parameter set of test 1 (`python tests/test_gpu_exchange_kernels.py`
# with the repository on PYTHONPATH prints it; payload 3: 3.31e-7, payload 6: 2.08e-7):   CPU_F32_WORST = 3.31e-7
# x 4 (1/sqrtf against torch's division, another association of the basis polynomials)   ->   TOL = 1.324e-6
# The HIP kernels' own worst ratio over the same set (MI355X):                            HIP_WORST = 3.46e-7
# (flat and split alike, payload 3, degree 3; payload 6: 1.81e-7; the rebuild of a real factored g in test 2: 3.41e-7).
# One coefficient of one row of the HIP output times (1 + 1e-4) fires the row assertion (the row's largest coefficient:
# in every case of four (entry point, k_stored, payload) groups; its first non-zero one: in 616 of 624 cases).
CPU_F32_WORST = 3.31e-7
TOL = 4 * CPU_F32_WORST
HIP_WORST = 3.46e-7  # (a record, not used by any assertion)
TINY = float(torch.finfo(torch.float32).tiny)

K_STORED = (1, 4, 9, 12, 16)
DEGREES = (0, 1, 2, 3)
N_VIEWS = (1, 3, 8)
PADS = (0, 1, 5)
OFFSETS = (0, 3)


def _block_rows():
    """BLOCK of csrc/sh.hip (rows per workgroup of the rebuild): `constexpr int BLOCK = ...` in sh.hip or a header it
    includes, through one #define if it names one."""
    csrc = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
    todo, seen, text = ["sh.hip"], set(), ""
    while todo:
        name = todo.pop()
        if name in seen or not os.path.exists(os.path.join(csrc, name)):
            continue
        seen.add(name)
        with open(os.path.join(csrc, name)) as f:
            src = f.read()
        text += src
        todo += re.findall(r'#include\s+"([^"]+)"', src)
    value = re.search(r"constexpr\s+int\s+BLOCK\s*=\s*(\w+)\s*;", text).group(1)
    if not value.isdigit():
        value = re.search(r"#define\s+" + value + r"\s+(\d+)", text).group(1)
    return int(value)


BLOCK = _block_rows()
NS = tuple(sorted({1, BLOCK - 1, BLOCK, BLOCK + 1, 255, 256, 257, 1000}))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (no CPU fallback exists)")
    _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- inputs of the rebuild (CPU, seeded; shared by the GPU test and the CPU float32 measurement) --------------------------
@functools.lru_cache(maxsize=None)
def _rebuild_inputs(n, n_views, pf):
    """-> means [n,3], [(g_v [n,3], camera position [3] | unit direction [n,3]) per view], float32 on the CPU.
    Means uniform in the cube [-1,1]^3; cameras 2 (one cube edge) to 4 away from the cube's circumscribed sphere;
    g = randn * 10^U(-4,1); about 40 % of the (view, row) pairs all zero; rows i % 7 == 3 zero in every view; rows
    i % 5 == 1 with one non-zero channel; the directions of all-zero rows are NaN (the kernel must not look at them)."""
    gen = torch.Generator().manual_seed(1000 * n + 10 * n_views + pf)
    means = torch.rand(n, 3, generator=gen) * 2 - 1
    rows = torch.arange(n)
    views = []
    for v in range(n_views):
        g = torch.randn(n, 3, generator=gen) * 10 ** (torch.rand(n, 1, generator=gen) * 5 - 4)
        one = (rows % 5 == 1)[:, None] & (torch.arange(3)[None, :] != (rows % 3)[:, None])
        g = torch.where(one, torch.zeros(()), g)
        dead = (torch.rand(n, generator=gen) < 0.4) | (rows % 7 == 3)
        if v == 0:
            dead[0] = False  # (N = 1 is not an all-zero case)
        g = torch.where(dead[:, None], torch.zeros(()), g)
        away = torch.nn.functional.normalize(torch.randn(3, generator=gen), dim=0)
        cam = away * (3.0**0.5 + 2.0 + 2.0 * float(torch.rand((), generator=gen)))
        if pf == 3:
            views.append((g, cam))
        else:  # every view saw its own (deformed) positions: the direction is carried, rounded to fp32
            d = torch.nn.functional.normalize(means + 0.05 * torch.randn(n, 3, generator=gen) - cam, dim=1)
            views.append((g, torch.where(dead[:, None], torch.full((), NAN), d)))
    return means, views


def _dense_blocks(views, n, pf, pad, fill=NAN):
    """The gathered dense payload as fg_sh_grad_accumulate reads it: one block per view, view_stride floats apart."""
    stride = (3 * n + 3 if pf == 3 else 6 * n) + pad
    payload = torch.full((len(views) * stride,), fill, dtype=torch.float32)
    for v, (g, second) in enumerate(views):
        blk = payload[v * stride : (v + 1) * stride]
        if pf == 3:
            blk[: 3 * n] = g.reshape(-1)
            blk[3 * n : 3 * n + 3] = second
        else:
            blk[: 6 * n] = torch.cat([g, second], dim=1).reshape(-1)
    return payload, stride


def _guarded(numel, offset=0):
    """A NaN-filled allocation of offset + numel + GUARD floats -> (whole, the numel floats the kernel may write)."""
    whole = torch.full((offset + numel + GUARD,), NAN, device=DEV, dtype=torch.float32)
    return whole, whole[offset : offset + numel]


def _untouched(whole, offset, numel):
    return bool(whole[:offset].isnan().all()) and bool(whole[offset + numel :].isnan().all())


def _hip_rebuild(entry, n, n_views, degree, k, means_dev, payload_dev, stride, pf, scale, offset=0):
    """One call of the rebuild -> v [n,k,3] on the CPU.  Outputs are NaN before the call, must be NaN-free after it and
    the floats around them must still be NaN."""
    lib = _lib.load()
    mp = means_dev.data_ptr() if means_dev is not None else None
    if entry == "flat":
        whole, out = _guarded(n * k * 3, offset)
        _lib.check(lib.fg_sh_grad_accumulate(n, n_views, degree, k, mp, payload_dev.data_ptr(), stride, pf, scale,
                                             out.data_ptr(), _stream()), "fg_sh_grad_accumulate")  # fmt: skip
        assert _untouched(whole, offset, n * k * 3), "written outside [N,k_stored,3]"
        v = out.view(n, k, 3).cpu()
    else:
        whole_dc, dc = _guarded(n * 3, offset)
        whole_rest, rest = _guarded(n * (k - 1) * 3, offset) if k > 1 else (None, None)
        _lib.check(lib.fg_sh_grad_accumulate_split(
            n, n_views, degree, k, mp, payload_dev.data_ptr(), stride, pf, scale, dc.data_ptr(),
            rest.data_ptr() if k > 1 else None, _stream()), "fg_sh_grad_accumulate_split")  # fmt: skip
        assert _untouched(whole_dc, offset, n * 3), "written outside features_dc [N,3]"
        v = dc.view(n, 1, 3).cpu()
        if k > 1:
            assert _untouched(whole_rest, offset, n * (k - 1) * 3), "written outside features_rest [N,k_stored-1,3]"
            v = torch.cat([v, rest.view(n, k - 1, 3).cpu()], dim=1)
    assert not bool(v.isnan().any()), "a NaN is left in the output"
    return v


def _assert_rows(v, v64, magnitude, degree, what):
    """The per-row bound, exact zeros where nothing is summed, exact zeros in the unused columns -> worst ratio."""
    err = (v.double() - v64).flatten(1).norm(dim=1)
    bound = TOL * magnitude + TINY
    worst = int((err - bound).argmax())
    assert bool((err <= bound).all()), f"{what}: row {worst}: error {float(err[worst]):.3e} > bound {float(bound[worst]):.3e}"
    nothing = magnitude == 0
    assert bool((v[nothing] == 0).all()), f"{what}: a row without any gradient is not exactly zero"
    assert bool((v[:, (degree + 1) ** 2 :] == 0).all()), f"{what}: a column beyond (degree+1)^2 is not exactly zero"
    return row_error_ratio(v, v64, magnitude)


def _cases_of(k):
    """(degree, n_views, N, scale, view-stride padding, output offset) of test 1 for one k_stored."""
    for i_d, degree in enumerate(d for d in DEGREES if (d + 1) ** 2 <= k):
        for i_v, n_views in enumerate(N_VIEWS):
            for i_n, n in enumerate(NS):
                for i_s, scale in enumerate((1.0, 1.0 / n_views)):
                    yield degree, n_views, n, scale, PADS[(i_n + i_v + i_d) % 3], OFFSETS[(i_n + i_s + i_d) % 2]


# ---- test 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pf", [3, 6])
@pytest.mark.parametrize("k", K_STORED)
@pytest.mark.parametrize("entry", ["flat", "split"])
def test_rebuild_equals_the_float64_sum_row_by_row(entry, k, pf):
    """fg_sh_grad_accumulate (flat) / fg_sh_grad_accumulate_split against rebuild64, every row on its own, over the
    parameter set of the module docstring.  Worst ratio error / forward magnitude of the HIP kernel: HIP_WORST."""
    worst = 0.0
    for degree, n_views, n, scale, pad, offset in _cases_of(k):
        means, views = _rebuild_inputs(n, n_views, pf)
        payload, stride = _dense_blocks(views, n, pf, pad)
        v = _hip_rebuild(entry, n, n_views, degree, k, means.to(DEV), payload.to(DEV), stride, pf, scale, offset)
        v64 = rebuild64(means, views, degree, k, scale, pf)
        magnitude = forward_magnitude64(means, views, degree, scale, pf)
        what = f"{entry} k_stored={k} pf={pf} degree={degree} n_views={n_views} N={n} scale={scale:g} pad={pad} offset={offset}"
        worst = max(worst, _assert_rows(v, v64, magnitude, degree, what))
    helpers._record("row_error_ratio", worst, depth=1)
    print(f"rebuild {entry} k_stored={k} pf={pf}: worst row error / forward magnitude {worst:.3e} (TOL {TOL:.3e})")


def cpu_float32_worst_ratio():
    """The tolerance's yardstick: the restatement in float32 on the CPU against itself in float64, worst row over the
    parameter set of test 1 (k_stored only cuts columns off: 16 covers the others)."""
    worst = 0.0
    for pf in (3, 6):
        for degree, n_views, n, scale, _pad, _offset in _cases_of(16):
            means, views = _rebuild_inputs(n, n_views, pf)
            v32 = rebuild(means, views, degree, 16, scale, pf, dtype=torch.float32)
            v64 = rebuild64(means, views, degree, 16, scale, pf)
            worst = max(worst, row_error_ratio(v32, v64, forward_magnitude64(means, views, degree, scale, pf)))
    return worst


# ---- test 2 ---------------------------------------------------------------------------------------------------------------
class _Sink:
    """A ``RasterContext.color_grad_sink`` that allocates the buffer of the factored colour gradient ([N,3], or [N,6]
    with the unit view direction), as the sinks of viewdp.py do, and does nothing else."""

    def __init__(self, pf):
        self.pf, self.g = pf, None

    def __call__(self, what, *a):
        if what == "alloc":  # (N, device[, means])
            self.g = torch.full((a[0], self.pf), NAN, device=a[1], dtype=torch.float32)  # must be overwritten
            return self.g
        return None  # "view", "records", "slices", "ready"


@functools.lru_cache(maxsize=None)
def _scene():
    return synthetic_scene(4000, 96, 64, n_views=1, seed=11)


@pytest.mark.parametrize("pf", [3, 6])
@pytest.mark.parametrize("degree,k", [(1, 4), (1, 16), (2, 9), (2, 16), (3, 16)])
@pytest.mark.parametrize("front_end", ["table", "raw"])
def test_factored_backward_and_rebuild_compose_to_the_full_backward(front_end, degree, k, pf):
    """One view, one saved forward state, one fixed cotangent on every output of the per-Gaussian pass; the ordinary
    backward (writes the coefficient gradient) and the factored backward (writes g [N,3] or [N,6]) run on that state
    through ``ops.preprocess`` ([N,K,3] table, rebuilt with the flat entry point) / ``ops.preprocess_raw`` (features_dc
    + features_rest, rebuilt with the split one).  n_views = 1, scale = 1.
    payload 6: rebuild(g, direction) == the ordinary coefficient gradient, torch.equal -- both sides apply the same
    sh_basis to the same direction bits, the sum is 0 + b g and the scale 1.0f.
    payload 3: the direction is recomputed from means - camera position (as viewdp.py places it: -(R^T t) in torch),
    so the comparison is the per-row bound of test 1 against float64 built from the factored g.
    Culled rows carry g == 0; the gradients of means, quats, scales and opacities are the same bits either way."""
    sc = _scene()
    n = sc.means.shape[0]
    vm, K = sc.viewmats[0].to(DEV), sc.Ks[0].to(DEV)
    if front_end == "table":
        cpu = (sc.means, sc.quats, sc.scales, sc.opacities, sc.colors[:, :k].contiguous())
    else:
        cpu = (sc.means, sc.quats, sc.scales.log(), torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4)),
               sc.colors[:, 0].contiguous(), sc.colors[:, 1:k].contiguous())  # fmt: skip
    t = [x.to(DEV).requires_grad_(True) for x in cpu]
    ctx = ops.RasterContext()
    with ops.use(ctx):
        if front_end == "table":
            radii, *outs = ops.preprocess(*t, None, vm, K, sc.width, sc.height, sh_degree=degree)
        else:
            radii, *outs = ops.preprocess_raw(*t, vm, K, sc.width, sc.height, degree)
    means2d, depths, conics, _tiles, splats = outs
    outs = (means2d, depths, conics, splats)
    gen = torch.Generator().manual_seed(5)
    cot = [torch.randn(o.shape, generator=gen).to(DEV) for o in outs]
    plain = torch.autograd.grad(outs, t, cot, retain_graph=True)
    sink = _Sink(pf)
    ctx.color_grad_sink = sink
    factored = torch.autograd.grad(outs, t, cot, allow_unused=True)
    g = sink.g
    assert g is not None and not bool(g.isnan().any())
    culled = radii <= 0
    assert 0 < int(culled.sum()) < n and bool((g[culled][:, :3] == 0).all())
    assert int((g[:, :3] != 0).any(dim=1).sum()) > n // 10
    for name, x, y in zip(("means", "quats", "scales", "opacities"), plain, factored):
        assert torch.equal(x, y), f"v_{name} differs between the ordinary and the factored backward"
    assert all(y is None for y in factored[4:])  # the coefficient gradients are the exchange's to fill
    v_plain = plain[4] if front_end == "table" else torch.cat([plain[4][:, None, :], plain[5]], dim=1)
    entry = "flat" if front_end == "table" else "split"
    if pf == 6:
        v = _hip_rebuild(entry, n, 1, degree, k, None, g, 6 * n, 6, 1.0)
        assert torch.equal(v, v_plain.cpu())
    else:
        cam = -(vm[:3, :3].T @ vm[:3, 3])
        payload = torch.cat([g.reshape(-1), cam])
        v = _hip_rebuild(entry, n, 1, degree, k, t[0].detach(), payload, 3 * n + 3, 3, 1.0)
        views = [(g.cpu(), cam.cpu())]
        v64 = rebuild64(sc.means, views, degree, k, 1.0, 3)
        worst = _assert_rows(v, v64, forward_magnitude64(sc.means, views, degree, 1.0, 3), degree, "rebuild of the factored g")
        helpers._record("row_error_ratio", worst, depth=1)
        print(f"factored {front_end} degree={degree} k_stored={k}: worst row error / forward magnitude {worst:.3e}")


# ---- test 3 ---------------------------------------------------------------------------------------------------------------
def _sparse_views(n, pf, n_views, density, seed):
    """Dense payload rows per view, float32 on the CPU: [(rows [n,pf], camera position [3])].  View v flags its rows
    with the density (density, density / 2, min(1, density + 0.2))[v]: different counts per view."""
    gen = torch.Generator().manual_seed(seed)
    views = []
    for v in range(n_views):
        p = (density, 0.5 * density, min(1.0, density + 0.2))[v]
        flag = torch.rand(n, generator=gen) < p
        rows = torch.randn(n, pf, generator=gen)
        rows[:, :3] = torch.where(flag[:, None], rows[:, :3] + 3.0 * rows[:, :3].sign(), torch.zeros(()))
        rows[1::4, 1:3] = 0.0  # (a single non-zero channel is a non-zero row)
        rows = torch.where((rows[:, :3] != 0).any(dim=1, keepdim=True), rows, torch.zeros(()))  # (no row: no direction)
        views.append((rows, torch.randn(3, generator=gen)))
    return views


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def _compact_all(n, pf, views, cap, block_stride):
    """fg_payload_compact of every view into its block of one gathered buffer, as ModelViewDP.step builds a block:
    incl = cumsum of the any-non-zero flag (int32), the camera position in words 1..3.  The buffer is SENTINEL before.
    -> (gathered [n_views * block_stride + GUARD] on the device, counts)."""
    lib = _lib.load()
    gathered = torch.full((len(views) * block_stride + GUARD,), SENTINEL, device=DEV, dtype=torch.int32).view(torch.float32)
    counts = []
    for v, (rows, cam) in enumerate(views):
        g = rows.to(DEV)
        incl = torch.cumsum((g[:, :3] != 0).any(dim=1), 0, dtype=torch.int32)
        block = gathered[v * block_stride : (v + 1) * block_stride]
        block[1:4] = cam.to(DEV)
        _lib.check(lib.fg_payload_compact(n, pf, g.data_ptr(), incl.data_ptr(), cap, block.data_ptr(), _stream()),
                   "fg_payload_compact")  # fmt: skip
        counts.append(int(incl[-1]))
    return gathered, counts


def _expected_blocks(pf, views, cap, block_stride):
    """What _compact_all must have left, as int32 bits: SENTINEL everywhere but the header and the first
    min(count, cap) rows of (id, payload row) in ascending id."""
    want = torch.full((len(views) * block_stride + GUARD,), SENTINEL, dtype=torch.int32)
    for v, (rows, cam) in enumerate(views):
        ids, kept = compact(rows)
        blk = want[v * block_stride : (v + 1) * block_stride]
        blk[0] = ids.numel()  # the TRUE count, also beyond the capacity
        blk[1:4] = _bits(cam)
        m = min(ids.numel(), cap)
        body = torch.cat([ids[:m, None].to(torch.int32), _bits(kept[:m]).view(m, pf)], dim=1)
        blk[4 : 4 + m * (1 + pf)] = body.reshape(-1)
    return want


def _expand(n, pf, n_views, gathered, block_stride, cap, dense_pad):
    """fg_payload_expand into dense blocks whose rows are zero (the contract) and whose every other float -- camera
    slot, padding, guard -- is SENTINEL.  -> (dense bits on the CPU, dense on the device, dense_stride)."""
    dense_stride = (3 * n + 3 if pf == 3 else 6 * n) + dense_pad
    dense = torch.full((n_views * dense_stride + GUARD,), SENTINEL, device=DEV, dtype=torch.int32).view(torch.float32)
    for v in range(n_views):
        dense[v * dense_stride : v * dense_stride + pf * n] = 0.0
    _lib.check(_lib.load().fg_payload_expand(n, pf, n_views, gathered.data_ptr(), block_stride, cap, dense.data_ptr(),
                                             dense_stride, _stream()), "fg_payload_expand")  # fmt: skip
    return _bits(dense), dense, dense_stride


def _expected_dense(n, pf, blocks_bits, n_views, block_stride, cap, dense_pad):
    """The expand, restated on the blocks' bits: the first min(count, cap) rows whose id is in [0, n) land at their id,
    the camera position (payload 3) behind the rows, nothing else changes."""
    dense_stride = (3 * n + 3 if pf == 3 else 6 * n) + dense_pad
    want = torch.full((n_views * dense_stride + GUARD,), SENTINEL, dtype=torch.int32)
    for v in range(n_views):
        blk = blocks_bits[v * block_stride : (v + 1) * block_stride]
        out = want[v * dense_stride : (v + 1) * dense_stride]
        out[: pf * n] = 0
        if pf == 3:
            out[3 * n : 3 * n + 3] = blk[1:4]
        m = max(0, min(int(blk[0]), cap))
        body = blk[4 : 4 + m * (1 + pf)].view(m, 1 + pf)
        ok = (body[:, 0] >= 0) & (body[:, 0] < n)
        out[: pf * n].view(n, pf)[body[ok, 0].long()] = body[ok, 1:]
    return want


@pytest.mark.parametrize("pf", [3, 6])
@pytest.mark.parametrize("n", [1, 256, 257, 5000])
def test_compact_and_expand_round_trip_and_the_overflow_contract(n, pf):
    """fg_payload_compact / fg_payload_expand against ``nonzero`` plus a gather, bit for bit.  Per (N, payload):
    row-flag density 0 | 0.01 | 0.3 | 1.0, capacity 0 | count-1 | count | count+7 | N (count = view 0's, clipped at 0),
    n_views 1 | 3 for the expand (different counts per view), block_stride and dense_stride padded by 0 | 3.
    The header keeps the true count when count > capacity and only the first `capacity` rows exist, in the block and
    after the expand; words 1..3 stay the caller's; no float outside header, rows, dense rows and camera slot changes."""
    for i_d, density in enumerate((0.0, 0.01, 0.3, 1.0)):
        for n_views in (1, 3):
            views = _sparse_views(n, pf, n_views, density, seed=100 * n + 10 * i_d + n_views)
            count0 = compact(views[0][0])[0].numel()
            for cap in sorted({0, max(count0 - 1, 0), count0, count0 + 7, n}):
                for pad in (0, 3):
                    block_stride = 4 + cap * (1 + pf) + pad
                    gathered, counts = _compact_all(n, pf, views, cap, block_stride)
                    want = _expected_blocks(pf, views, cap, block_stride)
                    what = f"N={n} pf={pf} density={density} n_views={n_views} capacity={cap} pad={pad}"
                    assert counts == [compact(r)[0].numel() for r, _ in views], what
                    assert torch.equal(_bits(gathered), want), f"compact: {what}"
                    got, _dense, dense_stride = _expand(n, pf, n_views, gathered, block_stride, cap, pad)
                    assert torch.equal(got, _expected_dense(n, pf, want, n_views, block_stride, cap, pad)), f"expand: {what}"
                    for v, (rows, cam) in enumerate(views):
                        blk = got[v * dense_stride : (v + 1) * dense_stride]
                        if counts[v] <= cap:  # the dense payload itself comes back
                            assert torch.equal(blk[: pf * n], _bits(rows).reshape(-1)), f"round trip: {what} view {v}"
                            if pf == 3:
                                assert torch.equal(blk[3 * n : 3 * n + 3], _bits(cam)), what
                        else:  # exactly the first `capacity` rows, nothing else
                            ids, kept = compact(rows)
                            first = torch.zeros(n, pf, dtype=torch.int32)
                            first[ids[:cap]] = _bits(kept[:cap]).view(-1, pf)
                            assert torch.equal(blk[: pf * n], first.reshape(-1)), f"truncated: {what} view {v}"


@pytest.mark.parametrize("pf", [3, 6])
def test_expand_leaves_out_rows_with_ids_outside_the_table_and_blocks_without_rows(pf):
    """The expand's own guard (id < 0 || id >= N skips the row) and its reading of the header: blocks written by hand
    with ids -1, N, N + 5, INT_MAX and INT_MIN among valid ones put only the valid rows in place; a header count of 0
    and a negative one write nothing but the camera position (payload 3) / nothing at all (payload 6)."""
    n, cap, pad = 300, 40, 3
    block_stride = 4 + cap * (1 + pf) + pad
    gen = torch.Generator().manual_seed(9)
    blocks = torch.full((3 * block_stride + GUARD,), SENTINEL, dtype=torch.int32)
    ids = torch.randperm(n, generator=gen)[:cap].sort().values.to(torch.int32)
    ids[[0, 5, 6, 20, 39]] = torch.tensor([-1, n, n + 5, 2**31 - 1, -(2**31)], dtype=torch.int32)
    body = torch.cat([ids[:, None], _bits(torch.randn(cap, pf, generator=gen) + 4.0)], dim=1).reshape(-1)
    for v, count in enumerate((cap, 0, -7)):
        blk = blocks[v * block_stride : (v + 1) * block_stride]
        blk[0] = count
        blk[1:4] = _bits(torch.randn(3, generator=gen))
        blk[4 : 4 + body.numel()] = body  # (the rows are there in every block: the header decides)
    got, _dense, _stride = _expand(n, pf, 3, blocks.to(DEV).view(torch.float32), block_stride, cap, pad)
    want = _expected_dense(n, pf, blocks, 3, block_stride, cap, pad)
    assert torch.equal(got, want)
    dense_stride = (3 * n + 3 if pf == 3 else 6 * n) + pad
    assert int((want[: pf * n].view(n, pf) != 0).any(dim=1).sum()) == cap - 5  # (the restatement kept the valid rows)
    for v in (1, 2):
        assert bool((got[v * dense_stride : v * dense_stride + pf * n] == 0).all())


@pytest.mark.parametrize("pf,n,degree,k", [(3, 257, 3, 16), (6, 257, 1, 9), (3, 1000, 2, 12), (6, 1000, 3, 16), (3, 63, 0, 1)])
def test_compact_expand_and_split_rebuild_equal_the_rebuild_from_dense_blocks(pf, n, degree, k):
    """End to end as ModelViewDP.step runs the sparse form: compact per view, expand, split rebuild == the split rebuild
    from the dense blocks themselves, torch.equal (three views, capacity = the largest count + 7, padded strides)."""
    means, views = _rebuild_inputs(n, 3, pf)
    rows = []
    for g, second in views:  # the dense rows as the factored backward leaves them: the direction of a culled row is (0, 0, 1)
        if pf == 6:
            second = torch.where(second.isnan(), torch.tensor([0.0, 0.0, 1.0]).expand(n, 3), second)
            rows.append((torch.cat([g, second], dim=1), torch.zeros(3)))
        else:
            rows.append((g.clone(), second))
    cap = max(compact(r)[0].numel() for r, _ in rows) + 7
    block_stride = 4 + cap * (1 + pf) + 3
    gathered, counts = _compact_all(n, pf, rows, cap, block_stride)
    assert max(counts) <= cap and min(counts) > 0
    _got, dense, dense_stride = _expand(n, pf, 3, gathered, block_stride, cap, 1)
    direct, stride = _dense_blocks([(r[:, :3], r[:, 3:] if pf == 6 else c) for r, c in rows], n, pf, 5)
    scale = 1.0 / 3
    means_dev = means.to(DEV)
    a = _hip_rebuild("split", n, 3, degree, k, means_dev, dense, dense_stride, pf, scale)
    b = _hip_rebuild("split", n, 3, degree, k, means_dev, direct.to(DEV), stride, pf, scale)
    assert torch.equal(a, b) and float(a.abs().max()) > 0


if __name__ == "__main__":  # the yardstick of TOL (needs no GPU)
    print(f"CPU float32 restatement against float64, worst row error / forward magnitude: {cpu_float32_worst_ratio():.3e}")
