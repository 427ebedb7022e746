"""The training step of ``tests/test_mlp_chunked_gpu.py::test_model_training_step_with_the_knob_set_and_unset`` cut at its
stage boundaries, and the host-side count of the float-atomic addends of the raster backward.  A helper, not a test.

THE STEP (``make_step`` / ``Step``): the blender model, ``n = deform.FUSED_MIN_ROWS`` Gaussians, a 16 x 16 image, step 4000,
``FG_FUSED_MLP_TRAIN=2``, ``FG_FUSED_MLP_WGRAD=1`` and ``FG_FUSED_MLP_CHUNKED`` set or unset (``knobs``).  ``Step.STAGES`` are
the pieces of ``FreeGaussianModel._outputs_from`` + ``get_loss_dict`` + their backward, each a function of a dict of tensors
(a recorded run, ``Step.chain``) that calls the entry point the model calls -- ``model.deform`` (``ops.mlp_train``),
``utils.transform_points``, ``ops.preprocess_raw``, ``ops.bin_tiles``, ``ops.rasterize_splats``, ``model.get_loss_dict``
(``ops.l1_ssim``) -- with the model's own arguments, on the calling thread's current ``ops.RasterContext``; the backward of a
stage is ``torch.autograd.grad`` through that stage's own node.  An image this small takes the stage-wise calls
(``ops.step_path_available`` wants job lists), which is why the step can be cut there at all.

    mlp_forward            x, times                                 -> d_xyz, d_rotation, d_scaling
    transform_forward      d_xyz (+ the means)                      -> means_d
    per_gaussian_forward   means_d, d_rotation, d_scaling (+ params)-> radii, means2d, depths, conics, tiles, splats,
                                                                       depth_keys, tile_rects (, tile_masks)
    binning                the above                                -> offsets, flatten_ids
    raster_forward         splats, means2d, offsets, flatten_ids    -> render, alphas, last_ids
    loss                   render                                   -> loss, v_render
    raster_backward        raster_forward's inputs, v_render        -> v_splats  (columns 0:2 are the means2d gradient)
    per_gaussian_backward  per_gaussian_forward's inputs, v_splats  -> v_means_d, v_quats, v_d_rotation, v_scales,
                                                                       v_d_scaling, v_opacities, v_features_dc, v_features_rest
    transform_backward     d_xyz, v_means_d                         -> v_d_xyz, v_means
    mlp_backward           x, times, v_d_xyz, v_d_rotation, v_d_scaling -> the 28 ``deform.*`` gradients, v_aux

One difference from the model's order of issue: the model enqueues the raster forward on the capacity-sized list and waits
for the list length afterwards; here the binning stage finishes its list first and the raster stages get the finished list.
The kernels, their arguments and the launch (``launch_of``) are the same.

THE COUNT (``addend_count``).  ``raster_bwd_body`` (csrc/raster.hip) ends every list entry to which at least one of a
WAVEFRONT's pixels contributes (``contributed``) with one wave reduction and ONE float atomic per gradient slot into
``v_splats[gid]``.  So the number ``k`` of separate addends a splat's record gradient receives is the number of
(tile, wavefront) pairs with a contributing pixel, and which pixels a wavefront owns is the launch's business:

    classic launch (``raster_bwd_kernel<C, PPT>``, one workgroup per tile, ``256 / PPT / 64`` wavefronts; ``wave_strips``):
        PPT = 1 (below 3000 tiles, ``raster_ppt_bwd``): FOUR wavefronts per tile, wavefront w owns rows 4w .. 4w + 3
        PPT = 2 (3000 .. 5999 tiles): two wavefronts, strips {w, w + 2};  PPT = 4 (from 6000 tiles): one wavefront
    job lists, pixel strips (``raster_bwd_mixed_kernel``, ``job_from_list``: entry = tile << 3 | strip + 1): one wavefront
        per job -- the whole tile (strip -1), strips {h, h + 2} (strip 4 + h) or one strip
    job lists, list shares (``share_from_list``: tile = e >> 12, part = e >> 6 & 63, parts = (e & 63) + 1; three channels,
        the forward's checkpoints present): one wavefront per job over the whole tile and ONE part of its list: every entry
        lies in exactly one part (``seg_bound``), so one addend per (splat, tile)
    (classic below ``FG_MIXED_MIN_TILES`` = 200 tiles -- ``raster_tail`` / ``mixed_tail_bwd`` -- lists from there on)

"Contributes" is the kernel's ``valid``: the entry is not behind the pixel's ``last_ids``, sigma >= 0, alpha >= 1/255.
``strip_hits`` evaluates that in float64 from the records and the forward's own ``last_ids`` with a margin of 1e-5 on both
thresholds, so ``k`` is an UPPER bound of the addends (a pixel on a knife edge counts): ``k <= 2`` proves a row repeatable
(0 + a + b = 0 + b + a in floating point), ``k >= 3`` allows a reordering of a k-term fp32 sum, which moves it by at most
``2 (k - 1) 2^-24 A`` with ``A`` the slot's absolute accumulation (``raster_restatement.backward``).
"""
import contextlib
import copy
import os

import torch

import raster_restatement as R
from oracle import raster_oracle as O

REPEATS = 8
U32 = 2.0**-24
TILE = 16
MIXED_MIN_TILES = 200  # raster.hip FG_MIXED_MIN_TILES
MARGIN = 1e-5
W_STEP = H_STEP = 16
ENV = {"FG_FUSED_MLP_TRAIN": "2", "FG_FUSED_MLP_WGRAD": "1", "FG_FUSED_MLP_CHUNKED": "1"}
OLD_SCALE_MEAN = -3.8  # log-scale the flaky test drew its splats around
SCALE_MEAN = -5.2  # ... and the one the repaired test draws them around: see ``make_step``


@contextlib.contextmanager
def knobs(chunked=True, wgrad_precision=None):
    """The three environment knobs of the flaky test (``FG_FUSED_MLP_CHUNKED`` set or unset), restored on exit."""
    want = dict(ENV)
    if not chunked:
        want["FG_FUSED_MLP_CHUNKED"] = None
    want["FG_FUSED_MLP_WGRAD_PRECISION"] = wgrad_precision
    old = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


# ---------------------------------------------------------------------------------------------------------------------
# the step


def make_step(device, scale_mean=SCALE_MEAN):
    """(model, camera, ground truth) exactly as the flaky test built them -- same seeds, same order of draws -- but for the
    mean of the log-scales.  At -3.8 the largest alpha >= 1/255 footprints are six pixel rows high and more: such a splat can
    reach three of a tile's 4-row strips, i.e. three wavefronts' atomics (``step_scene_host`` counts them: one does).  At -5.2 the
    footprint is the 0.3-pixel blur's (opacity 0.1: alpha >= 1/255 within 1.4 px of the centre), at most four rows, at most two
    strips."""
    from freegaussian_amd import deform as D
    from freegaussian_amd.model import Camera, FreeGaussianModel, FreeGaussianModelConfig
    from freegaussian_amd.scenes import look_at_viewmat

    torch.manual_seed(0)
    n, W, H = D.FUSED_MIN_ROWS, W_STEP, H_STEP  # the smallest count that reaches the dispatch
    cfg = FreeGaussianModelConfig(background_color="white", num_downscales=0, warm_up=3000)
    model = FreeGaussianModel(cfg, seed_points=(torch.rand(n, 3) - 0.5) * 2.0, init_scales=-3.8, is_blender=True)
    with torch.no_grad():
        model.gauss_params["scales"].normal_(scale_mean, 0.3)
        model.gauss_params["features_rest"].normal_(0, 0.1)
        for q in model.deform.parameters():
            q.mul_(0.3)
    model.step = 4000  # behind warm_up: the deformation net runs
    model = model.to(device).train()
    c2w = torch.linalg.inv(look_at_viewmat(torch.tensor([0.3, -0.2, -3.0]), torch.zeros(3)))
    c2w[:3, 1:3] *= -1
    cam = Camera(c2w[None, :3], 56.0, 60.0, W / 2, H / 2, W, H, times=torch.tensor([[0.4]]))
    gt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(12)).to(device)
    return model, cam, gt


def _clone(t):
    return None if t is None else t.detach().clone()


class Step:
    """The step on the GPU, stage by stage (module docstring).  Every stage function takes a dict of tensors and returns a
    dict of new tensors (detached copies); none keeps state."""

    def __init__(self, device="cuda", scale_mean=SCALE_MEAN):
        self.model, self.cam, self.gt = make_step(device, scale_mean)
        m = self.model
        self.viewmat, self.K, self.W, self.H = m._camera_setup(copy.deepcopy(self.cam))
        self.viewmat, self.K = self.viewmat.clone(), self.K.clone()  # (views of a ring of staging words otherwise)
        self.n = m.num_points
        self.sh_degree = min(m.step // m.config.sh_degree_interval, m.config.sh_degree)
        self.background = m._get_background_color()
        self.x = m.gauss_params["means"].detach().clone()
        self.times = self.cam.times.to(m.device).expand(self.n, -1)
        self.deform_names = [k for k, _ in m.deform.named_parameters()]

    STAGES = ("mlp_forward", "transform_forward", "per_gaussian_forward", "binning", "raster_forward", "loss",
              "raster_backward", "per_gaussian_backward", "transform_backward", "mlp_backward")  # fmt: skip

    # -- the deformation net ----------------------------------------------------------------------------------------
    def _deform(self, s):
        return self.model.deform(s["x"], s["times"])  # (x carries no gradient: _outputs_from detaches it)

    def mlp_forward(self, s):
        d_xyz, rot, scal = self._deform(s)  # (the taped call, as in the step)
        return dict(d_xyz=_clone(d_xyz), d_rotation=_clone(rot), d_scaling=_clone(scal))

    def mlp_backward(self, s):
        """The 28 parameter gradients, and the gradient of the trunk's auxiliary input rows (the time net's output: the
        fused backward's input-row gradient, ``fg_mlp_bwd_inputs`` / ``fg_mlp_train_bwd``)."""
        from freegaussian_amd import ops

        seen, real = {}, ops.mlp_train

        def spy(x, aux, *a, **k):
            aux.retain_grad()
            seen["aux"] = aux
            return real(x, aux, *a, **k)

        ops.mlp_train = spy
        try:
            outs = self._deform(s)
        finally:
            ops.mlp_train = real
        params = [p for _, p in self.model.deform.named_parameters()]
        self.model.deform.zero_grad(set_to_none=True)
        torch.autograd.backward(outs, (s["v_d_xyz"], s["v_d_rotation"], s["v_d_scaling"]))
        out = {"deform." + k: _clone(p.grad) for k, p in zip(self.deform_names, params)}
        out["v_aux"] = _clone(seen["aux"].grad)
        self.model.deform.zero_grad(set_to_none=True)
        return out

    # -- the transform of the means (torch) --------------------------------------------------------------------------
    def transform_forward(self, s):
        from freegaussian_amd.utils import transform_points

        with torch.no_grad():
            return dict(means_d=transform_points(s["d_xyz"], self.model.gauss_params["means"]).clone())

    def transform_backward(self, s):
        from freegaussian_amd.utils import transform_points

        T, pts = s["d_xyz"].detach().requires_grad_(True), self.model.gauss_params["means"].detach().requires_grad_(True)
        g_T, g_pts = torch.autograd.grad(transform_points(T, pts), (T, pts), s["v_means_d"])
        return dict(v_d_xyz=_clone(g_T), v_means=_clone(g_pts))

    # -- the per-Gaussian pass ---------------------------------------------------------------------------------------
    def _pg_inputs(self, s, grad):
        p = self.model.gauss_params
        leaf = lambda t: t.detach().requires_grad_(grad)  # noqa: E731
        return dict(means=leaf(s["means_d"]), quats=leaf(p["quats"]), scales=leaf(p["scales"]), opacities=leaf(p["opacities"]),
                    dc=leaf(p["features_dc"]), rest=leaf(p["features_rest"]), d_rot=leaf(s["d_rotation"]), d_scal=leaf(s["d_scaling"]))  # fmt: skip

    def _preprocess(self, i):
        from freegaussian_amd import ops

        return ops.preprocess_raw(i["means"], i["quats"], i["scales"], i["opacities"], i["dc"], i["rest"], self.viewmat[0],
                                  self.K[0], self.W, self.H, self.sh_degree, d_quats=i["d_rot"], d_scales=i["d_scal"], extra=None,
                                  eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0, tile_size=TILE,
                                  antialiased=False, with_depth=False)  # fmt: skip

    def per_gaussian_forward(self, s):
        with torch.no_grad():
            radii, means2d, depths, conics, tiles, splats = self._preprocess(self._pg_inputs(s, False))
        out = dict(radii=_clone(radii), means2d=_clone(means2d), depths=_clone(depths), conics=_clone(conics), tiles=_clone(tiles),
                   splats=_clone(splats))  # fmt: skip
        side = getattr(splats, "_fg_bin", None)
        if side is not None:
            out.update(depth_keys=_clone(side[0]), tile_rects=_clone(side[1]))
            if len(side) > 2 and side[2] is not None:
                out["tile_masks"] = _clone(side[2])
        return out

    def per_gaussian_backward(self, s):
        i = self._pg_inputs(s, True)
        radii, means2d, depths, conics, tiles, splats = self._preprocess(i)
        v_splats = s["v_splats"]
        names = ("means", "quats", "d_rot", "scales", "d_scal", "opacities", "dc", "rest")
        # (the means2d gradient is columns 0:2 of the record gradient, a strided view, as _RasterSplats hands it back)
        g = torch.autograd.grad((means2d, splats), [i[k] for k in names], (v_splats[:, 0:2], v_splats))
        outs = ("v_means_d", "v_quats", "v_d_rotation", "v_scales", "v_d_scaling", "v_opacities", "v_features_dc", "v_features_rest")
        return {k: _clone(t) for k, t in zip(outs, g)}

    # -- the lists ---------------------------------------------------------------------------------------------------
    def binning(self, s):
        from freegaussian_amd import ops

        tw, th = (self.W + TILE - 1) // TILE, (self.H + TILE - 1) // TILE
        keys_rects = None
        if "depth_keys" in s:  # (the depth-first path sorts the keys in place: a copy per call)
            keys_rects = (s["depth_keys"].clone(), s["tile_rects"].clone(), _clone(s.get("tile_masks")))
        with torch.no_grad():
            _, ids, offsets, finish = ops.bin_tiles(s["means2d"], s["radii"], s["depths"], s["tiles"], TILE, tw, th, defer=True,
                                                    want_keys=False, keys_rects=keys_rects, raster_hint=(3, self.W, self.H))  # fmt: skip
            if finish is not None:
                _, ids, _ = finish()
        torch.cuda.synchronize()
        return dict(offsets=_clone(offsets), flatten_ids=_clone(ids))

    # -- compositing -------------------------------------------------------------------------------------------------
    def _raster(self, s, grad):
        from freegaussian_amd import ops

        splats = s["splats"].detach().requires_grad_(grad)
        means2d = s["means2d"].detach().unsqueeze(0).requires_grad_(grad)
        out = ops.rasterize_splats(splats, means2d, 3, self.W, self.H, TILE, s["offsets"], s["flatten_ids"], absgrad=True,
                                   background=self.background, n_clamp=3)  # fmt: skip
        return splats, means2d, out

    def raster_forward(self, s):
        with torch.no_grad():
            _, _, (render, alphas, last_ids) = self._raster(s, False)
        return dict(render=_clone(render), alphas=_clone(alphas), last_ids=_clone(last_ids))

    def raster_backward(self, s):
        splats, means2d, (render, _, _) = self._raster(s, True)
        v_splats, v_m2 = torch.autograd.grad(render, (splats, means2d), s["v_render"])
        assert torch.equal(v_m2.reshape(-1, 2), v_splats[:, 0:2])
        return dict(v_splats=_clone(v_splats))

    # -- the loss ----------------------------------------------------------------------------------------------------
    def loss(self, s):
        render = s["render"].detach().requires_grad_(True)
        out = {"rgb": render, "background": self.background}
        loss = self.model.get_loss_dict(out, {"image": self.gt})["main_loss"]
        (v,) = torch.autograd.grad(loss, render)
        return dict(loss=_clone(loss), v_render=_clone(v))

    # -- the chain ---------------------------------------------------------------------------------------------------
    def chain(self, recorded=None):
        """-> {stage: its outputs}.  ``recorded`` None: one run's own outputs flow from stage to stage; else every stage
        reads its inputs from that dict of (an earlier run's) tensors."""
        flow = dict(x=self.x, times=self.times)
        outs = {}
        for name in self.STAGES:
            outs[name] = getattr(self, name)(flow if recorded is None else recorded)
            if recorded is None:
                flow.update(outs[name])
        torch.cuda.synchronize()
        return outs

    @staticmethod
    def flat(outs):
        """{name: tensor} over all stages of a chain (the names are unique), + x and times."""
        return {k: v for stage in outs.values() for k, v in stage.items()}

    def record(self):
        outs = self.chain()
        rec = dict(x=self.x, times=self.times)
        rec.update(self.flat(outs))
        return rec, outs

    def final_gradients(self, flat):
        """What ``loss.backward()`` leaves on the model's parameters, by parameter name."""
        g = {"gauss_params.means": flat["v_means"], "gauss_params.quats": flat["v_quats"], "gauss_params.scales": flat["v_scales"],
             "gauss_params.opacities": flat["v_opacities"], "gauss_params.features_dc": flat["v_features_dc"],
             "gauss_params.features_rest": flat["v_features_rest"]}  # fmt: skip
        g.update({k: v for k, v in flat.items() if k.startswith("deform.")})
        return g


def model_step(model, cam, gt):
    """The step as the flaky test runs it: -> (loss, {parameter: gradient})."""
    model.zero_grad(set_to_none=True)
    out = model.get_outputs(copy.deepcopy(cam))
    loss = model.get_loss_dict(out, {"image": gt})["main_loss"]
    loss.backward()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def differing(a, b):
    """{name: elements that differ} over two dicts of tensors with the same keys (bitwise; NaN never equals)."""
    out = {}
    for k in a:
        if a[k] is None and b[k] is None:
            continue
        if not torch.equal(a[k], b[k]):
            out[k] = int((a[k] != b[k]).sum())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the launch of the raster backward, and the addends it makes


def classic_ppt_bwd(n_tiles):
    """raster.hip ``raster_ppt_bwd``: pixels per lane of the classic backward launch."""
    return 4 if n_tiles >= 6000 else (2 if n_tiles >= 3000 else 1)


def classic_groups(ppt):
    """The strip sets (bit s = rows 4s .. 4s + 3) of a classic workgroup's wavefronts (``wave_strips``)."""
    return {1: [1, 2, 4, 8], 2: [5, 10], 4: [15]}[ppt]


def launch_of(width, height):
    """"classic" or "jobs" for the default policy (``raster_tail``: job lists from FG_MIXED_MIN_TILES tiles on)."""
    n_tiles = ((width + TILE - 1) // TILE) * ((height + TILE - 1) // TILE)
    return "classic" if n_tiles < MIXED_MIN_TILES else "jobs"


def groups_classic(n_tiles, ppt=None):
    g = classic_groups(classic_ppt_bwd(n_tiles) if ppt is None else ppt)
    return torch.tensor([g + [0] * (4 - len(g))] * n_tiles, dtype=torch.int64)


def groups_from_jobs(jobs, n_tiles, shares, offsets):
    """[n_tiles, 4] strip sets of the wavefronts that add into a tile's splats, decoded from the backward's job list
    (``fg_raster_build_jobs`` / ``fg_stbin_fill_jobs``; layout: csrc/jobs_build.h, decoders: raster.hip ``job_from_list`` /
    ``share_from_list``).  Every tile with a list must be covered: by strip jobs that own each strip once, or by the parts
    0 .. P - 1 of its list, each once (then the tile is ONE group: an entry lies in one part)."""
    jobs = [int(v) for v in jobs.cpu().tolist()]
    words = len(jobs)
    cap = (words - 8 - n_tiles) // 8  # (heavy tiles off: 8 counts, 8 segments of cap entries, the table of first slots)
    assert cap > 0 and 8 + 8 * cap + n_tiles == words, (words, n_tiles)
    per_tile = {}
    for xcd in range(8):
        assert 0 <= jobs[xcd] <= cap
        for k in range(jobs[xcd]):
            e = jobs[8 + xcd * cap + k]
            if shares:
                per_tile.setdefault(e >> 12, []).append(((e >> 6) & 63, (e & 63) + 1))
            else:
                e &= ~((1 << 30) | (1 << 28))
                per_tile.setdefault(e >> 3, []).append((e & 7) - 1)
    offs = offsets.cpu().tolist()
    G = torch.zeros(n_tiles, 4, dtype=torch.int64)
    for t in range(n_tiles):
        got = per_tile.get(t)
        if got is None:
            assert offs[t + 1] == offs[t], f"tile {t} has a list and no job"
            continue
        if shares:
            parts = {p for _, p in got}
            assert len(parts) == 1 and sorted(i for i, _ in got) == list(range(got[0][1])), (t, got)
            G[t, 0] = 15
        else:
            masks = [15 if s < 0 else ((1 << (s - 4)) | (1 << (s - 2))) if s >= 4 else (1 << s) for s in got]
            assert len(masks) <= 4 and sum(masks) == 15 and len(set(masks)) == len(masks), (t, got)
            G[t, : len(masks)] = torch.tensor(masks)
    return G


def strip_hits(means2d, conics, opacities, offsets, flatten_ids, last_ids, width, height, chunk=2048):
    """float64, CPU.  -> (gid [E], tile [E], hits [E] int64): for every list entry some pixel of its tile may use (it is not
    behind the largest ``last_ids`` of the tile), the 4-bit set of the tile's strips with a pixel that may CONTRIBUTE --
    entry <= last_ids[pixel], sigma >= 0 and alpha >= 1/255, both with a margin of ``MARGIN`` towards "contributes"."""
    m2, con, op = means2d.detach().cpu().double(), conics.detach().cpu().double(), opacities.detach().cpu().double().reshape(-1)
    offsets, flatten_ids, last_ids = offsets.cpu(), flatten_ids.cpu(), last_ids.cpu()
    tw, th = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    gids, tiles, hits = [], [], []
    for t in range(tw * th):
        s, e = int(offsets[t]), int(offsets[t + 1])
        ty, tx = divmod(t, tw)
        y0, x0, y1, x1 = ty * TILE, tx * TILE, min(ty * TILE + TILE, height), min(tx * TILE + TILE, width)
        last = last_ids[y0:y1, x0:x1].reshape(-1).long()
        e = min(e, int(last.max()) + 1) if e > s else e
        if e <= s:
            continue
        yy, xx = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        px, py = xx.reshape(-1).double() + 0.5, yy.reshape(-1).double() + 0.5
        strip = ((yy.reshape(-1) - y0) // 4).long()
        for c0 in range(s, e, chunk):
            c1 = min(c0 + chunk, e)
            ids = flatten_ids[c0:c1].long()
            dx = m2[ids, 0][None, :] - px[:, None]
            dy = m2[ids, 1][None, :] - py[:, None]
            qa, qb, qc = 0.5 * con[ids, 0][None, :] * dx * dx, con[ids, 1][None, :] * dx * dy, 0.5 * con[ids, 2][None, :] * dy * dy
            sigma = qa + qc + qb
            ok = (torch.arange(c0, c1)[None, :] <= last[:, None]) & (sigma >= -MARGIN * (qa.abs() + qb.abs() + qc.abs()) - 1e-12)
            ok &= op[ids][None, :] * torch.exp(-sigma.clamp_min(0.0)) >= O.ALPHA_SKIP * (1.0 - MARGIN)
            h = torch.zeros(c1 - c0, dtype=torch.int64)
            for k in range(4):
                h |= ok[strip == k].any(dim=0).long() << k
            gids.append(ids)
            tiles.append(torch.full_like(ids, t))
            hits.append(h)
    if not gids:
        z = torch.zeros(0, dtype=torch.int64)
        return z, z, z
    return torch.cat(gids), torch.cat(tiles), torch.cat(hits)


def addend_count(n, gid, tile, hits, groups):
    """[n] int64: k per splat = over its list entries, the wavefronts (``groups[tile]``: their strip sets) one of whose strips
    is hit."""
    per_entry = ((hits[:, None] & groups[tile]) != 0).sum(dim=1)
    return torch.zeros(n, dtype=torch.int64).index_add_(0, gid, per_entry)


def addend_count_brute(n, means2d, conics, opacities, offsets, flatten_ids, last_ids, width, height, jobs_of_tile):
    """The same number by the kernel's own loops: ``jobs_of_tile[t]`` = the wavefronts that walk tile t, each a list of
    the pixel ROWS (within the tile) it owns; for every wavefront, every entry, every pixel: one addend if any contributes.
    Plain Python, for the tiny hand-built case of the host test."""
    import math

    k = [0] * n
    tw = (width + TILE - 1) // TILE
    for t, waves in jobs_of_tile.items():
        ty, tx = divmod(t, tw)
        for rows in waves:
            for idx in range(int(offsets[t]), int(offsets[t + 1])):
                g = int(flatten_ids[idx])
                x, y, (a, b, c), o = float(means2d[g, 0]), float(means2d[g, 1]), (float(v) for v in conics[g]), float(opacities[g])
                hit = False
                for r in rows:
                    for col in range(TILE):
                        iy, ix = ty * TILE + r, tx * TILE + col
                        if iy >= height or ix >= width or idx > int(last_ids[iy, ix]):
                            continue
                        dx, dy = x - (ix + 0.5), y - (iy + 0.5)
                        sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
                        hit = hit or (sigma >= 0 and o * math.exp(-sigma) >= O.ALPHA_SKIP)
                k[g] += int(hit)
    return torch.tensor(k, dtype=torch.int64)


def census(k):
    """{"0": rows without an addend, "1", "2", ">=3", "max"}."""
    return {"0": int((k == 0).sum()), "1": int((k == 1).sum()), "2": int((k == 2).sum()), ">=3": int((k >= 3).sum()),
            "max": int(k.max()) if k.numel() else 0}  # fmt: skip


def order_bound(k, accum16):
    """[N,16] float64: what two runs of the raster backward may differ by per record-gradient slot: 0 where k <= 2, else
    2 (k - 1) 2^-24 A."""
    kk = k.double()[:, None]
    return torch.where(kk >= 3, 2.0 * (kk - 1.0) * U32 * accum16.double(), torch.zeros_like(accum16, dtype=torch.float64))


def accum_slots(accum):
    """[N,16] from ``raster_restatement.backward``'s absolute accumulations, in the record gradient's slot order
    (``unpack_grads_kernel``: 0:2 means2d, 2 opacity, 3:6 conic, 6:8 absgrad, 8:11 the three colours)."""
    n = accum["means2d"].shape[0]
    A = torch.zeros(n, 16, dtype=torch.float64)
    A[:, 0:2], A[:, 2:3], A[:, 3:6], A[:, 6:8] = accum["means2d"], accum["opacities"], accum["conics"], accum["absgrad"]
    A[:, 8 : 8 + accum["features"].shape[1]] = accum["features"]
    return A


# ---------------------------------------------------------------------------------------------------------------------
# the small scenes of the raster stage on its own

RASTER_SCENES = {
    # name: (width, height, splats, (sigma ranges of the small / medium / large thirds), launch)
    "one_tile": (16, 16, 300, ((0.3, 0.7), (1.2, 2.2), (3.0, 6.0)), "classic"),
    "two_tiles": (32, 16, 400, ((0.3, 0.7), (1.2, 2.2), (3.0, 6.0)), "classic"),
    # 20 x 10 = 200 tiles: the fewest for which fg_raster_jobs_words > 0 (FG_MIXED_MIN_TILES)
    "job_lists": (320, 160, 1500, ((0.4, 1.2), (2.5, 5.0), (8.0, 16.0)), "jobs"),
}


def raster_scene(name, seed=7):
    """A ``raster_restatement.RegimeScene`` (2-D splats, explicit lists from generous radius boxes) whose rows fall in one,
    in two and in three or more wavefronts' pixel sets: a third each of splats well inside a 4-row strip's height, about a
    strip high, and several strips (or tiles) high, anywhere in the image; opacities 0.05 .. 0.35 so that lists stay open."""
    width, height, n, sizes, _ = RASTER_SCENES[name]
    g = torch.Generator().manual_seed(seed)

    def U(m, lo, hi):
        return lo + (hi - lo) * torch.rand(m, generator=g, dtype=torch.float64)

    labels = [("small", "medium", "large")[i * 3 // n] for i in range(n)]
    lo = torch.tensor([sizes[("small", "medium", "large").index(l)][0] for l in labels], dtype=torch.float64)
    hi = torch.tensor([sizes[("small", "medium", "large").index(l)][1] for l in labels], dtype=torch.float64)
    sx, sy, rho = lo + (hi - lo) * U(n, 0, 1), lo + (hi - lo) * U(n, 0, 1), U(n, -0.5, 0.5)
    xy = torch.stack([U(n, 0.0, float(width)), U(n, 0.0, float(height))], -1)
    radius = torch.ceil(3.5 * torch.maximum(sx, sy)) + 1.0
    perm = torch.randperm(n, generator=g)
    return R.with_lists(xy.float()[perm], R.conic_of(sx, sy, rho).float()[perm], U(n, 0.05, 0.35).float()[perm],
                        U(n, 1.0, 10.0).float()[perm], radius.to(torch.int32)[perm], U(8 * n, 0.0, 1.0).reshape(n, 8).float()[perm],
                        [labels[int(i)] for i in perm], width, height)  # fmt: skip


def raster_cotangent(scene, seed=3):
    """v_render [H,W,3] float64, standard normal."""
    return torch.randn(scene.height, scene.width, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def pack_records(scene):
    """[N,16] float32 records as ``fg_pack_splats`` lays them out: x, y, opacity, conic a b c, then the colours."""
    n = scene.means2d.shape[0]
    rec = torch.zeros(n, 16)
    rec[:, 0:2], rec[:, 2], rec[:, 3:6], rec[:, 6:9] = scene.means2d, scene.opacities, scene.conics, scene.features(3)
    return rec


def host_last_ids(scene, chunk=2048):
    """[H,W] int32 ``last_ids`` of the float64 walk (the tile's start - 1 where nothing contributes), in chunks of the list:
    what ``raster_restatement.composite`` returns, for lists too long to hold a [pixels, entries] array of."""
    m2, con, op = scene.means2d.double(), scene.conics.double(), scene.opacities.double()
    last_ids = torch.zeros(scene.height, scene.width, dtype=torch.int32)
    for t, s, e, y0, y1, x0, x1 in R._tiles(scene):
        P = (y1 - y0) * (x1 - x0)
        last, T, done = torch.full((P,), s - 1, dtype=torch.int64), torch.ones(P, dtype=torch.float64), torch.zeros(P, dtype=torch.bool)
        px, py = R._pixel_centres(y0, y1, x0, x1, torch.float64)
        for c0 in range(s, e, chunk):
            if bool(done.all()):
                break
            ids = scene.flatten_ids[c0 : min(c0 + chunk, e)].long()
            _, _, _, alpha, valid = O._tile_terms(px, py, m2[ids], con[ids], op[ids])
            a = torch.where(valid, alpha, torch.zeros_like(alpha))
            T_incl = T[:, None] * torch.cumprod(1.0 - a, dim=1)
            stopped = torch.cumsum((valid & (T_incl <= O.T_STOP)).to(torch.int32), dim=1) > 0
            include = valid & ~stopped & ~done[:, None]
            idx = torch.arange(c0, c0 + ids.numel())[None, :].expand_as(include)
            last = torch.maximum(last, torch.where(include, idx, torch.full_like(idx, -1)).max(dim=1).values)
            # (the transmittance behind the chunk: the product over the included entries only)
            T = T * torch.where(include, 1.0 - a, torch.ones_like(a)).prod(dim=1)
            done |= stopped.any(dim=1)
        last_ids[y0:y1, x0:x1] = last.reshape(y1 - y0, x1 - x0).to(torch.int32)
    return last_ids


def scene_addends(scene, groups, last_ids=None):
    """k [N] of a 2-D scene under the wavefront sets ``groups`` ([n_tiles, 4]); ``last_ids``: the forward's (default: the
    float64 walk's)."""
    last_ids = host_last_ids(scene) if last_ids is None else last_ids
    gid, tile, hits = strip_hits(scene.means2d, scene.conics, scene.opacities, scene.offsets, scene.flatten_ids, last_ids,
                                 scene.width, scene.height)  # fmt: skip
    return addend_count(scene.means2d.shape[0], gid, tile, hits, groups)


def n_tiles_of(scene):
    return ((scene.width + TILE - 1) // TILE) * ((scene.height + TILE - 1) // TILE)


def step_scene_host(scale_mean):
    """The step's splats as a 2-D scene, on the CPU: the model of ``make_step`` through its torch path, the oracle's
    projection and the reference's lists (radius boxes: a superset of the footprint lists the GPU walks; the extra
    entries contribute to no pixel).  The GPU's own census comes from its own records (tests/test_step_repeat_gpu.py)."""
    from freegaussian_amd.utils import transform_points

    model, cam, _ = make_step("cpu", scale_mean)
    p = model.gauss_params
    with torch.no_grad():
        viewmat, K, W, H = model._camera_setup(copy.deepcopy(cam))
        pts = p["means"]
        d_xyz, d_rot, d_scal = model.deform(pts, cam.times.expand(pts.shape[0], -1))
        means = transform_points(d_xyz, pts)
        quats = p["quats"] / p["quats"].norm(dim=-1, keepdim=True) + d_rot
        P = O.project(means, quats, torch.exp(p["scales"]) + d_scal, viewmat[0], K[0], W, H)
        n = pts.shape[0]
        return R.with_lists(P.means2d, P.conics, torch.sigmoid(p["opacities"]).reshape(-1), P.depths, P.radii,
                            torch.zeros(n, 8), ["step"] * n, W, H)  # fmt: skip


# ---------------------------------------------------------------------------------------------------------------------
# the two contracts


def bit_failures(tag, runs):
    """``runs``: one dict of tensors per run.  -> a line per (run, tensor) that is not ``torch.equal`` to the first run's."""
    out = []
    for i, r in enumerate(runs[1:], 1):
        assert set(r) == set(runs[0])
        out += [f"{tag}: run {i} differs from run 0 in {n} elements of {name}" for name, n in differing(runs[0], r).items()]
    return out


def order_failures(tag, runs, k, bound):
    """``runs``: the [N,16] record gradients of several runs; ``k`` [N]; ``bound`` [N,16] (``order_bound``).  Rows with
    k <= 2 must be equal bit for bit in all runs; over the others no slot may spread, between any two runs, by more than its
    bound (which is 0 where nothing accumulates)."""
    g = torch.stack([r.detach().cpu() for r in runs])
    out = []
    if not bool(torch.isfinite(g).all()):
        out.append(f"{tag}: a gradient is not finite")
    exact = k <= 2
    moved = (g != g[:1]).any(dim=0).any(dim=1)
    bad = (moved & exact).nonzero().flatten()
    if bad.numel():
        out.append(f"{tag}: {bad.numel()} rows with k <= 2 are not bit-equal across runs, first row {int(bad[0])} (k = {int(k[bad[0]])})")
    spread = g.double().max(dim=0).values - g.double().min(dim=0).values
    over = ((spread > bound) & ~exact[:, None]).any(dim=1).nonzero().flatten()
    if over.numel():
        r = int(over[0])
        out.append(f"{tag}: {over.numel()} rows with k >= 3 spread beyond 2 (k - 1) 2^-24 A, first row {r} (k = {int(k[r])}): "
                   f"spread / bound per slot {[f'{float(s):.2e}/{float(b):.2e}' for s, b in zip(spread[r, :11], bound[r, :11])]}")  # fmt: skip
    return out
