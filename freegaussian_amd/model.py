"""Host-side mirror of the reference's model surface around the raster call.

``FreeGaussianModel.get_outputs(camera)`` here reproduces rows H1-H4 + O1 of SURVEY.md §8a --
the ~50 lines of reference ``freegaussian/freegaussian_model.py:753-898`` that assemble the
inputs of ``rasterization(...)`` and post-process its outputs -- and S1 (``after_train_iter``,
:369-392).  ``FreeGaussianControlModel.get_outputs`` mirrors the stage-2 variant
(``freegaussian_control_model.py:52-209``).  nerfstudio is not a dependency: ``Camera`` is a
minimal stand-in for the fields of ``nerfstudio.cameras.Cameras`` the reference touches, and
``nerfstudio_adapter.py`` registers the methods only if nerfstudio imports.

Everything here is plain torch (small elementwise ops and the MLP GEMMs); the raster itself is
the HIP library behind ``freegaussian_amd.rasterization``."""
from __future__ import annotations

import contextlib
import copy
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Union

import torch
from torch import nn

from .deform import FreeGaussianControllableModel, FreeGaussianDeformableModel, fused_applies, fused_control, fused_se3
from .rasterization import num_sh_bases, rasterization
from .utils import get_viewmat, knn_mean_distance, random_quat_tensor, resize_image, transform_points


@dataclass
class Camera:
    """One pinhole camera (the reference asserts a batch of exactly one, :773)."""

    camera_to_worlds: torch.Tensor  # [1,3,4] OpenGL convention (nerfstudio)
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int
    times: Optional[torch.Tensor] = None  # [1,1]
    metadata: Dict = field(default_factory=dict)

    @property
    def shape(self):
        return (self.camera_to_worlds.shape[0],)

    def rescale_output_resolution(self, s: float) -> None:
        """In place, like nerfstudio's Cameras.rescale_output_resolution with its default
        ``scale_rounding_mode="floor"``: intrinsics scale linearly, the image size is floored --
        the same ``H // d`` the ground truth gets from ``resize_image`` (utils.py:248-261), so
        render and target agree in shape at every size (1014 rows at d = 4 -> 253, not 254).
        (nerfstudio's source is not readable here: SURVEY.md citation discipline -- the default is
        recalled; the shape agreement with ``get_gt_img`` is what the tests pin.)"""
        self.fx, self.fy, self.cx, self.cy = self.fx * s, self.fy * s, self.cx * s, self.cy * s
        # s is 1 / 2^k or 2^k: the product is exact in floating point, floor is safe
        self.width = int(self.width * s)
        self.height = int(self.height * s)

    def get_intrinsics_matrices(self) -> torch.Tensor:
        return torch.tensor([[[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]]])


@dataclass
class OrientedBox:
    """Stand-in for ``nerfstudio.data.scene_box.OrientedBox`` as ``set_crop`` / ``get_outputs`` use
    it (:397-398, :779-783): any object with ``within(points[N,3]) -> bool[N] or [N,1]`` works.
    R [3,3] rotation, T [3] centre, S [3] full side lengths (recalled layout; nerfstudio's source is
    not readable here)."""

    R: torch.Tensor
    T: torch.Tensor
    S: torch.Tensor

    def within(self, pts: torch.Tensor) -> torch.Tensor:
        R, T, S = (x.to(pts) for x in (self.R, self.T, self.S))
        local = (pts - T) @ R  # = R^T (p - T) per row
        return ((local > -S / 2) & (local < S / 2)).all(dim=-1, keepdim=True)


@dataclass
class FreeGaussianModelConfig:
    """Raster-relevant subset of reference FreeGaussianModelConfig (:51-131), same names/defaults."""

    warm_up: int = 3000
    refine_every: int = 100
    resolution_schedule: int = 3000
    background_color: str = "random"
    num_downscales: int = 2
    sh_degree_interval: int = 1000
    sh_degree: int = 3
    stop_split_at: int = 15000
    # adaptive density control (:58-88), consumed by freegaussian_amd.densify.refinement_after
    refine_start: int = 500
    cull_alpha_thresh: float = 0.1
    cull_scale_thresh: float = 0.5
    continue_cull_post_densification: bool = True
    reset_alpha_every: int = 30
    densify_grad_thresh: float = 0.0008
    densify_size_thresh: float = 0.01
    n_split_samples: int = 2
    cull_screen_size: float = 0.15
    split_screen_size: float = 0.05
    stop_screen_size_at: int = 4000
    output_depth_during_training: bool = False
    ssim_lambda: float = 0.2  # (:96)
    use_scale_regularization: bool = False  # (:102; the PhysGaussian ratio penalty, every 10th step)
    max_gauss_ratio: float = 10.0  # (:104)
    use_bilateral_grid: bool = False  # (:122; per-image affine colour grids, freegaussian_amd/bilagrid.py)
    grid_shape: tuple = (16, 16, 8)  # (:124; X, Y, W)
    color_corrected_metrics: bool = False  # (:126)
    rasterize_mode: str = "classic"
    num_random: int = 50000
    random_scale: float = 10.0
    # build extension: fold the SH cat, exp / sigmoid / quaternion
    # normalisation (+ MLP deltas) and the background composite + clamp into the HIP passes
    fused_front_end: bool = True
    # build extension: flow-supervised stage-1 training (INTEGRATION.md "Flow supervision").  0 = off: nothing below is looked at.
    # Above 0, a training camera whose metadata["cameras0"] is a camera of its own with times adds the composited Gaussian flow
    # (ops.flow_displacement as two extra raster channels) to the outputs, and get_loss_dict adds
    # flow_loss_weight * ops.flow_l1 against batch["flows"].
    flow_loss_weight: float = 0.0
    # False: batch["flows"] is interflow (camera flow already removed: what the reference's loader delivers), both frames are
    # projected under the current camera; True: raw optical flow, frame 0 is projected under cameras0's pose
    flow_camera_motion: bool = False
    # False: the frame-0 means are evaluated under no_grad (the gradient-free fused MLP forward where that applies)
    flow_frame0_grad: bool = True


# where get_loss_dict / get_metrics_dict leave the fused target call's (image, mask, l1, ssim, mse) in the outputs dict
FUSED_TARGET_KEY = "_fused_target"
_EVAL_BACKGROUND = {"random": torch.tensor([0.1490, 0.1647, 0.2157]), "white": torch.ones(3), "black": torch.zeros(3)}

_POSE_RING = None


def _pose_slot():
    """(tensor[25], its numpy view) of the next slot of a ring of pinned staging buffers for viewmat + K."""
    global _POSE_RING
    if _POSE_RING is None:
        ring = torch.empty(64, 32, dtype=torch.float32).pin_memory()
        _POSE_RING = [ring, ring.numpy(), 0]
    ring, ring_np, i = _POSE_RING
    _POSE_RING[2] = (i + 1) % ring.shape[0]
    return ring[i, :25], ring_np[i, :25]


# Per-step bookkeeping attributes (plain tensors / ints, never Parameters or sub-modules) are set past
# nn.Module.__setattr__, whose parameter / buffer / module checks cost ~5 us a time, six times a step.
_plain_set = object.__setattr__


def _se3_fused_for(pts: torch.Tensor, times: torch.Tensor) -> bool:
    """Whether the deformation's heads move ``pts`` through ``ops.se3_apply``: ``FG_FUSED_SE3=1`` (``deform.fused_se3``) and
    CUDA float32 tensors, at least one row.  Taped or not."""
    if not fused_se3():
        return False
    return pts.is_cuda and times.is_cuda and pts.dtype == times.dtype == torch.float32 and pts.dim() == 2 and pts.shape[0] >= 1


def _se3_apply(w: torch.Tensor, v: torch.Tensor, pts: torch.Tensor) -> torch.Tensor:
    from . import ops

    return ops.se3_apply(w, v, pts)


def fused_control_applies(means: torch.Tensor, gaussian_mask: torch.Tensor, crop: Optional[torch.Tensor], plan=None) -> bool:
    """Whether stage 2's control stage runs through the ``ops.control_*`` calls: ``FG_FUSED_CONTROL=1``
    (``deform.fused_control``), CUDA float32 means and a CUDA bool mask [N,M] of 1 <= M <= 32 attributes on one device, and no
    active crop (a crop changes the rows on every call: the torch ops keep it).  With the mask's ``plan`` (``ops.control_plan``,
    or a callable that returns it, called only once everything above holds) also: at least one row, and every attribute with
    at least one (the reference's empty attribute is a NaN that poisons every value; the torch ops keep that behaviour)."""
    if not fused_control() or crop is not None:
        return False
    if not (means.is_cuda and gaussian_mask.is_cuda and means.device == gaussian_mask.device and means.dtype == torch.float32):
        return False
    if gaussian_mask.dtype != torch.bool or gaussian_mask.dim() != 2 or gaussian_mask.shape[0] != means.shape[0]:
        return False
    if not 1 <= gaussian_mask.shape[1] <= 32:
        return False
    if plan is None:
        return True
    return (plan() if callable(plan) else plan).refusal() is None


def _mask_key(mask: torch.Tensor):
    """Changes whenever the mask does: another tensor, an in-place edit, another shape, another device."""
    return (mask.data_ptr(), mask._version, tuple(mask.shape), mask.device)


class FreeGaussianModel(nn.Module):
    """Gaussian parameter store + deform/control MLPs + ``get_outputs``."""

    def __init__(self, config: Optional[FreeGaussianModelConfig] = None, num_points: Optional[int] = None,
                 seed_points: Optional[torch.Tensor] = None, is_blender: bool = True,
                 init_scales: Optional[float] = None, num_train_data: Optional[int] = None,
                 device: Optional[Union[str, torch.device]] = None):  # fmt: skip
        """``num_train_data``: the number of training images (one bilateral grid each, :227-233).  ``init_scales``: None = the reference's initial scales, the mean distance to the three nearest neighbours
        (:158-162; on the GPU ``ops.knn``; on the CPU a tree query over all points with scikit-learn,
        quadratic brute force without); a float = that log-scale everywhere, for harnesses
        that overwrite the scales anyway.  ``device``: where every parameter is created and where the neighbour search
        runs; the random draws still come from the CPU generator in the same order, so a seed gives the same model on
        either device.  None = as before, the CPU -- or, for CUDA ``seed_points``, their device."""
        super().__init__()
        self.config = config or FreeGaussianModelConfig()
        if device is None and seed_points is not None and seed_points.is_cuda:
            device = seed_points.device
        on = (lambda t: t) if device is None else (lambda t: t.to(device))
        if seed_points is not None:
            means = on(seed_points.float())
        else:
            n = num_points or self.config.num_random
            means = on((torch.rand(n, 3) - 0.5) * self.config.random_scale)
        n = means.shape[0]
        dim_sh = num_sh_bases(self.config.sh_degree)
        # layout and activations of reference gauss_params (:187-196): log-scales, logit-opacities
        self.gauss_params = nn.ParameterDict(
            {
                "means": nn.Parameter(means),
                "scales": nn.Parameter(torch.log(knn_mean_distance(means, 3)).repeat(1, 3) if init_scales is None
                                       else on(torch.full((n, 3), float(init_scales)))),
                "quats": nn.Parameter(on(random_quat_tensor(n))),
                "features_dc": nn.Parameter(on(torch.rand(n, 3))),
                "features_rest": nn.Parameter(on(torch.zeros(n, dim_sh - 1, 3))),
                "opacities": nn.Parameter(on(torch.logit(0.1 * torch.ones(n, 1)))),
            }
        )
        self.deform = on(FreeGaussianDeformableModel(is_blender=is_blender))  # :198
        self.control = on(FreeGaussianControllableModel())  # :200
        if self.config.use_bilateral_grid:  # (:227-233)
            from .bilagrid import BilateralGrid

            if not num_train_data:
                raise ValueError("use_bilateral_grid needs num_train_data (one grid per training image)")
            gx, gy, gw = self.config.grid_shape
            self.bil_grids = on(BilateralGrid(num=int(num_train_data), grid_X=gx, grid_Y=gy, grid_W=gw))
        self.step = 0
        # (:221-226) Viser's default grey for "random", else the named colour: what an eval render composites over with
        # background "random" (:653), and the colour of the empty-crop output in every mode (:782)
        self.background_color = _EVAL_BACKGROUND[self.config.background_color].clone()
        self.xys: Optional[torch.Tensor] = None
        self.radii: Optional[torch.Tensor] = None
        self.xys_grad_norm: Optional[torch.Tensor] = None
        self.vis_counts: Optional[torch.Tensor] = None
        self.max_2Dsize: Optional[torch.Tensor] = None
        self.last_size = (1, 1)
        self.last_list_length = 0
        self.crop_box = None  # (:220) set through set_crop by the viewer / render scripts
        self._active_crop: Optional[torch.Tensor] = None

    def set_crop(self, crop_box) -> None:
        """(:397-398)"""
        self.crop_box = crop_box

    @staticmethod
    def get_empty_outputs(width: int, height: int, background: torch.Tensor):
        """(:641-646) what an eval render returns when the crop box holds no Gaussian."""
        rgb = background.repeat(height, width, 1)
        depth = background.new_ones(*rgb.shape[:2], 1) * 10
        accumulation = background.new_zeros(*rgb.shape[:2], 1)
        return {"rgb": rgb, "depth": depth, "accumulation": accumulation, "background": background}

    def _crop_ids(self):
        """Eval-only crop (:778-785): None = all Gaussians; an all-False mask = empty output."""
        if self.crop_box is None or self.training:
            return None
        return self.crop_box.within(self.gauss_params["means"]).reshape(-1)

    # -- accessors with the reference's names -------------------------------------------------
    def _p(self, name: str) -> torch.Tensor:
        """A Gaussian parameter; inside a cropped eval render, its rows within the crop box (the
        reference's ``*_crop`` tensors, :786-798)."""
        t = self.gauss_params[name]
        return t if self._active_crop is None else t[self._active_crop]

    means = property(lambda self: self._p("means"))
    scales = property(lambda self: self._p("scales"))
    quats = property(lambda self: self._p("quats"))
    features_dc = property(lambda self: self._p("features_dc"))
    features_rest = property(lambda self: self._p("features_rest"))
    opacities = property(lambda self: self._p("opacities"))
    num_points = property(lambda self: self.gauss_params["means"].shape[0])
    device = property(lambda self: self.gauss_params["means"].device)

    def load_state_dict(self, state_dict, **kwargs):  # type: ignore[override]
        """(:278-291) the Gaussian parameters are re-allocated to the checkpoint's count, legacy
        un-prefixed names are remapped, and -- as in the reference -- the step jumps to 30000 (SH
        degree maxed, warm-up over)."""
        self.step = 30000
        state_dict = dict(state_dict)
        if "means" in state_dict:
            for p in ("means", "scales", "quats", "features_dc", "features_rest", "opacities"):
                state_dict[f"gauss_params.{p}"] = state_dict.pop(p)
        if "gauss_params.means" in state_dict:
            newp = state_dict["gauss_params.means"].shape[0]
            for name, param in self.gauss_params.items():
                new_shape = (newp,) + tuple(param.shape[1:])
                if tuple(param.shape) != new_shape:
                    self.gauss_params[name] = nn.Parameter(torch.zeros(new_shape, device=param.device))
        return super().load_state_dict(state_dict, **kwargs)

    # -- H3 ---------------------------------------------------------------------------------------
    def _get_downscale_factor(self) -> int:
        """2^max(num_downscales - step // resolution_schedule, 0) while training, else 1 (:626-633)."""
        if self.training:
            return 2 ** max(self.config.num_downscales - self.step // self.config.resolution_schedule, 0)
        return 1

    def _get_background_color(self) -> torch.Tensor:
        """(:648-660)"""
        mode = self.config.background_color
        if mode == "random":
            return torch.rand(3, device=self.device) if self.training else self.background_color.to(self.device)
        if mode == "white":
            return torch.ones(3, device=self.device)
        if mode == "black":
            return torch.zeros(3, device=self.device)
        raise ValueError(f"Unknown background color {mode}")

    def get_gt_img(self, image: torch.Tensor) -> torch.Tensor:
        """(:900-909)"""
        if image.dtype == torch.uint8:
            image = image.float() / 255.0
        d = self._get_downscale_factor()
        return (resize_image(image, d) if d > 1 else image).to(self.device)

    def composite_with_background(self, image: torch.Tensor, background: torch.Tensor) -> torch.Tensor:
        """(:911-922) a ground-truth image with an alpha channel over the step's background colour."""
        if image.shape[2] == 4:
            alpha = image[..., -1].unsqueeze(-1).repeat((1, 1, 3))
            return alpha * image[..., :3] + (1 - alpha) * background
        return image

    def _fused_target(self, outputs, batch):
        """``FG_FUSED_TARGET=1`` (``harness.fused_target``) and a batch the fused call takes (``harness.fused_target_applies``):
        (L1, SSIM, squared error) of ``outputs["rgb"]`` against the target that the raw batch image stands for, through one
        ``ops.target_loss`` -- no target tensor is built.  Else None: the torch ops.  ``get_loss_dict`` and
        ``get_metrics_dict`` share the call: whichever runs first leaves (image, mask, l1, ssim, mse) in ``outputs`` under
        ``FUSED_TARGET_KEY``, and the other takes it where image and mask are the same objects (a call made without a tape is
        not reused by one that needs the gradient)."""
        from . import harness

        if not harness.fused_target():
            return None
        image, mask, pred = batch["image"], batch.get("mask"), outputs["rgb"]
        taped = pred.requires_grad and torch.is_grad_enabled()
        kept = outputs.get(FUSED_TARGET_KEY)
        if kept is not None and kept[0] is image and kept[1] is mask and (kept[2].requires_grad or not taped):
            return kept[2:]
        d = self._get_downscale_factor()
        bg = outputs["background"]
        if not harness.fused_target_applies(pred, image, mask, d):
            return None
        if image.shape[-1] == 4 and not (bg.is_cuda and bg.device == pred.device and bg.dtype == torch.float32 and bg.numel() == 3):
            return None
        from . import ops

        vals = ops.target_loss(pred, image, bg if image.shape[-1] == 4 else None, mask, d)
        outputs[FUSED_TARGET_KEY] = (image, mask) + tuple(vals)
        return vals

    def get_metrics_dict(self, outputs, batch):
        """(:924-941) without the colour-corrected variant and the camera optimizer (mode "off", :120).  With
        ``FG_FUSED_TARGET=1`` and no colour-corrected metrics the squared error is ``_fused_target``'s (the colour-corrected
        pair needs the target as a tensor and keeps the torch statement)."""
        fused = None if self.config.color_corrected_metrics else self._fused_target(outputs, batch)
        if fused is not None:
            return {"psnr": -10.0 * torch.log10(fused[2]), "gaussian_count": self.num_points}
        gt_rgb = self.composite_with_background(self.get_gt_img(batch["image"]), outputs["background"])
        mse = torch.nn.functional.mse_loss(outputs["rgb"], gt_rgb)
        metrics = {"psnr": -10.0 * torch.log10(mse)}
        if self.config.color_corrected_metrics:  # (:935-937)
            from .bilagrid import color_correct

            cc = color_correct(outputs["rgb"].detach(), gt_rgb)
            metrics["cc_psnr"] = -10.0 * torch.log10(torch.nn.functional.mse_loss(cc, gt_rgb))
        metrics["gaussian_count"] = self.num_points
        return metrics

    @torch.no_grad()
    def get_image_metrics_and_images(self, outputs, batch):
        """(:1005-1051) the evaluation metrics of one rendered image against its composited ground truth, as Python floats,
        and the side-by-side image: ({"psnr", "ssim"[, "cc_psnr", "cc_ssim"]}, {"img": [H, 2W, 3]}).  PSNR as
        ``get_metrics_dict`` computes it; SSIM through ``harness.l1_and_ssim`` (the fused kernel on the GPU, ``harness.ssim``
        on the host: the definition of the reference's pytorch_msssim callable); the colour-corrected pair with
        ``config.color_corrected_metrics``, through ``bilagrid.color_correct`` (``FG_FUSED_COLOR_CORRECT`` decides its path).
        **LPIPS is not mirrored**: the reference's third metric needs the ``lpips`` / ``torchmetrics`` packages and the
        weights of a trained network, none of which this project ships; the ``lpips`` and ``cc_lpips`` keys are absent,
        not faked."""
        from .harness import l1_and_ssim

        gt_rgb = self.composite_with_background(self.get_gt_img(batch["image"]), outputs["background"])
        predicted_rgb = outputs["rgb"].detach()
        combined_rgb = torch.cat([gt_rgb, predicted_rgb], dim=1)
        mse = torch.nn.functional.mse_loss(predicted_rgb, gt_rgb)
        metrics = {"psnr": float((-10.0 * torch.log10(mse)).item()), "ssim": float(l1_and_ssim(predicted_rgb, gt_rgb)[1])}
        if self.config.color_corrected_metrics:  # (:1024-1026, :1040-1047)
            from .bilagrid import color_correct

            cc_rgb = color_correct(predicted_rgb, gt_rgb)
            metrics["cc_psnr"] = float((-10.0 * torch.log10(torch.nn.functional.mse_loss(cc_rgb, gt_rgb))).item())
            metrics["cc_ssim"] = float(l1_and_ssim(cc_rgb, gt_rgb)[1])
        return metrics, {"img": combined_rgb}

    def get_loss_dict(self, outputs, batch, metrics_dict=None):
        """(:944-990) main loss (1 - ssim_lambda) L1 + ssim_lambda (1 - SSIM) on the composited ground truth, the
        optional mask (both images blacked out), the optional scale-ratio regulariser on every 10th step, and while
        training with bilateral grids 10 x their total variation (:988-989).  The camera-optimizer term of the reference
        is not mirrored (mode "off" in every shipped config).  With ``FG_FUSED_TARGET=1`` and a batch
        the fused call takes, L1 and SSIM come from ``_fused_target`` and no target is built; the regulariser and the TV term
        are the same either way."""
        from .harness import l1_and_ssim

        fused = self._fused_target(outputs, batch)  # (FG_FUSED_TARGET=1: the target is never built)
        if fused is not None:
            l1, sim = fused[0], fused[1]
        else:
            gt_img = self.composite_with_background(self.get_gt_img(batch["image"]), outputs["background"])
            pred_img = outputs["rgb"]
            if "mask" in batch:
                d = self._get_downscale_factor()
                mask = batch["mask"]
                mask = (resize_image(mask.float(), d) if d > 1 else mask.float()).to(self.device)
                assert mask.shape[:2] == gt_img.shape[:2] == pred_img.shape[:2]
                gt_img = gt_img * mask
                pred_img = pred_img * mask
            l1, sim = l1_and_ssim(pred_img, gt_img)  # (fused on the GPU: ops.l1_ssim)
        flow_term = self._flow_loss(outputs, batch)
        simloss = 1 - sim
        if self.config.use_scale_regularization and self.step % 10 == 0:
            scale_exp = torch.exp(self.scales)
            ratio = scale_exp.amax(dim=-1) / scale_exp.amin(dim=-1)
            limit = torch.tensor(self.config.max_gauss_ratio, device=ratio.device)
            scale_reg = 0.1 * (torch.maximum(ratio, limit) - self.config.max_gauss_ratio).mean()
        elif fused is not None:
            scale_reg = torch.zeros((), device=self.device)  # (a fill, not a host-to-device copy: the fused path never waits for the host)
        else:
            scale_reg = torch.tensor(0.0, device=self.device)
        lam = self.config.ssim_lambda
        loss_dict = {"main_loss": (1 - lam) * l1 + lam * simloss, "scale_reg": scale_reg}
        if self.training and self.config.use_bilateral_grid:
            from .bilagrid import total_variation_loss

            loss_dict["tv_loss"] = 10 * total_variation_loss(self.bil_grids.grids)
        if flow_term is not None:
            loss_dict["flow_loss"] = flow_term
        return loss_dict

    def _flow_loss(self, outputs, batch):
        """``flow_loss_weight`` x the masked L1 of ``outputs["flow"]`` against ``batch["flows"]`` ([H0,W0,2], full-resolution
        pixels; flow.py has the convention) through one ``ops.flow_l1`` -- the downscale, the mask's box mean and the weights of
        non-finite source pixels are formed inside the call, nothing is read back.  None where the outputs carry no flow or the
        batch no flows: the key is then absent."""
        if "flow" not in outputs or "flows" not in batch:
            return None
        from . import ops

        flows = torch.as_tensor(batch["flows"]).to(self.device, torch.float32).contiguous()
        mask = batch.get("mask")
        if mask is not None:
            mask = mask.to(self.device).contiguous()
        return self.config.flow_loss_weight * ops.flow_l1(outputs["flow"], flows, mask, self._get_downscale_factor())

    # -- the pieces of get_outputs shared by stage 1 and stage 2 ------------------------------------
    def _camera_setup(self, camera: Camera):
        """viewmat, K, W, H at the scheduled resolution (:806-815)."""
        cam0 = camera.metadata.get("cameras0")
        if cam0 is not None and cam0 is not camera:  # (:802-804)
            assert bool((cam0.get_intrinsics_matrices() == camera.get_intrinsics_matrices()).all()), \
                "Intrinsics matrices should be the same"
        s = self._get_downscale_factor()
        # Without a cameras0 of its own the reference aliases it to the camera (:769-770) and rescales that one object
        # twice (:807-808): a d^2 render at d > 1.  Training cameras always carry their own (the data parser's), so the
        # alias only matters to a viewer render at training time; here the camera is rescaled once.
        # The reference rescales by 1/s and later by s (:807-808, :813-814).  With floor rounding that
        # does not restore a size that s does not divide (1014 -> 253 -> 1012): its camera objects
        # shrink once and, one schedule step later, render 506 rows against a 507-row target.  Here the
        # cameras get their own sizes back exactly, so render and get_gt_img agree at every step.
        saved = [(c, (c.fx, c.fy, c.cx, c.cy, c.width, c.height)) for c in ((camera, cam0) if cam0 is not None and cam0 is not camera else (camera,))]
        camera.rescale_output_resolution(1 / s)
        if cam0 is not None and cam0 is not camera:  # (:808, :814) rescaled and restored alongside
            cam0.rescale_output_resolution(1 / s)
        c2w = camera.camera_to_worlds
        if c2w.is_cuda or self.device.type != "cuda":
            viewmat = get_viewmat(c2w.to(self.device))
            K = camera.get_intrinsics_matrices().to(self.device)
        else:
            # host-side pose: 25 floats through a pinned buffer, asynchronously.  A pageable
            # `.to(device)` blocks the host until the queue has drained, i.e. until the previous
            # step's backward has finished -- the host could then never run ahead of the GPU.
            # The staging words come from a ring of pinned slots: a slot is written again 64 camera set-ups later, and
            # the host is never that far ahead of the queue (every render waits for its own list length).
            stage, stage_np = _pose_slot()
            stage[:16] = get_viewmat(c2w.float()).reshape(-1)
            stage_np[16:] = (camera.fx, 0.0, camera.cx, 0.0, camera.fy, camera.cy, 0.0, 0.0, 1.0)
            dev = stage.to(self.device, non_blocking=True)
            viewmat, K = dev[:16].view(1, 4, 4), dev[16:].view(1, 3, 3)
        W, H = int(camera.width), int(camera.height)
        _plain_set(self, "last_size", (H, W))
        for c, (fx, fy, cx, cy, w, h) in saved:
            c.fx, c.fy, c.cx, c.cy, c.width, c.height = fx, fy, cx, cy, w, h
        return viewmat, K, W, H

    def _colors_and_degree(self):
        """(:801, :826-830)"""
        colors = torch.cat((self.features_dc[:, None, :], self.features_rest), dim=1)
        if self.config.sh_degree > 0:
            return colors, min(self.step // self.config.sh_degree_interval, self.config.sh_degree)
        return torch.sigmoid(colors), None

    def _render_mode(self) -> str:
        if self.config.rasterize_mode not in ("antialiased", "classic"):
            raise ValueError("Unknown rasterize_mode: %s", self.config.rasterize_mode)
        return "RGB+ED" if (self.config.output_depth_during_training or not self.training) else "RGB"

    def _rasterize_and_finish(self, means, quats, scales, colors, sh_degree, viewmat, K, W, H, extra_channels=None):
        """The raster call with the reference's exact kwargs (:847-868) and O1 (:869-898).  ``extra_channels`` [N,2] (the flow
        branch): composited behind the render-mode channels and returned as ``"flow"``, a view of the render."""
        render_mode = self._render_mode()
        render, alpha, info = rasterization(
            means=means,
            quats=quats,
            scales=scales,
            opacities=torch.sigmoid(self.opacities).squeeze(-1),
            colors=colors,
            viewmats=viewmat,
            Ks=K,
            width=W,
            height=H,
            tile_size=16,
            packed=False,
            near_plane=0.01,
            far_plane=1e10,
            render_mode=render_mode,
            sh_degree=sh_degree,
            sparse_grad=False,
            absgrad=True,
            rasterize_mode=self.config.rasterize_mode,
            **({} if extra_channels is None else {"extra_channels": extra_channels}),
        )
        if self.training and info["means2d"].requires_grad:
            info["means2d"].retain_grad()
        _plain_set(self, "xys", info["means2d"])  # [1,N,2]
        _plain_set(self, "radii", info["radii"][0])  # [N]
        _plain_set(self, "last_list_length", int(info["raster_flatten_ids"].numel()))  # (the capacity, in static-shape mode)
        background = self._get_background_color()
        rgb = torch.clamp(render[..., :3] + (1 - alpha) * background, 0.0, 1.0)
        if render_mode == "RGB+ED":
            depth = render[..., 3:4]
            depth = torch.where(alpha > 0, depth, depth.detach().max()).squeeze(0)
        else:
            depth = None
        if not self.training:
            background = background.expand(H, W, 3)
        out = {"rgb": rgb.squeeze(0), "depth": depth, "accumulation": alpha.squeeze(0), "background": background}
        if extra_channels is not None:
            out["flow"] = render[0, :, :, render.shape[-1] - 2 :]
        return out

    def _render(self, means, d_rotation, d_scaling, viewmat, K, W, H, extra_channels=None):
        """Activations (:801, :826-830, :844-851) + raster call + O1, either folded into the HIP
        passes (``fused_front_end``; SH path only) or spelled out in torch exactly like the
        reference."""
        if self.config.fused_front_end and self.config.sh_degree > 0:
            return self._rasterize_raw_and_finish(means, d_rotation, d_scaling, viewmat, K, W, H, extra_channels)
        colors, sh_degree = self._colors_and_degree()
        scales = torch.exp(self.scales) + d_scaling
        quats = self.quats / self.quats.norm(dim=-1, keepdim=True) + d_rotation
        return self._rasterize_and_finish(means, quats, scales, colors, sh_degree, viewmat, K, W, H, extra_channels)

    def _rasterize_raw_and_finish(self, means, d_rotation, d_scaling, viewmat, K, W, H, extra_channels=None):
        from .rasterization import rasterize_gauss_params

        render_mode = self._render_mode()
        background = self._get_background_color()
        sh_degree = min(self.step // self.config.sh_degree_interval, self.config.sh_degree)
        rgb, alpha, info = rasterize_gauss_params(
            means, self.quats, self.scales, self.opacities, self.features_dc, self.features_rest, viewmat, K, W, H,
            sh_degree,
            d_quats=d_rotation if torch.is_tensor(d_rotation) else None,
            d_scales=d_scaling if torch.is_tensor(d_scaling) else None,
            background=background, clamp=True, near_plane=0.01, far_plane=1e10, tile_size=16,
            render_mode=render_mode, absgrad=True, rasterize_mode=self.config.rasterize_mode,
            **({} if extra_channels is None else {"extra_channels": extra_channels}),
        )  # fmt: skip
        if self.training and info["means2d"].requires_grad:
            info["means2d"].retain_grad()
        _plain_set(self, "xys", info["means2d"])
        _plain_set(self, "radii", info["radii"][0])
        _plain_set(self, "last_list_length", int(info["raster_flatten_ids"].numel()))  # (the capacity, in static-shape mode)
        if render_mode == "RGB+ED":
            depth = rgb[..., 3:4]
            depth = torch.where(alpha > 0, depth, depth.detach().max()).squeeze(0)
        else:
            depth = None
        if not self.training:
            background = background.expand(H, W, 3)
        # (a full-width slice is still a SliceBackward node: a zeros + a copy launch in every backward)
        out = {"rgb": (rgb if rgb.shape[-1] == 3 else rgb[..., :3]).squeeze(0), "depth": depth, "accumulation": alpha.squeeze(0),
               "background": background}  # fmt: skip
        if extra_channels is not None:
            out["flow"] = rgb[0, :, :, rgb.shape[-1] - 2 :]
        return out

    # -- H1 + H4 -----------------------------------------------------------------------------------
    def get_outputs(self, camera: Camera) -> Dict[str, Union[torch.Tensor, List, None]]:
        if not isinstance(camera, Camera):
            print("Called get_outputs with not a camera")
            return {}
        if "cameras0" not in camera.metadata:
            camera.metadata["cameras0"] = camera
        if self.training:
            assert camera.shape[0] == 1, "Only one camera at a time"
        crop = self._crop_ids()
        if crop is not None and int(crop.sum()) == 0:  # (:781-782)
            return self.get_empty_outputs(int(camera.width), int(camera.height), self.background_color.to(self.device))
        _plain_set(self, "_active_crop", crop)
        try:
            return self._get_outputs_on_active_rows(camera)
        finally:
            _plain_set(self, "_active_crop", None)

    def _get_outputs_on_active_rows(self, camera: Camera):
        viewmat, K, W, H = self._camera_setup(camera)
        cam0 = self.flow_camera0(camera)
        if cam0 is None:
            return self._bilateral(self._outputs_from(viewmat, K, W, H, camera.times), camera)
        # the flow branch: frame 0's time, and its pose where the batch flows still hold the camera's motion
        viewmat0 = self._staged_viewmat(cam0) if self.config.flow_camera_motion else None
        return self._bilateral(self._outputs_from(viewmat, K, W, H, camera.times, flow=(cam0.times, viewmat0)), camera)

    def flow_camera0(self, camera: Camera) -> Optional[Camera]:
        """The frame-0 camera of the flow branch, or None where ``get_outputs`` does not take it.  It does while training with
        ``flow_loss_weight`` > 0 for a camera whose ``metadata["cameras0"]`` is a ``Camera`` of its own with ``times``, from
        ``warm_up`` on -- or from the first step with ``flow_camera_motion``: before the warm-up both frames have the same means,
        so under one camera the displacement is identically zero and carries no gradient."""
        cfg = self.config
        if not (self.training and cfg.flow_loss_weight > 0):
            return None
        cam0 = camera.metadata.get("cameras0") if camera.metadata is not None else None
        if not isinstance(cam0, Camera) or cam0 is camera or cam0.times is None or camera.times is None:
            return None
        if self.step < cfg.warm_up and not cfg.flow_camera_motion:
            return None
        return cam0

    def _staged_viewmat(self, camera: Camera) -> torch.Tensor:
        """``camera``'s world-to-camera matrix [1,4,4] on the device; a host-side pose goes through the pinned staging ring of
        ``_camera_setup``, asynchronously."""
        c2w = camera.camera_to_worlds
        if c2w.is_cuda or self.device.type != "cuda":
            return get_viewmat(c2w.to(self.device))
        stage, _ = _pose_slot()
        stage[:16] = get_viewmat(c2w.float()).reshape(-1)
        return stage[:16].to(self.device, non_blocking=True).view(1, 4, 4)

    def _flow_channels(self, means, flow, viewmat, K, W, H):
        """[N,2]: the displacement of every projected centre since frame 0 (``ops.flow_displacement``; margin = the longer image
        side).  The frame-0 means take the deformation path of the current ones, at ``cameras0``'s time; before the warm-up they
        are the means themselves."""
        from . import ops

        times0, viewmat0 = flow
        with contextlib.nullcontext() if self.config.flow_frame0_grad else torch.no_grad():
            means0 = self.means if self.step < self.config.warm_up else self._deformed(self.means, times0)[0]
        if not self.config.flow_frame0_grad:
            means0 = means0.detach()
        return ops.flow_displacement(means, means0, viewmat, viewmat0, K, W, H, near=0.01, margin=float(max(W, H)))

    def _bilateral(self, out, camera: Camera):
        """(:879-882) while training, the rendered image through the bilateral grid of its training camera."""
        if self.config.use_bilateral_grid and self.training and camera.metadata is not None and "cam_idx" in camera.metadata:
            from .bilagrid import apply_to_render

            rgb = out["rgb"]
            out["rgb"] = apply_to_render(self.bil_grids, rgb.unsqueeze(0), camera.metadata["cam_idx"], rgb.shape[0], rgb.shape[1]).squeeze(0)
        return out

    def _outputs_from(self, viewmat, K, W, H, times, flow=None):
        """H4 + the raster call on device-resident camera data: everything of ``get_outputs`` behind the host
        side of the camera (what ``graphed.GraphedModelStep`` captures).  ``flow``: None, or the flow branch's (frame-0 times,
        frame-0 viewmat or None for the current camera)."""
        if self.step < self.config.warm_up:
            means = self.means
            d_rotation, d_scaling = 0.0, 0.0
        else:
            means, d_rotation, d_scaling = self._deformed(self.means, times)
        if flow is None:
            return self._render(means, d_rotation, d_scaling, viewmat, K, W, H)
        return self._render(means, d_rotation, d_scaling, viewmat, K, W, H, self._flow_channels(means, flow, viewmat, K, W, H))

    def _deformed(self, pts, times):
        """(means, d_rotation, d_scaling) of ``pts`` (the undetached parameter) moved by the deformation net at ``times``."""
        times = times.to(self.device).expand(pts.shape[0], -1)
        if not torch.is_grad_enabled() and fused_applies(self.deform, pts, times):
            # (no gradient wanted: the fused forward applies the transform itself and never writes [N,4,4])
            return self.deform.deformed_points(pts.detach(), times)
        if _se3_fused_for(pts, times):
            # (FG_FUSED_SE3=1: the heads to the moved means in one launch, and one in the backward; pts is the
            #  undetached parameter, so its gradient arrives as it does below)
            w, v, d_rotation, d_scaling = self.deform.heads(pts.detach(), times)
            return _se3_apply(w, v, pts), d_rotation, d_scaling
        d_xyz, d_rotation, d_scaling = self.deform(pts.detach(), times)
        return transform_points(d_xyz, pts), d_rotation, d_scaling  # (:840-843; not torch.bmm: utils.small_bmm)

    @torch.no_grad()
    def get_outputs_for_camera(self, camera: Camera):
        """(:992-1003)"""
        return self.get_outputs(camera)

    # -- S1 -----------------------------------------------------------------------------------------
    def step_cb(self, step: int) -> None:
        self.step = step

    def after_train_iter(self, step: int) -> None:
        """Densification statistics from ``xys.absgrad`` and ``radii`` (:369-392)."""
        assert step == self.step
        if self.step >= self.config.stop_split_at:
            return
        with torch.no_grad():
            if self.xys_grad_norm is None:
                self.xys_grad_norm = torch.zeros(self.num_points, device=self.device)
                self.vis_counts = torch.ones(self.num_points, device=self.device)
            if self.max_2Dsize is None:
                self.max_2Dsize = torch.zeros(self.num_points, device=self.device)
            absgrad, radii = self.xys.absgrad[0], self.radii.flatten()
            if absgrad.is_cuda:
                # one pass over the Gaussians (csrc/densify.hip) instead of nine torch launches
                from . import ops

                ops.densify_stats(absgrad, radii, float(max(self.last_size)), self.xys_grad_norm, self.vis_counts, self.max_2Dsize)
                return
            # The reference indexes with the boolean mask (`x[visible] += ...`, :379-392): every such line is
            # a nonzero() with a host sync and a gather / scatter pair.  The same numbers with fixed shapes:
            # adding 0.0 and taking max(x, 0) with x >= 0 leave the invisible rows bit-for-bit as they were.
            visible = radii > 0
            grads = absgrad.norm(dim=-1)
            self.vis_counts += visible.to(self.vis_counts.dtype)
            self.xys_grad_norm += torch.where(visible, grads, torch.zeros_like(grads))
            new = radii.float() / float(max(self.last_size))
            self.max_2Dsize = torch.maximum(self.max_2Dsize, torch.where(visible, new, torch.zeros_like(new)))

    def get_gaussian_param_groups(self) -> Dict[str, List[nn.Parameter]]:
        return {k: [self.gauss_params[k]] for k in ("means", "scales", "quats", "features_dc", "features_rest", "opacities")}

    def get_param_groups(self) -> Dict[str, List[nn.Parameter]]:
        groups = self.get_gaussian_param_groups()
        groups["deform"] = list(self.deform.parameters())
        groups["control"] = list(self.control.parameters())
        if self.config.use_bilateral_grid:  # (:617-618)
            groups["bilateral_grid"] = list(self.bil_grids.parameters())
        return groups


class FreeGaussianControlModel(FreeGaussianModel):
    """Stage 2 (reference freegaussian_control_model.py): a frozen deform net supplies the mean
    displacement of each attribute's Gaussians; the control MLP turns it into per-Gaussian
    deltas scattered into the full set; then the same raster call."""

    def __init__(self, gaussian_mask: torch.Tensor, init_camera: Camera, **kw):
        super().__init__(**kw)
        self.register_buffer("gaussian_mask", gaussian_mask.bool())  # [N,M] (gaussian_mask_NxM.npy)
        self.init_camera = copy.deepcopy(init_camera)
        self.step = 30000  # load_state_dict forces this (:280): SH maxed, warm-up over
        self.control_values: Optional[torch.Tensor] = None  # viewer-supplied [M,3] when no cameras0

    def get_outputs(self, camera: Camera):
        if not isinstance(camera, Camera):
            print("Called get_outputs with not a camera")
            return {}
        crop = self._crop_ids()  # (freegaussian_control_model.py:73-86: the mask is cropped alongside)
        if crop is not None and int(crop.sum()) == 0:
            return self.get_empty_outputs(int(camera.width), int(camera.height), self.background_color.to(self.device))
        _plain_set(self, "_active_crop", crop)
        try:
            return self._get_outputs_on_active_rows(camera)
        finally:
            _plain_set(self, "_active_crop", None)

    def _get_outputs_on_active_rows(self, camera: Camera):
        viewmat, K, W, H = self._camera_setup(camera)
        means, d_rotation, d_scaling = self._control_stage(camera)
        return self._bilateral(self._render(means, d_rotation, d_scaling, viewmat, K, W, H), camera)  # (control model :190-193)

    def _control_plan(self):
        """``ops.control_plan`` of the mask, kept until the mask changes (``_mask_key``; the mask itself is kept with it, so
        that its address is not handed to another tensor meanwhile).  An edit that does not raise the mask's ``_version`` -- through
        ``mask.data``, or under ``torch.inference_mode`` -- is not seen: the plan stays that of the mask before it.  Assign a new
        tensor after such an edit."""
        from . import ops

        mask = self.gaussian_mask
        cached = self.__dict__.get("_control_plan_cache")
        if cached is None or cached[0] != _mask_key(mask):
            cached = (_mask_key(mask), ops.control_plan(mask), mask)
            _plain_set(self, "_control_plan_cache", cached)
        return cached[1]

    def _frozen_deformed(self, pts: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        """(:128-138) the selected rows moved by the frozen deformation net at time ``t``."""
        t = t.to(self.device).expand(pts.shape[0], -1)
        if fused_applies(self.deform, pts, t):
            return self.deform.deformed_points(pts, t)[0]
        if _se3_fused_for(pts, t):
            w, v, _, _ = self.deform.heads(pts, t)
            return _se3_apply(w, v, pts)
        T, _, _ = self.deform(pts, t)
        return transform_points(T, pts)

    def _control_stage(self, camera: Camera):
        """From the mask's rows to ``(means, d_rotation, d_scaling)``, the three full-N arrays of the raster call."""
        # (the plan is asked for only once the knob, the tensors and the crop allow the fused stage; it is kept, so the second
        #  look below costs a key comparison)
        if fused_control_applies(self.gauss_params["means"], self.gaussian_mask, self._active_crop, self._control_plan):
            return self._control_stage_fused(camera, self._control_plan())
        gmask = self.gaussian_mask if self._active_crop is None else self.gaussian_mask[self._active_crop]
        all_means, all_scales, all_quats = self.means, self.scales, self.quats
        sel = gmask.any(-1)
        pts = all_means[sel]
        pmask = gmask[sel]  # [n,M]
        if not self.training and "cameras0" not in camera.metadata and self.control_values is not None:
            d_avg = self.control_values.to(self.device)
        else:
            with torch.no_grad():  # (:128-138)
                delta = self._frozen_deformed(pts, camera.times) - self._frozen_deformed(pts, self.init_camera.times)
                d_avg = torch.stack([delta[pmask[:, i]].mean(0) for i in range(pmask.shape[1])])
        value = pmask.float() @ d_avg / pmask.sum(-1, keepdim=True)  # (:140)
        d_xyz, d_rot, d_scale = self.control(pts, value)
        idx = (sel.nonzero().squeeze(-1),)
        means = all_means + torch.zeros_like(all_means).index_put(idx, d_xyz)
        d_scaling = torch.zeros_like(all_scales).index_put(idx, d_scale)
        d_rotation = torch.zeros_like(all_quats).index_put(idx, d_rot)
        return means, d_rotation, d_scaling

    def _control_stage_fused(self, camera: Camera, plan):
        """``FG_FUSED_CONTROL=1``: the same stage on the mask's plan -- one ``index_select``, the two frozen-deform
        evaluations as above, then four small calls (csrc/control.hip) around the control MLP.  No boolean indexing, no
        ``nonzero``, no Python loop over the attributes: nothing is read back, so the host runs ahead of the GPU."""
        from . import ops

        all_means = self.means
        pts = all_means.index_select(0, plan.sel_index64)
        if not self.training and "cameras0" not in camera.metadata and self.control_values is not None:
            d_avg = self.control_values.to(device=self.device, dtype=torch.float32)
        else:
            with torch.no_grad():
                d_avg = ops.control_attr_mean(plan, self._frozen_deformed(pts, camera.times),
                                              self._frozen_deformed(pts, self.init_camera.times))  # fmt: skip
        value = ops.control_value_rows(plan, d_avg)
        d_xyz, d_rot, d_scale = self.control(pts, value)
        return ops.control_scatter(plan, all_means, d_xyz, d_rot, d_scale)

    def get_param_groups(self):
        groups = super().get_param_groups()
        groups.pop("deform")  # (:215-218)
        return groups
