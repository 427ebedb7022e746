"""The reference's optional bilateral-grid colour correction (default off): ``use_bilateral_grid`` /
``color_corrected_metrics`` of ``freegaussian/freegaussian_model.py:122-126``, used at ``:227-233`` (one grid per
training image), ``:617-618`` (its parameter group), ``:879-882`` (applied to the rendered image while training),
``:935-937`` / ``:1024-1045`` (colour-corrected PSNR) and ``:988-989`` (10 x total variation of the grids).

The reference imports these four names from ``nerfstudio.model_components.lib_bilagrid`` -- a third-party dependency
(nerfstudio, pinned ``>= 1.1.3`` in the reference's pyproject) that is NOT in ``/root/reference`` and not installed
here.  This file restates that library's published algorithm ("Bilateral Guided Radiance Field Processing", Wang et
al. 2024: a per-image 3-D grid of 3x4 affine colour transforms, sliced at (x, y, luma) with trilinear interpolation)
with the same names, arguments and tensor layouts.  **Parity unpinned**: there is no golden vector for it in the
reference and the library cannot be run here; ``tests/test_bilagrid.py`` checks it against a scalar restatement of
trilinear slicing and against the properties the algorithm defines (identity grids, affine recovery).

Torch ops by default: an image-sized ``grid_sample`` plus a 3x4 multiply per pixel, off the section-8 hot path and off by
default.  ``FG_FUSED_BILAGRID=1`` (opt-in) sends ``apply_to_render`` -- the slice of a whole rendered image, the one use on
the training path -- through ``ops.bilagrid_apply`` instead (csrc/bilagrid.hip: one streaming launch forward, the grid
gradient as a gather with a fixed order of addition, no per-pixel matrices in memory; measured in
profiles/bilagrid_fused.md).  ``FG_FUSED_COLOR_CORRECT=1`` (opt-in) sends ``color_correct`` -- the metric-side fit, whose
torch statement copies fifteen float64 feature matrices to the host per image -- through ``ops.color_correct`` instead
(csrc/color_correct.hip: the normal equations summed on the device, measured in profiles/color_correct_fused.md).  ``slice``
at free coordinates and ``total_variation_loss`` are torch ops either way."""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch
import torch.nn.functional as F
from torch import nn


def color_affine_transform(affine_mats: torch.Tensor, rgb: torch.Tensor) -> torch.Tensor:
    """``affine_mats`` [..., 3, 4] applied to ``rgb`` [..., 3]: A[:, :3] rgb + A[:, 3]."""
    return torch.matmul(affine_mats[..., :3], rgb.unsqueeze(-1)).squeeze(-1) + affine_mats[..., 3]


def total_variation_loss(x: torch.Tensor) -> torch.Tensor:
    """Mean squared forward difference of a batch of 3-D grids [B, C, L, H, W] along L, H and W, summed over the
    three axes and averaged over the batch."""
    tv = x.new_zeros(())
    for axis in (2, 3, 4):
        n = x.shape[axis]
        a = x.narrow(axis, 1, n - 1)
        b = x.narrow(axis, 0, n - 1)
        count = max(a[0].numel(), 1)
        tv = tv + (a - b).pow(2).sum() / count
    return tv / x.shape[0]


class BilateralGrid(nn.Module):
    """``num`` grids of 3x4 affine colour transforms, [num, 12, grid_W, grid_Y, grid_X], initialised to the identity.
    ``forward(grid_xy, rgb, idx)`` slices them at (x, y, luma(rgb)) and returns the per-pixel matrices [..., 3, 4]."""

    def __init__(self, num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8):
        super().__init__()
        self.grid_width = grid_W
        eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
        self.grids = nn.Parameter(eye.view(1, 12, 1, 1, 1).repeat(num, 1, grid_W, grid_Y, grid_X))
        self.register_buffer("rgb2gray_weight", torch.tensor([[0.299, 0.587, 0.114]]))

    def rgb2gray(self, rgb: torch.Tensor) -> torch.Tensor:
        """Luma in [-1, 1] (the guidance coordinate of the slice)."""
        return (rgb @ self.rgb2gray_weight.T) * 2.0 - 1.0

    def tv_loss(self) -> torch.Tensor:
        return total_variation_loss(self.grids)

    def forward(self, grid_xy: torch.Tensor, rgb: torch.Tensor, idx: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``grid_xy`` [N, h, w, 2] in [0, 1]; ``rgb`` [N, h, w, 3]; ``idx`` [N] or [N, 1] picks the grids."""
        grids = self.grids
        if idx is not None:
            grids = grids[idx.reshape(-1)]
        assert grids.shape[0] == grid_xy.shape[0], (grids.shape, grid_xy.shape)
        lead = grid_xy.shape[:-1]
        xyz = torch.cat([(grid_xy - 0.5) * 2.0, self.rgb2gray(rgb)], dim=-1)  # [N,h,w,3] in [-1,1]: (x, y, luma)
        xyz = xyz.reshape(xyz.shape[0], 1, -1, 1, 3) if xyz.dim() != 4 else xyz.unsqueeze(1)  # [N,1,h,w,3]
        mats = F.grid_sample(grids, xyz, mode="bilinear", align_corners=True, padding_mode="border")  # [N,12,1,h,w]
        mats = mats.permute(0, 2, 3, 4, 1)
        return mats.reshape(*lead, 3, 4)


def slice(bil_grids: BilateralGrid, xy: torch.Tensor, rgb: torch.Tensor, grid_idx: torch.Tensor) -> Dict[str, torch.Tensor]:  # noqa: A001
    """(the library's name) Slice grid ``grid_idx`` at pixel coordinates ``xy`` in [0, 1] guided by ``rgb`` and apply
    the sliced transforms: {"rgb", "rgb_affine_mats"}.  Inputs without a batch axis get one."""
    shape = rgb.shape
    if xy.dim() == 2:  # [P,2] -> [1,P,1,2]
        xy, rgb = xy[None, :, None], rgb[None, :, None]
    elif xy.dim() == 3:  # [h,w,2]
        xy, rgb = xy[None], rgb[None]
    grid_idx = grid_idx.reshape(-1)
    if grid_idx.numel() == 1 and xy.shape[0] != 1:
        grid_idx = grid_idx.expand(xy.shape[0])
    mats = bil_grids(xy, rgb, grid_idx)
    out = color_affine_transform(mats, rgb)
    return {"rgb": out.reshape(shape), "rgb_affine_mats": mats.reshape(*shape[:-1], 3, 4)}


def fused_bilagrid() -> bool:
    """``FG_FUSED_BILAGRID`` (opt-in; read here and nowhere else, on the host, on every call): unset or ``0`` = the torch ops,
    ``1`` = the fused slice where it applies.  Anything else is an error, not a silent default."""
    knob = os.environ.get("FG_FUSED_BILAGRID", "0")
    if knob not in ("0", "1"):
        raise ValueError(f"FG_FUSED_BILAGRID wants 0 or 1, got {knob!r}")
    return knob == "1"


def fused_applies(bil_grids: BilateralGrid, rgb: torch.Tensor) -> bool:
    """Does ``apply_to_render`` take the fused call for this image?  Only with the knob set, CUDA float32 tensors, a grid
    shape and an image size the library takes (its own queries say), one image of at least 2 x 2 pixels."""
    if not fused_bilagrid():
        return False
    grids = bil_grids.grids
    if not (grids.is_cuda and rgb.is_cuda and grids.dtype == torch.float32 and rgb.dtype == torch.float32):
        return False
    if rgb.dim() not in (3, 4) or rgb.shape[-1] != 3 or (rgb.dim() == 4 and rgb.shape[0] != 1):
        return False
    H, W = int(rgb.shape[-3]), int(rgb.shape[-2])
    from . import _lib

    lib = _lib.load()
    _, _, GL, GY, GX = grids.shape
    return H >= 2 and W >= 2 and bool(lib.fg_bilagrid_supported(GX, GY, GL)) and lib.fg_bilagrid_bwd_workspace_bytes(H, W, GX, GY, GL) > 0


def apply_to_render(bil_grids: BilateralGrid, rgb: torch.Tensor, cam_idx: int, H: int, W: int) -> torch.Tensor:
    """What the reference's base class does with a rendered image [1, H, W, 3] of training camera ``cam_idx``
    (``_apply_bilateral_grid``, called at ``freegaussian_model.py:882``): a [0, 1]^2 pixel grid, one slice.  With
    ``FG_FUSED_BILAGRID=1`` and tensors the fused kernels take (``fused_applies``): ``ops.bilagrid_apply``."""
    if fused_applies(bil_grids, rgb) and tuple(rgb.shape[-3:-1]) == (int(H), int(W)):
        from . import ops

        return ops.bilagrid_apply(bil_grids.grids, int(cam_idx), rgb.reshape(int(H), int(W), 3)).reshape(rgb.shape)
    dev = rgb.device
    gy, gx = torch.meshgrid(torch.linspace(0, 1.0, H, device=dev), torch.linspace(0, 1.0, W, device=dev), indexing="ij")
    grid_xy = torch.stack([gx, gy], dim=-1).unsqueeze(0)
    return slice(bil_grids, grid_xy, rgb, torch.tensor([int(cam_idx)], device=dev, dtype=torch.long))["rgb"]


def fused_color_correct() -> bool:
    """``FG_FUSED_COLOR_CORRECT`` (opt-in; read here and nowhere else, on the host, on every call): unset or ``0`` = the torch
    ops, ``1`` = the fused fit where it applies.  Anything else is an error, not a silent default."""
    knob = os.environ.get("FG_FUSED_COLOR_CORRECT", "0")
    if knob not in ("0", "1"):
        raise ValueError(f"FG_FUSED_COLOR_CORRECT wants 0 or 1, got {knob!r}")
    return knob == "1"


def fused_color_correct_applies(img: torch.Tensor, ref: torch.Tensor, num_iters, eps) -> bool:
    """Does ``color_correct`` take the fused call for this pair?  Only with the knob set, CUDA float32 tensors of one shape
    on one device, 3 channels, arguments in the range the library takes, and nothing that wants a gradient."""
    if not fused_color_correct():
        return False
    if not (img.is_cuda and ref.is_cuda and img.device == ref.device and img.dtype == torch.float32 and ref.dtype == torch.float32):
        return False
    if img.dim() < 1 or img.shape != ref.shape or img.shape[-1] != 3 or img.numel() == 0:
        return False
    if torch.is_grad_enabled() and (img.requires_grad or ref.requires_grad):
        return False
    from . import ops

    return ops.color_correct_supported(img.numel(), num_iters, eps)


def color_correct(img: torch.Tensor, ref: torch.Tensor, num_iters: int = 5, eps: float = 0.5 / 255) -> torch.Tensor:
    """Warp ``img`` to match the colours of ``ref`` with a per-channel quadratic colour transform fitted by least
    squares on the pixels that are unclipped in both, re-fitted ``num_iters`` times (the metric-side correction of the
    bilateral-grid paper, after mip-NeRF 360's).

    With ``FG_FUSED_COLOR_CORRECT=1`` and tensors the fused call takes (``fused_color_correct_applies``):
    ``ops.color_correct``, the same iteration with each fit solved from its float64 normal equations on the device (the
    contract is in include/fgraster.h).  The two agree within the parity bar where every fit has full rank.  They DIFFER
    where the feature matrix has exactly zero columns (an image channel that is 0 everywhere): there the default driver of
    ``torch.linalg.lstsq`` below (gelsy) reports rank 1 and returns something that is not a least-squares solution, while
    the fused path returns a least-squares fit (zero weights on the zero columns).  On a grey image (r = g = b) the
    fits are rank 3 and then near-deficient, and no two solvers agree: no parity is claimed there."""
    if img.shape[-1] != ref.shape[-1]:
        raise ValueError(f"img's {img.shape[-1]} and ref's {ref.shape[-1]} channels must match")
    if fused_color_correct_applies(img, ref, num_iters, eps):
        from . import ops

        return ops.color_correct(img, ref, num_iters=num_iters, eps=eps)
    C = img.shape[-1]
    x = img.reshape(-1, C)
    y = ref.reshape(-1, C)

    def unclipped(z):
        return (z >= eps) & (z <= 1 - eps)

    mask0 = unclipped(x)
    for _ in range(num_iters):
        cols = [x[:, c : c + 1] * x[:, c:] for c in range(C)]  # the quadratic terms
        cols += [x, torch.ones_like(x[:, :1])]  # linear + bias
        A = torch.cat(cols, dim=-1)
        warp = []
        for c in range(C):
            b = y[:, c]
            m = mask0[:, c] & unclipped(x[:, c]) & unclipped(b)
            Am = torch.where(m[:, None], A, torch.zeros_like(A))
            bm = torch.where(m, b, torch.zeros_like(b))
            w = torch.linalg.lstsq(Am.double().cpu(), bm.double().cpu()[:, None]).solution[:, 0]
            assert bool(torch.isfinite(w).all())
            warp.append(w.to(x))
        x = torch.clamp(A @ torch.stack(warp, dim=-1), 0, 1)
    return x.reshape(img.shape)
