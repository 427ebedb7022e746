"""Plain-torch restatement of the view-DP gradient exchange kernels (a helper, not a test; nothing of the package
under test is imported here):

    rebuild      v[i,k,:] = scale * sum_v basis_k(dir_v(i)) * g_v[i,:]        (fg_sh_grad_accumulate / _split)
    compact      rows with a non-zero g, as (id, payload row), in ascending id (fg_payload_compact)

The 16 basis values of a direction come from ``oracle.raster_oracle.sh_eval`` fed an identity coefficient table
(coefficient k of "channel" c is 1 where k == c): its 16 "colours" are then the basis values themselves, and the ones
of k >= (degree+1)^2 are zero because sh_eval never touches them.  sh_eval normalises the direction it is given; band l
of the basis is a homogeneous polynomial of degree l, so basis_k(d) = |d|^l basis_k(d/|d|) gives the value AT a carried
direction (payload_floats == 6: the kernel evaluates the polynomial at the fp32 direction it received, which is a unit
vector only up to fp32 rounding)."""
import torch

from oracle import raster_oracle as O

BAND = torch.tensor([0] + [1] * 3 + [2] * 5 + [3] * 7)  # the band l of coefficient k


def basis(degree: int, dirs: torch.Tensor, at_given_length: bool = False) -> torch.Tensor:
    """dirs [M,3] -> [M,16] in dirs' dtype: basis_k(dirs/|dirs|), or basis_k(dirs) itself (``at_given_length``);
    columns k >= (degree+1)^2 are zero."""
    eye = torch.eye(16, dtype=dirs.dtype).expand(dirs.shape[0], 16, 16)
    b = O.sh_eval(degree, dirs, eye)
    if at_given_length:
        n = torch.sqrt(((dirs[:, 0] * dirs[:, 0] + dirs[:, 1] * dirs[:, 1]) + dirs[:, 2] * dirs[:, 2]))
        b = b * n[:, None] ** BAND.to(dirs.dtype)[None, :]
    return b


def _view_terms(means, payload_views, degree, payload_floats, dtype):
    """Per view: (basis [N,16], g [N,3], live [N]) in ``dtype``; rows whose g is all zero are not live and their
    direction (which may be anything, NaN included) is not looked at."""
    if payload_floats not in (3, 6):
        raise ValueError("payload_floats is 3 or 6")
    out = []
    for g, second in payload_views:
        g = g.detach().cpu().to(dtype)
        live = (g != 0).any(dim=1)
        if payload_floats == 3:  # second = the camera position [3]
            d = means.detach().cpu().to(dtype) - second.detach().cpu().to(dtype)[None, :]
        else:  # second = the carried unit directions [N,3]
            d = second.detach().cpu().to(dtype)
        d = torch.where(live[:, None], d, torch.tensor([0.0, 0.0, 1.0], dtype=dtype)[None, :])
        out.append((basis(degree, d, at_given_length=(payload_floats == 6)), g, live))
    return out


def rebuild(means, payload_views, degree, k_stored, scale, payload_floats, dtype=torch.float64):
    """-> v [N, k_stored, 3] in ``dtype`` (CPU).  ``payload_views``: one (g [N,3], camera position [3]) per view for
    payload_floats == 3 (direction = normalize(means - camera)), one (g [N,3], unit direction [N,3]) per view for
    payload_floats == 6.  A view whose g row is all zero adds nothing to that row."""
    if not (0 <= degree <= 3 and (degree + 1) ** 2 <= k_stored <= 16):
        raise ValueError("degree 0..3, (degree+1)^2 <= k_stored <= 16")
    n = payload_views[0][0].shape[0]
    v = torch.zeros(n, 16, 3, dtype=dtype)
    for b, g, live in _view_terms(means, payload_views, degree, payload_floats, dtype):
        v = v + torch.where(live[:, None, None], b[:, :, None] * g[:, None, :], torch.zeros((), dtype=dtype))
    return (v * torch.tensor(scale, dtype=dtype))[:, :k_stored].contiguous()


def rebuild64(means, payload_views, degree, k_stored, scale, payload_floats):
    return rebuild(means, payload_views, degree, k_stored, scale, payload_floats, torch.float64)


def forward_magnitude64(means, payload_views, degree, scale, payload_floats):
    """-> [N] float64: |scale| * sum_v ||basis(dir_v(i))|| ||g_v[i]||, the size of what row i of the rebuild adds up
    (no cancellation between views): the yardstick of the per-row error bound."""
    n = payload_views[0][0].shape[0]
    m = torch.zeros(n, dtype=torch.float64)
    for b, g, live in _view_terms(means, payload_views, degree, payload_floats, torch.float64):
        m = m + torch.where(live, b.norm(dim=1) * g.norm(dim=1), torch.zeros((), dtype=torch.float64))
    return m * abs(scale)


def row_error_ratio(v, v64, magnitude):
    """max over the rows with a non-zero magnitude of ||v[i] - v64[i]|| / magnitude[i]  (0.0 if there is none)."""
    err = (v.detach().cpu().double() - v64).flatten(1).norm(dim=1)
    live = magnitude > 0
    return float((err[live] / magnitude[live]).max()) if bool(live.any()) else 0.0


def compact(dense_rows: torch.Tensor):
    """dense_rows [N,pf] float32 -> (ids int64 [count] ascending, rows [count,pf]): the rows whose first three floats
    are not all zero -- ``nonzero`` plus a gather."""
    ids = (dense_rows[:, :3] != 0).any(dim=1).nonzero().flatten()
    return ids, dense_rows[ids]
