#!/usr/bin/env python3
"""Flow maps for training from a directory of frames: ``ops.optical_flow`` (classical pyramidal Lucas-Kanade as HIP; NOT a
learned estimator -- its quality against one on real footage has not been measured) in place of the reference's mmflow step
(preprocess/epipolar_flow.py:367-372).  Needs a GPU, no network and nothing beyond PIL, numpy and torch.

    python scripts/make_flows.py DATA_DIR --interval K [--images images] [--grid current|frame0]
                                 [--transforms transforms.json --depths DEPTH_DIR]
                                 [--levels L --iters 4 --radius 3 --min-eig 1e-5 --consistency 1.0]

Frames are the PNG files of DATA_DIR/images in sorted order; frame i is paired with frame i - K.

  opticflow_n{K}/<frame>.png.npy   float32 [H,W,2], NaN where the estimate is invalid.  ``--grid current`` (the default): on
      frame i's grid, where the surface is now minus where it was K frames earlier (``flow.optical_flow_since``) -- the
      convention of ``batch["flows"]`` with ``flow_camera_motion=True`` and of ``masks.flow_motion_labels``.
      ``--grid frame0``: on frame i - K's grid, the layout mmflow returns (``flow.optical_flow_forward``).
  interflow_n{K}/<frame>.png.npy   with ``--transforms`` and ``--depths``: the forward flow plus the camera flow of frame
      i - K's depth under the relative motion of the two poses (``flow.relative_camera_motion``, ``flow.camera_flow_map``),
      written by ``io.save_interflow`` under the name of frame i, as the reference stores it.  Always on frame i - K's grid.

``transforms.json`` is the nerfstudio file: ``fl_x fl_y cx cy`` at the top (or per frame) and ``frames`` with ``file_path``
and ``transform_matrix``; a depth map is DEPTH_DIR/<frame stem>.npy, [H,W] or [H,W,1], inf where there is no surface."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def frame_files(image_dir: str):
    return sorted(f for f in os.listdir(image_dir) if f.lower().endswith(".png"))


def load_frame(path: str, dev) -> torch.Tensor:
    """uint8 [H,W,3] on the device; an alpha channel is composited over white first (the estimator takes 1 or 3 channels)."""
    from PIL import Image

    img = Image.open(path)
    if img.mode in ("RGBA", "LA") or "transparency" in img.info:
        rgba = np.asarray(img.convert("RGBA"), dtype=np.float32)
        rgb = rgba[..., :3] * (rgba[..., 3:] / 255.0) + 255.0 * (1.0 - rgba[..., 3:] / 255.0)
        arr = np.clip(np.rint(rgb), 0, 255).astype(np.uint8)
    else:
        arr = np.array(img.convert("RGB"), dtype=np.uint8)
    return torch.from_numpy(arr).to(dev)


def opticflow_path(data_dir: str, name: str, interval: int) -> str:
    return os.path.join(data_dir, f"opticflow_n{interval}", name + ".npy")


def read_transforms(path: str) -> dict:
    """{frame file name: (K float32 [3,3], c2w float64 [4,4])} of a nerfstudio transforms.json."""
    meta = json.load(open(path))
    out = {}
    for fr in meta["frames"]:
        g = lambda k: float(fr.get(k, meta.get(k)))  # noqa: E731
        K = torch.tensor([[g("fl_x"), 0.0, g("cx")], [0.0, g("fl_y"), g("cy")], [0.0, 0.0, 1.0]], dtype=torch.float32)
        out[os.path.basename(fr["file_path"])] = (K, torch.tensor(fr["transform_matrix"], dtype=torch.float64))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("data_dir")
    ap.add_argument("--interval", type=int, required=True)
    ap.add_argument("--images", default="images")
    ap.add_argument("--grid", choices=("current", "frame0"), default="current")
    ap.add_argument("--transforms")
    ap.add_argument("--depths")
    ap.add_argument("--levels", type=int)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--min-eig", type=float, default=1e-5)
    ap.add_argument("--consistency", type=float, default=1.0)
    ap.add_argument("--device", default="cuda", help="where the frames go (the estimator itself runs on a GPU only)")
    a = ap.parse_args(argv)
    if a.interval < 1:
        ap.error("--interval must be at least 1")
    if bool(a.transforms) != bool(a.depths):
        ap.error("--transforms and --depths go together")
    from freegaussian_amd import flow, io

    dev = torch.device(a.device)
    image_dir = os.path.join(a.data_dir, a.images)
    names = frame_files(image_dir)
    if len(names) <= a.interval:
        ap.error(f"{len(names)} PNG frames in {image_dir}: nothing is {a.interval} frames apart")
    kw = dict(levels=a.levels, iters=a.iters, radius=a.radius, min_eig=a.min_eig, consistency=a.consistency)
    poses = read_transforms(a.transforms) if a.transforms else None
    os.makedirs(os.path.dirname(opticflow_path(a.data_dir, names[0], a.interval)), exist_ok=True)
    frames = {}  # the last `interval` + 1 frames on the device
    for i, name in enumerate(names):
        frames[i] = load_frame(os.path.join(image_dir, name), dev)
        frames.pop(i - a.interval - 1, None)
        if i < a.interval:
            continue
        image0, image1 = frames[i - a.interval], frames[i]
        forward = flow.optical_flow_forward(image0, image1, **kw) if (a.grid == "frame0" or poses) else None
        out = forward if a.grid == "frame0" else flow.optical_flow_since(image0, image1, **kw)
        np.save(opticflow_path(a.data_dir, name, a.interval), out.cpu().numpy())
        line = f"{name}: {float(torch.isfinite(out).all(-1).float().mean()):.1%} valid"
        if poses:
            name0 = names[i - a.interval]
            (K, c2w0), (_, c2w1) = poses[name0], poses[name]
            depth0 = torch.from_numpy(np.load(os.path.join(a.depths, os.path.splitext(name0)[0] + ".npy"))).float().to(dev)
            veloc, omega = flow.relative_camera_motion(c2w0, c2w1)
            camera = flow.camera_flow_map(depth0, K.to(dev), veloc.float().to(dev), omega.float().to(dev))
            line += ", interflow -> " + io.save_interflow(a.data_dir, f"./images/{name}", a.interval, forward + camera)
        print(line)


if __name__ == "__main__":
    main()
