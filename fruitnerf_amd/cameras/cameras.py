"""Per-image cameras of a real dataset: a minimal stand-in for `nerfstudio.cameras.cameras.Cameras`.

The reference's dataparser (fruit_nerf/data/fruitnerf_dataparser.py:86-131, 226-273) reads `fl_x, fl_y, cx, cy` per
dataset or per frame and COLMAP's OPENCV coefficients `k1..k4, p1, p2`, and builds
`Cameras(fx, fy, cx, cy, distortion_params, height, width, camera_to_worlds, camera_type)`.  nerfstudio is not
installable here, so this class carries the same field names; a real `Cameras` can be passed wherever one is taken
(duck typing, as rays.py does) — `camera_table_of` / `generate_rays_of` read attributes only.

Ray generation runs in libfruitnerf_hip.so (fnr_camera_rays; training draws through fnr_train_prologue_cams): the
camera model is the contract of include/fruitnerf_hip.h (fnr_camera_table).  Only PERSPECTIVE cameras; fisheye and
equirectangular ones raise.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple, Union

import torch
from torch import Tensor

PERSPECTIVE = 1     # nerfstudio.cameras.cameras.CameraType.PERSPECTIVE.value


def _camera_type_values(camera_type, n: int) -> list:
    """camera_type as nerfstudio stores it (an enum, an int, or an [M,1] tensor of enum values) -> list of ints."""
    if camera_type is None:
        return [PERSPECTIVE]
    if isinstance(camera_type, Tensor):
        return [int(v) for v in camera_type.reshape(-1).tolist()]
    if isinstance(camera_type, (list, tuple)):
        return [int(getattr(v, "value", v)) for v in camera_type]
    return [int(getattr(camera_type, "value", camera_type))]


def _column(v: Union[float, Tensor], n: int, name: str) -> Tensor:
    """A scalar (per dataset) or [M] / [M,1] (per frame) value -> float32 [M,1]."""
    t = torch.as_tensor(v, dtype=torch.float32).reshape(-1, 1)
    if t.shape[0] == 1:
        t = t.expand(n, 1)
    if t.shape[0] != n:
        raise ValueError(f"{name}: {t.shape[0]} values for {n} cameras")
    return t.contiguous()


def _check_perspective(camera_type, n: int) -> None:
    bad = sorted(set(v for v in _camera_type_values(camera_type, n) if v != PERSPECTIVE))
    if bad:
        raise NotImplementedError(f"camera_type {bad}: only PERSPECTIVE cameras (pinhole + OpenCV radial / tangential "
                                  "distortion) are generated on the device; fisheye and equirectangular are not")


class Cameras:
    """camera_to_worlds [M,3,4]; fx, fy, cx, cy [M,1] (given per dataset as scalars or per frame); distortion_params
    [M,6] (k1, k2, k3, k4, p1, p2) or None; height, width ints (set-wide); camera_type PERSPECTIVE."""

    def __init__(self, camera_to_worlds: Tensor, fx, fy, cx, cy, width: int, height: int,
                 distortion_params: Optional[Tensor] = None, camera_type=PERSPECTIVE):
        c2w = torch.as_tensor(camera_to_worlds, dtype=torch.float32)
        if c2w.dim() != 3 or c2w.shape[1:] != (3, 4):
            raise ValueError(f"camera_to_worlds is [M,3,4], got {tuple(c2w.shape)}")
        n = c2w.shape[0]
        _check_perspective(camera_type, n)
        self.camera_to_worlds = c2w
        self.fx, self.fy = _column(fx, n, "fx"), _column(fy, n, "fy")
        self.cx, self.cy = _column(cx, n, "cx"), _column(cy, n, "cy")
        self.width, self.height = int(width), int(height)
        self.camera_type = camera_type
        if distortion_params is not None:
            d = torch.as_tensor(distortion_params, dtype=torch.float32)
            if d.dim() == 1:
                d = d[None].expand(n, -1)
            if d.shape != (n, 6):
                raise ValueError(f"distortion_params is [M,6] (k1, k2, k3, k4, p1, p2), got {tuple(d.shape)}")
            distortion_params = d.contiguous()
        self.distortion_params = distortion_params

    def __len__(self) -> int:
        return self.camera_to_worlds.shape[0]

    def rescale_output_resolution(self, scale: float) -> None:
        """Nerfstudio's Cameras.rescale_output_resolution, in place: fx, fy, cx, cy are multiplied by `scale` and the
        image becomes floor(height * scale) x floor(width * scale)."""
        scale = float(scale)
        if not scale > 0.0:
            raise ValueError(f"rescale_output_resolution: scale {scale} must be positive")
        height, width = math.floor(self.height * scale), math.floor(self.width * scale)
        if height < 1 or width < 1:
            raise ValueError(f"rescale_output_resolution: scale {scale} leaves a {height} x {width} image")
        self.fx, self.fy, self.cx, self.cy = self.fx * scale, self.fy * scale, self.cx * scale, self.cy * scale
        self.height, self.width = height, width

    def camera_table(self, device):
        return camera_table_of(self, device)

    def generate_rays(self, camera_indices: int, rows: Optional[Tuple[int, int]] = None):
        return generate_rays_of(self, camera_indices, rows)


def _image_size(cameras) -> Tuple[int, int]:
    """(H, W) of a camera set: ints here, [M,1] tensors in nerfstudio (which must then agree: H, W are set-wide)."""
    out = []
    for v in (cameras.height, cameras.width):
        if isinstance(v, Tensor):
            if not bool((v == v.reshape(-1)[0]).all()):
                raise NotImplementedError("per-image height / width: the image set has one H x W")
            v = v.reshape(-1)[0]
        out.append(int(v))
    return out[0], out[1]


def camera_table_of(cameras, device):
    """K.CameraTableArg (intrinsics [M,4], distortion [M,6] | None) of a Cameras / nerfstudio Cameras on `device`."""
    from .. import _kernels as K
    n = cameras.camera_to_worlds.shape[0]
    _check_perspective(getattr(cameras, "camera_type", None), n)
    cols = [_column(getattr(cameras, k), n, k).to(device) for k in ("fx", "fy", "cx", "cy")]
    dist = getattr(cameras, "distortion_params", None)
    return K.CameraTableArg(torch.cat(cols, dim=1), None if dist is None else dist.to(device))


def generate_rays_of(cameras, camera_index: int, rows: Optional[Tuple[int, int]] = None):
    """Full-image RayBundle of camera `camera_index`, shape [H, W] (or the row block rows = (y0, y1): what sharding.py
    splits an evaluation image by), camera_indices filled, pixel_area None.  The cameras' tensors must be on the HIP
    device (fnr_camera_rays; no CPU path)."""
    from .. import _kernels as K
    from ..rays import RayBundle
    n = cameras.camera_to_worlds.shape[0]
    _check_perspective(getattr(cameras, "camera_type", None), n)
    i = int(camera_index)
    if not 0 <= i < n:
        raise IndexError(f"camera {i} of {n}")
    H, W = _image_size(cameras)
    y0, y1 = (0, H) if rows is None else (int(rows[0]), int(rows[1]))
    c2w = cameras.camera_to_worlds[i]
    dev = c2w.device
    intr = torch.cat([_column(getattr(cameras, k), n, k)[i] for k in ("fx", "fy", "cx", "cy")]).to(dev)
    dist = getattr(cameras, "distortion_params", None)
    o, d = K.camera_rays(c2w, intr, None if dist is None else dist[i], H, W, y0, y1)
    cam = torch.full((y1 - y0, W, 1), i, dtype=torch.int32, device=dev)
    return RayBundle(o.view(y1 - y0, W, 3), d.view(y1 - y0, W, 3), None, cam)
