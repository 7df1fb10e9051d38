"""TSDF volume of the mesh export: Nerfstudio's `exporter/tsdf_utils.py::TSDF` (what `ns-export tsdf` fuses rendered depth
into), as recalled — nerfstudio is not available to this project, so the contract is the one stated in
include/fruitnerf_hip.h (fnr_tsdf_volume).  Fusion and surface extraction run in libfruitnerf_hip.so (csrc/tsdf.hip): one
launch per batch of cameras, and marching tetrahedra in place of scikit-image's Lewiner marching cubes (whose case tables
this project cannot carry), so the mesh differs from Nerfstudio's in its triangulation, not in its surface."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from .. import _kernels as K
from .. import _lib as L


class TSDF:
    """values / weights [nx,ny,nz] and colors [nx,ny,nz,3] over the nodes lo + (i,j,k) * voxel_size of the box [lo, hi]
    (voxel_size = (hi - lo) / dims), initialised to -1 / 0 / 0.  truncation = truncation_margin * voxel_size.x.

    depth_kind: L.FNR_TSDF_DEPTH_RAY — the depth images hold the distance along each pixel's ray (this model's "depth"
    output; the default here) — or L.FNR_TSDF_DEPTH_Z — they hold z-depth, which is what Nerfstudio compares.
    max_weight 1 is Nerfstudio's clamp; a large value gives the plain running average over the cameras."""

    def __init__(self, lo: Sequence[float], hi: Sequence[float], volume_dims: Union[int, Sequence[int]], device,
                 truncation_margin: float = 5.0, max_weight: float = 1.0, depth_kind: int = L.FNR_TSDF_DEPTH_RAY):
        dims = [int(volume_dims)] * 3 if isinstance(volume_dims, int) else [int(v) for v in volume_dims]
        if len(dims) != 3:
            raise ValueError(f"volume_dims: one int or three, got {volume_dims!r}")
        self.device = torch.device(device)
        self.lo = torch.as_tensor(lo, dtype=torch.float32).reshape(3).cpu()
        self.hi = torch.as_tensor(hi, dtype=torch.float32).reshape(3).cpu()
        self.truncation_margin, self.max_weight, self.depth_kind = float(truncation_margin), float(max_weight), depth_kind
        self.values = torch.full(dims, -1.0, device=self.device)
        self.weights = torch.zeros(dims, device=self.device)
        self.colors = torch.zeros(dims + [3], device=self.device)
        self._arg = K.TsdfVolumeArg(self.values, self.weights, self.colors, self.lo.tolist(), self.hi.tolist(),
                                    self.truncation_margin, self.max_weight)

    @classmethod
    def from_aabb(cls, aabb, volume_dims, device=None, **kwargs) -> "TSDF":
        """aabb: [2,3] = box minimum, box maximum (Nerfstudio's TSDF.from_aabb)."""
        aabb = torch.as_tensor(aabb, dtype=torch.float32)
        if aabb.shape != (2, 3):
            raise ValueError(f"aabb is [2,3] (minimum, maximum), got {tuple(aabb.shape)}")
        return cls(aabb[0], aabb[1], volume_dims, aabb.device if device is None else device, **kwargs)

    @property
    def volume_dims(self) -> Tuple[int, int, int]:
        return tuple(self.values.shape)

    @property
    def voxel_size(self) -> Tensor:
        return (self.hi - self.lo) / torch.tensor(self.volume_dims, dtype=torch.float32)

    @property
    def truncation(self) -> float:
        return float(torch.tensor(self.truncation_margin, dtype=torch.float32) * self.voxel_size[0])

    def integrate(self, c2w: Tensor, intrinsics: Tensor, depth_images: Tensor, color_images: Tensor,
                  mask_images: Optional[Tensor] = None) -> None:
        """Fuses a batch of cameras in the order given.  c2w [n,3,4]; intrinsics [n,4] = fx, fy, cx, cy or [n,3,3]
        pinhole matrices; depth_images [n,H,W] (or [n,H,W,1]); color_images [n,H,W,3]; mask_images [n,H,W] (or
        [n,H,W,1]), zero / False = leave the pixel out.  Batches may be split freely: the volume is the same bit for bit."""
        if intrinsics.dim() == 3:
            intrinsics = torch.stack([intrinsics[:, 0, 0], intrinsics[:, 1, 1], intrinsics[:, 0, 2], intrinsics[:, 1, 2]], 1)
        if depth_images.dim() == 4:
            depth_images = depth_images[..., 0]
        if mask_images is not None and mask_images.dim() == 4:
            mask_images = mask_images[..., 0]
        K.tsdf_integrate(self._arg, c2w, intrinsics, depth_images, color_images, mask_images, self.depth_kind)

    def get_mesh(self):
        """-> vertices [V,3] (world units), faces [F,3] int32, normals [V,3], colors [V,3], on the device.  Vertices
        ascend by edge key, faces by (cell, tetrahedron, triangle): the same volume gives the same arrays."""
        return K.tsdf_mesh(self._arg)

    def get_triangle_mesh(self):
        """get_mesh() as an export.mesh.TriangleMesh (connected components, selection, writing)."""
        from .mesh import TriangleMesh
        vertices, faces, normals, colors = self.get_mesh()
        return TriangleMesh(vertices, faces, normals, colors)

    def export(self, path: str) -> None:
        from . import ply
        vertices, faces, normals, colors = self.get_mesh()
        ply.write_triangle_mesh(str(path), vertices.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy(),
                                colors.cpu().numpy())
