"""TriangleMesh: the mesh of the TSDF export as an object, with the Open3D calls its users follow the export with —
cluster_connected_triangles(), selection by face / vertex mask, removal of small components — as recalled (Open3D is not
available to this project; the contract is the one stated in include/fruitnerf_hip.h, "triangle-mesh connectivity").
Connectivity, statistics and selection run in libfruitnerf_hip.so (csrc/mesh.hip); there is no CPU path.

The filters those users call first — filter_smooth_laplacian / filter_smooth_taubin, compute_vertex_normals,
simplify_vertex_clustering — follow the section "triangle-mesh filters" of the same header (csrc/mesh_filters.hip): every
sum is a sequential float64 sum over a per-vertex row with a fixed order, so a filtered mesh has one defined bit pattern."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _kernels as K
from .. import _lib as L


@dataclass
class ComponentStats:
    """Per-component tensors on the mesh's device, C entries each (the fields of fnr_mesh_stats, and what Python forms
    from them).  volume is signed and means something only for a `closed` component with consistent winding."""
    n_faces: Tensor             # int32 [C]
    boundary_edges: Tensor      # int32 [C]: edges with one incidence
    nonmanifold_edges: Tensor   # int32 [C]: edges with three or more
    lo: Tensor                  # float32 [C,3]
    hi: Tensor                  # float32 [C,3]
    area: Tensor                # float64 [C]
    volume: Tensor              # float64 [C]
    moment: Tensor              # float64 [C,3]: sum of face area * face centroid
    centroid: Tensor            # float64 [C,3]: moment / area (NaN for a component without area)
    closed: Tensor              # bool [C]: boundary_edges == nonmanifold_edges == 0

    def __len__(self) -> int:
        return int(self.n_faces.shape[0])


class TriangleMesh:
    """vertices float32 [V,3], faces int32 [F,3] (indices in [0, V)), optional per-vertex normals / colors [V,3]; device
    tensors.  The mesh is immutable: every selection returns a new one."""

    def __init__(self, vertices: Tensor, faces: Tensor, normals: Optional[Tensor] = None, colors: Optional[Tensor] = None):
        L.require_gpu_tensor(vertices, "TriangleMesh vertices")
        L.require_gpu_tensor(faces, "TriangleMesh faces")
        if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
            raise ValueError(f"TriangleMesh: vertices are float32 [V,3], got {vertices.dtype} {tuple(vertices.shape)}")
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32 or faces.device != vertices.device:
            raise ValueError(f"TriangleMesh: faces are int32 [F,3] on the vertices' device, got {faces.dtype} "
                             f"{tuple(faces.shape)}")
        for name, t in (("normals", normals), ("colors", colors)):
            if t is not None and (t.shape != vertices.shape or t.device != vertices.device):
                raise ValueError(f"TriangleMesh: {name} are [V,3] on the vertices' device, got {tuple(t.shape)}")
        self.vertices, self.faces = vertices.contiguous(), faces.contiguous()
        self.normals = None if normals is None else normals.contiguous()
        self.colors = None if colors is None else colors.contiguous()
        self._components = None      # (face_component, n_components, workspace)
        self._stats = None
        self._adjacency = None       # (offsets, neighbours)
        self._vertex_faces = None    # (offsets, faces)
        self.vertex_cluster = None   # int32 [V of the source mesh]: set on the result of simplify_vertex_clustering

    @property
    def device(self):
        return self.vertices.device

    @property
    def n_vertices(self) -> int:
        return int(self.vertices.shape[0])

    @property
    def n_faces(self) -> int:
        return int(self.faces.shape[0])

    # ---- connectivity ---------------------------------------------------------------------------------------------------
    def connected_components(self) -> Tuple[Tensor, int]:
        """-> (face_component int32 [F], n_components); computed once."""
        if self._components is None:
            self._components = K.mesh_components(self.faces, self.n_vertices)
        return self._components[0], self._components[1]

    def component_stats(self) -> ComponentStats:
        if self._stats is None:
            labels, n = self.connected_components()
            s = K.mesh_component_stats(self.vertices, self.faces, labels, n, self._components[2])
            self._stats = ComponentStats(centroid=s["moment"] / s["area"][:, None],
                                         closed=(s["boundary_edges"] == 0) & (s["nonmanifold_edges"] == 0), **s)
        return self._stats

    def cluster_connected_triangles(self) -> Tuple[Tensor, Tensor, Tensor]:
        """Open3D's triple: (triangle_clusters int32 [F], cluster_n_triangles int32 [C], cluster_area float64 [C])."""
        labels, _ = self.connected_components()
        stats = self.component_stats()
        return labels, stats.n_faces, stats.area

    # ---- selection --------------------------------------------------------------------------------------------------------
    def select_by_face_mask(self, mask: Tensor) -> "TriangleMesh":
        """The faces with a set mask entry in their old order, and the vertices they reference in their old order."""
        faces, vertex_ids, _ = K.mesh_select(self.faces, self.n_vertices, mask)
        ids = vertex_ids.long()
        return TriangleMesh(self.vertices[ids], faces, None if self.normals is None else self.normals[ids],
                            None if self.colors is None else self.colors[ids])

    def select_by_vertex_mask(self, mask: Tensor) -> "TriangleMesh":
        """A face stays iff all three of its vertices pass."""
        if mask.shape != (self.n_vertices,):
            raise ValueError(f"select_by_vertex_mask: the mask is [V] = [{self.n_vertices}], got {tuple(mask.shape)}")
        L.require_gpu_tensor(mask, "select_by_vertex_mask mask")
        return self.select_by_face_mask((mask != 0)[self.faces.long()].all(dim=1))

    def _select_components(self, keep: Tensor) -> "TriangleMesh":
        labels, _ = self.connected_components()
        return self.select_by_face_mask(keep[labels.long()])

    def remove_small_components(self, min_faces: int) -> "TriangleMesh":
        """Without the components of fewer than min_faces faces."""
        if self.n_faces == 0:
            return self.select_by_face_mask(torch.zeros(0, dtype=torch.bool, device=self.device))
        return self._select_components(self.component_stats().n_faces >= int(min_faces))

    def keep_largest_components(self, k: int) -> "TriangleMesh":
        """The k components with the most faces; ties go to the smaller component index."""
        if self.n_faces == 0:
            return self.select_by_face_mask(torch.zeros(0, dtype=torch.bool, device=self.device))
        n = self.component_stats().n_faces
        order = torch.sort(n.long(), descending=True, stable=True).indices[:max(int(k), 0)]
        keep = torch.zeros_like(n, dtype=torch.bool)
        keep[order] = True
        return self._select_components(keep)

    # ---- filters ----------------------------------------------------------------------------------------------------------
    def vertex_adjacency(self) -> Tuple[Tensor, Tensor]:
        """-> (offsets int32 [V + 1], neighbours int32 [E]): row a holds every b != a that shares a face with a, once,
        ascending; computed once."""
        if self._adjacency is None:
            self._adjacency = K.mesh_vertex_rows(self.faces, self.n_vertices, K.MESH_ROWS_NEIGHBOURS)
        return self._adjacency

    def vertex_faces(self) -> Tuple[Tensor, Tensor]:
        """-> (offsets int32 [V + 1], faces int32 [E]): row a holds every face that lists a, once, ascending; computed once."""
        if self._vertex_faces is None:
            self._vertex_faces = K.mesh_vertex_rows(self.faces, self.n_vertices, K.MESH_ROWS_FACES)
        return self._vertex_faces

    def _smoothed(self, factors, weights: str) -> "TriangleMesh":
        offsets, neighbours = self.vertex_adjacency()
        mesh = TriangleMesh(K.mesh_smooth(self.vertices, offsets, neighbours, factors, weights), self.faces, self.normals,
                            self.colors)
        mesh._adjacency, mesh._vertex_faces, mesh._components = self._adjacency, self._vertex_faces, self._components
        return mesh

    def filter_smooth_laplacian(self, number_of_iterations: int = 1, lambda_filter: float = 0.5,
                                weights: str = "inverse_distance") -> "TriangleMesh":
        """number_of_iterations steps p' = p + lambda_filter * (weighted mean of the neighbours - p); it shrinks the mesh.
        Faces, colours and the OLD normals are kept (compute_vertex_normals refreshes them)."""
        return self._smoothed([float(lambda_filter)] * max(int(number_of_iterations), 0), weights)

    def filter_smooth_taubin(self, number_of_iterations: int = 1, lambda_filter: float = 0.5, mu: float = -0.53,
                             weights: str = "inverse_distance") -> "TriangleMesh":
        """number_of_iterations pairs of a lambda_filter step and a mu step (mu < -lambda_filter < 0): smooths without
        the shrinkage of the Laplacian filter.  Faces, colours and the OLD normals are kept."""
        return self._smoothed([float(lambda_filter), float(mu)] * max(int(number_of_iterations), 0), weights)

    def compute_vertex_normals(self) -> "TriangleMesh":
        """The mesh with area-weighted vertex normals of its faces ((0, 0, 0) for a vertex without a face of any area)."""
        offsets, rows = self.vertex_faces()
        mesh = TriangleMesh(self.vertices, self.faces, K.mesh_vertex_normals(self.vertices, self.faces, offsets, rows),
                            self.colors)
        mesh._adjacency, mesh._vertex_faces = self._adjacency, self._vertex_faces
        mesh._components, mesh._stats = self._components, self._stats
        return mesh

    def simplify_vertex_clustering(self, voxel_size: float) -> "TriangleMesh":
        """One vertex per occupied cell of a voxel_size grid whose origin is the minimum bound minus half a voxel: the
        mean of the cell's vertices (and of their colours); the faces re-indexed, without those that collapse and
        without later duplicates; the normals recomputed if the mesh had any.  The result's `vertex_cluster` int32 [V]
        maps this mesh's vertices to its own."""
        voxel_size = float(voxel_size)
        origin = [0.0, 0.0, 0.0]
        if self.n_vertices > 0:
            origin = [x - 0.5 * voxel_size for x in self.vertices.min(dim=0).values.double().tolist()]
        c = K.mesh_cluster(self.vertices, self.faces, voxel_size, origin)
        mean = lambda t: None if t is None else K.mesh_rows_mean(c["offsets"], c["members"], t.float())   # noqa: E731
        mesh = TriangleMesh(mean(self.vertices), c["new_faces"], None, mean(self.colors))
        if self.normals is not None:
            mesh = mesh.compute_vertex_normals()
        mesh.vertex_cluster = c["vertex_cluster"]
        return mesh

    def write(self, path) -> None:
        """Binary PLY through ply.write_triangle_mesh (missing normals / colours are written as zeros)."""
        from . import ply
        zeros = torch.zeros_like(self.vertices)
        ply.write_triangle_mesh(str(path), self.vertices.cpu().numpy(), self.faces.cpu().numpy(),
                                (zeros if self.normals is None else self.normals).cpu().numpy(),
                                (zeros if self.colors is None else self.colors).cpu().numpy())
