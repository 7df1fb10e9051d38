"""Binary PLY sink for the exported point sets — the file layout Open3D's `o3d.io.write_point_cloud` produces for a
PointCloud with points + colors (what /root/reference/fruit_nerf/scripts/exporter.py:116-119 calls on the three
sets of `sample_volume`), so the reference's clustering stage (clustering/*.py: `o3d.io.read_point_cloud`) can read
our exports unchanged.  open3d is not installed here: vertex = double x, y, z + uchar red, green, blue,
little-endian, colours quantised as round(clamp(c, 0, 1) * 255).  A cloud with normals (Nerfstudio's `pointcloud`
export after estimate_normals) gains double nx, ny, nz between position and colour, as Open3D writes it.
write_triangle_mesh / read_triangle_mesh: the TSDF export's mesh (export/tsdf.py), a layout of its own."""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import numpy as np

_VERTEX = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_VERTEX_NORMALS = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("nx", "<f8"), ("ny", "<f8"), ("nz", "<f8"),
                            ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def write_point_cloud(path: str, points: np.ndarray, colors: np.ndarray, normals: Optional[np.ndarray] = None) -> None:
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    colors = np.asarray(colors, dtype=np.float64).reshape(-1, 3)
    if points.shape[0] != colors.shape[0]:
        raise ValueError(f"{points.shape[0]} points but {colors.shape[0]} colours")
    v = np.empty(points.shape[0], dtype=_VERTEX if normals is None else _VERTEX_NORMALS)
    v["x"], v["y"], v["z"] = points[:, 0], points[:, 1], points[:, 2]
    if normals is not None:
        normals = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
        if normals.shape[0] != points.shape[0]:
            raise ValueError(f"{points.shape[0]} points but {normals.shape[0]} normals")
        v["nx"], v["ny"], v["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    q = np.rint(np.clip(colors, 0.0, 1.0) * 255.0).astype(np.uint8)
    v["red"], v["green"], v["blue"] = q[:, 0], q[:, 1], q[:, 2]
    header = ("ply\nformat binary_little_endian 1.0\ncomment Created by Open3D\n"
              f"element vertex {points.shape[0]}\n"
              "property double x\nproperty double y\nproperty double z\n"
              + ("" if normals is None else "property double nx\nproperty double ny\nproperty double nz\n") +
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())


def read_point_cloud(path: str):
    """Reader for files written by write_point_cloud (tests, count checks): points float64 [n,3], colours in [0,1];
    a file with normals returns (points, colours, normals float64 [n,3])."""
    with open(path, "rb") as f:
        n = None
        has_normals = False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            line = line.decode("ascii").strip()
            if line.startswith("format") and "binary_little_endian" not in line:
                raise ValueError(f"{path}: only binary_little_endian PLY is supported")
            if line.startswith("element vertex"):
                n = int(line.split()[-1])
            if line == "property double nx":
                has_normals = True
            if line == "end_header":
                break
        dtype = _VERTEX_NORMALS if has_normals else _VERTEX
        v = np.frombuffer(f.read(n * dtype.itemsize), dtype=dtype, count=n)
    pts = np.stack([v["x"], v["y"], v["z"]], axis=1)
    cols = np.stack([v["red"], v["green"], v["blue"]], axis=1).astype(np.float64) / 255.0
    if has_normals:
        return pts, cols, np.stack([v["nx"], v["ny"], v["nz"]], axis=1)
    return pts, cols


_MESH_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                         ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_MESH_FACE = np.dtype([("count", "u1"), ("vertex_indices", "<u4", (3,))])
_MESH_PROPERTIES = ("property float x\nproperty float y\nproperty float z\n"
                    "property float nx\nproperty float ny\nproperty float nz\n"
                    "property uchar red\nproperty uchar green\nproperty uchar blue\n")


def write_triangle_mesh(path: str, vertices: np.ndarray, faces: np.ndarray, normals: np.ndarray,
                        colors: np.ndarray) -> None:
    """The TSDF export's mesh (export/tsdf.py) as a binary little-endian PLY: float x, y, z, nx, ny, nz and uchar red,
    green, blue per vertex (colours quantised as round(clamp(c, 0, 1) * 255)), then `list uchar uint vertex_indices`
    triangles.  An empty mesh is a valid file with two empty elements."""
    vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    colors = np.asarray(colors, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    n = vertices.shape[0]
    if normals.shape[0] != n or colors.shape[0] != n:
        raise ValueError(f"{n} vertices but {normals.shape[0]} normals and {colors.shape[0]} colours")
    if faces.size and (int(faces.min()) < 0 or int(faces.max()) >= n):
        raise ValueError(f"face indices outside 0..{n - 1}")
    v = np.empty(n, dtype=_MESH_VERTEX)
    v["x"], v["y"], v["z"] = vertices[:, 0], vertices[:, 1], vertices[:, 2]
    v["nx"], v["ny"], v["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    q = np.rint(np.clip(colors, 0.0, 1.0) * 255.0).astype(np.uint8)
    v["red"], v["green"], v["blue"] = q[:, 0], q[:, 1], q[:, 2]
    f = np.empty(faces.shape[0], dtype=_MESH_FACE)
    f["count"] = 3
    f["vertex_indices"] = faces
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\n" + _MESH_PROPERTIES +
              f"element face {faces.shape[0]}\nproperty list uchar uint vertex_indices\nend_header\n")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(f.tobytes())


def read_triangle_mesh(path: str):
    """Reader for files written by write_triangle_mesh -> vertices float32 [V,3], faces int32 [F,3], normals float32
    [V,3], colours float64 [V,3] in [0,1] (the order TSDF.get_mesh returns)."""
    with open(path, "rb") as fh:
        header = []
        while True:
            line = fh.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            header.append(line.decode("ascii").strip())
            if header[-1] == "end_header":
                break
        elements = [ln.split() for ln in header if ln.startswith("element")]
        if header[:2] != ["ply", "format binary_little_endian 1.0"] or [e[1] for e in elements] != ["vertex", "face"] \
                or "\n".join(ln for ln in header if ln.startswith("property")) + "\n" != \
                _MESH_PROPERTIES + "property list uchar uint vertex_indices\n":
            raise ValueError(f"{path}: not a triangle mesh written by write_triangle_mesh")
        n, m = int(elements[0][2]), int(elements[1][2])
        body = fh.read()
    if len(body) != n * _MESH_VERTEX.itemsize + m * _MESH_FACE.itemsize:
        raise ValueError(f"{path}: {len(body)} bytes of data for {n} vertices and {m} faces")
    v = np.frombuffer(body, dtype=_MESH_VERTEX, count=n)
    f = np.frombuffer(body, dtype=_MESH_FACE, count=m, offset=n * _MESH_VERTEX.itemsize)
    if m and not bool((f["count"] == 3).all()):
        raise ValueError(f"{path}: a face that is not a triangle")
    vertices = np.stack([v["x"], v["y"], v["z"]], axis=1)
    normals = np.stack([v["nx"], v["ny"], v["nz"]], axis=1)
    colors = np.stack([v["red"], v["green"], v["blue"]], axis=1).astype(np.float64) / 255.0
    return vertices, f["vertex_indices"].astype(np.int32), normals, colors


def write_point_clouds(pcd_list: Dict[str, dict]) -> Dict[str, int]:
    """The export script's final loop (scripts/exporter.py:116-119) over sample_volume()'s result: every set that has
    a path is written; returns the point count per set."""
    counts = {}
    for name, entry in pcd_list.items():
        counts[name] = int(entry["points"].shape[0])
        if entry.get("path"):
            write_point_cloud(entry["path"], entry["points"], entry["colors"])
    return counts
