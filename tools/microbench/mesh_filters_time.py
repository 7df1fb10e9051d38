"""Time of the mesh-filter entry points (profiles/mesh_filters.md) on the marching-tetrahedra mesh of an analytic TSDF at the
exporter's default resolution 128: a ball of radius 0.55 with 32 fruit-sized balls of radius 0.09 around it, the signed
distance clipped to five voxels as the fusion would leave it.  Stages, through their _kernels wrappers (allocation of the
outputs and the entry points' host reads included): both kinds of vertex rows, ten Taubin pairs on prebuilt rows, vertex
normals on prebuilt rows, vertex clustering at two voxels with two row means — next to a float64 NumPy restatement of the same
stages on the host (the host_* functions below: the route of tests/mesh_filters_reference.py, every row summed in order "by
rank"), with which the device arrays are compared bit for bit before anything is timed.  Host clock around work that ends in a device synchronise; medians of 7 after a warm-up.
    python tools/microbench/mesh_filters_time.py"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

RESOLUTION = 128


def volume():
    """float32 node values [R,R,R] over [-1, 1]^3"""
    rng = np.random.default_rng(0)
    axis = -1.0 + np.arange(RESOLUTION) * (2.0 / RESOLUTION)
    grid = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1)
    d = np.linalg.norm(grid - np.array([0.013, -0.021, 0.017]), axis=-1) - 0.55
    directions = rng.standard_normal((32, 3))
    directions /= np.linalg.norm(directions, axis=1, keepdims=True)
    for centre in directions * rng.uniform(0.62, 0.85, (32, 1)):
        d = np.minimum(d, np.linalg.norm(grid - centre, axis=-1) - 0.09)
    return np.clip(d / (5.0 * 2.0 / RESOLUTION), -1.0, 1.0).astype(np.float32)


NEIGHBOURS, FACES = 0, 1


def host_rows(faces, V, kind):
    """-> (offsets int32 [V + 1], entries int32 [E]): distinct sorted (row << 32) | entry keys"""
    faces = faces.astype(np.int64)
    if kind == NEIGHBOURS:
        pairs = [(s, t) for s in range(3) for t in range(3) if s != t]
        a = np.concatenate([faces[:, s] for s, _ in pairs])
        b = np.concatenate([faces[:, t] for _, t in pairs])
        a, b = a[a != b], b[a != b]
    else:
        a, b = faces.reshape(-1), np.repeat(np.arange(faces.shape[0], dtype=np.int64), 3)
    keys = np.unique((a << 32) | b)
    offsets = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys >> 32, minlength=V), out=offsets[1:])
    return offsets.astype(np.int32), (keys & 0xffffffff).astype(np.int32)


def ranked(offsets):
    """for j = 0, 1, ...: (the rows that have a term j, where it is)"""
    offsets = offsets.astype(np.int64)
    length = np.diff(offsets)
    for j in range(int(length.max()) if length.size else 0):
        rows = np.flatnonzero(length > j)
        yield rows, offsets[rows] + j


def host_row_sums(offsets, terms):
    total = np.zeros((offsets.size - 1,) + terms.shape[1:])
    for rows, at in ranked(offsets):
        total[rows] = total[rows] + terms[at]
    return total


def host_smooth(vertices, offsets, neighbours, factors):
    """inverse-distance weights; float64 across the steps -> float32"""
    p = vertices.astype(np.float64)
    has_row = np.diff(offsets.astype(np.int64)) > 0
    for factor in factors:
        S, W = np.zeros_like(p), np.zeros(p.shape[0])
        for rows, at in ranked(offsets):
            pn = p[neighbours[at]]
            d = p[rows] - pn
            w = 1.0 / (np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + 1e-12)
            S[rows] = S[rows] + w[:, None] * pn
            W[rows] = W[rows] + w
        q = p.copy()
        q[has_row] = p[has_row] + factor * (S[has_row] / W[has_row][:, None] - p[has_row])
        p = q
    return p.astype(np.float32)


def host_normals(vertices, faces, offsets, face_rows):
    v = vertices.astype(np.float64)
    e1, e2 = v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]
    fn = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    n = host_row_sums(offsets, fn[face_rows])
    sq = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    out = np.zeros_like(n)
    out[sq > 0] = n[sq > 0] / np.sqrt(sq[sq > 0])[:, None]
    return out.astype(np.float32)


def host_cluster(vertices, faces, colors, voxel, origin):
    """-> clustered vertices, faces, colours"""
    V = vertices.shape[0]
    cell = np.floor((vertices.astype(np.float64) - origin) / voxel).astype(np.int64)
    _, raw = np.unique((cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2], return_inverse=True)
    raw = raw.reshape(-1)
    first = np.full(int(raw.max()) + 1, V, dtype=np.int64)
    np.minimum.at(first, raw, np.arange(V))
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    vc = rank[raw]
    members = np.argsort(vc, kind="stable")
    offsets = np.zeros(first.size + 1, dtype=np.int64)
    np.cumsum(np.bincount(vc, minlength=first.size), out=offsets[1:])
    nf = vc[faces.astype(np.int64)]
    ids = np.flatnonzero((nf[:, 0] != nf[:, 1]) & (nf[:, 1] != nf[:, 2]) & (nf[:, 0] != nf[:, 2]))
    s, i = np.argmin(nf[ids], axis=1), np.arange(ids.size)
    rotated = np.stack([nf[ids][i, (s + k) % 3] for k in range(3)], axis=1)
    keep = np.sort(ids[np.unique(rotated, axis=0, return_index=True)[1]])
    count = np.diff(offsets).astype(np.float64)[:, None]
    mean = lambda a: (host_row_sums(offsets, a.astype(np.float64)[members]) / count).astype(np.float32)     # noqa: E731
    return mean(vertices), nf[keep].astype(np.int32), mean(colors)


def timed(fn, n=7):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out)


def host(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def same(a, b):
    a = a.cpu().numpy()
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def main():
    from fruitnerf_amd import _kernels as K
    from fruitnerf_amd.export.tsdf import TSDF
    dev = torch.device("cuda:0")
    tsdf = TSDF.from_aabb(torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]), (RESOLUTION,) * 3, dev)
    tsdf.values.copy_(torch.as_tensor(volume()))
    tsdf.colors.copy_(torch.rand((RESOLUTION,) * 3 + (3,), generator=torch.Generator().manual_seed(1)))
    mesh = tsdf.get_triangle_mesh()
    V, F = mesh.n_vertices, mesh.n_faces
    voxel = 2.0 * 2.0 / RESOLUTION
    vertices, faces, colors = [t.cpu().numpy() for t in (mesh.vertices, mesh.faces, mesh.colors)]
    print(f"mesh: {V} vertices, {F} faces, {mesh.connected_components()[1]} components", flush=True)

    # the host restatement, one run per stage
    (nb, t_nb), (fc, t_fc) = host(lambda: host_rows(faces, V, NEIGHBOURS)), host(lambda: host_rows(faces, V, FACES))
    ref_smooth, t_smooth = host(lambda: host_smooth(vertices, *nb, [0.5, -0.53] * 10))
    ref_normals, t_normals = host(lambda: host_normals(vertices, faces, *fc))
    origin = vertices.min(axis=0).astype(np.float64) - 0.5 * voxel
    ref_cluster, t_cluster = host(lambda: host_cluster(vertices, faces, colors, voxel, origin))
    print(f"host: rows {t_nb:.1f} + {t_fc:.1f} ms, ten Taubin pairs {t_smooth:.1f} ms, normals {t_normals:.1f} ms, "
          f"clustering with means {t_cluster:.1f} ms; longest neighbour row {int(np.diff(nb[0]).max())}", flush=True)

    origin = origin.tolist()

    def cluster():
        c = K.mesh_cluster(mesh.vertices, mesh.faces, voxel, origin)
        return c, K.mesh_rows_mean(c["offsets"], c["members"], mesh.vertices), K.mesh_rows_mean(c["offsets"], c["members"],
                                                                                                 mesh.colors)

    d_nb, d_fc = mesh.vertex_adjacency(), mesh.vertex_faces()
    c, mean_v, mean_c = cluster()
    equal = [same(d_nb[0], nb[0]), same(d_nb[1], nb[1]), same(d_fc[0], fc[0]), same(d_fc[1], fc[1]),
             same(K.mesh_smooth(mesh.vertices, *d_nb, [0.5, -0.53] * 10), ref_smooth),
             same(K.mesh_vertex_normals(mesh.vertices, mesh.faces, *d_fc), ref_normals),
             same(mean_v, ref_cluster[0]), same(c["new_faces"], ref_cluster[1]), same(mean_c, ref_cluster[2])]
    print(f"device arrays equal the restatement bit for bit: {equal}; clustering at {voxel}: {mean_v.shape[0]} vertices, "
          f"{c['new_faces'].shape[0]} faces", flush=True)

    rows = {name: timed(lambda k=kind: K.mesh_vertex_rows(mesh.faces, V, k))
            for name, kind in (("neighbour rows", K.MESH_ROWS_NEIGHBOURS), ("face rows", K.MESH_ROWS_FACES))}
    rows["ten Taubin pairs"] = timed(lambda: K.mesh_smooth(mesh.vertices, *d_nb, [0.5, -0.53] * 10))
    rows["one Taubin pair"] = timed(lambda: K.mesh_smooth(mesh.vertices, *d_nb, [0.5, -0.53]))
    rows["vertex normals"] = timed(lambda: K.mesh_vertex_normals(mesh.vertices, mesh.faces, *d_fc))
    rows["clustering with two means"] = timed(cluster)
    for name, (median, least) in rows.items():
        print(f"  {name}: {median:.3f} ms (min {least:.3f})", flush=True)


if __name__ == "__main__":
    main()
