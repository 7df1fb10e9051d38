"""Float64 NumPy restatement of the mesh-filter contract of include/fruitnerf_hip.h ("triangle-mesh filters": per-vertex
rows, Laplacian / Taubin smoothing, area-weighted vertex normals, vertex clustering, row means).  It shares no code with the
product (csrc/mesh_filters.hip); every floating-point sum is the sequential sum of a row in ascending order, done "by rank"
so that it stays vectorised, and every operation is one rounded float64 operation: the device result is compared with these
arrays bit for bit.  test_mesh_filters_cpu.py checks the restatement itself."""
import numpy as np

from tests import mesh_components_reference as mr
from tests import tsdf_reference as tr

NEIGHBOURS, FACES = 0, 1
UNIFORM, INVERSE_DISTANCE = 0, 1
MAX_CELLS = 1 << 21


def _f64(a):
    return np.asarray(np.asarray(a, dtype=np.float32), dtype=np.float64).reshape(-1, 3)


# ---- rows ---------------------------------------------------------------------------------------------------------------
def _rows_of_pairs(row, entry, n_rows):
    keys = np.unique((row << 32) | entry)                     # sorted and distinct
    offsets = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys >> 32, minlength=n_rows), out=offsets[1:])
    return offsets.astype(np.int32), (keys & 0xffffffff).astype(np.int32)


def vertex_rows(faces, n_vertices, kind):
    """-> (offsets int32 [V + 1], entries int32 [E]).  NEIGHBOURS: row a = every b != a that shares a face with a, once,
    ascending.  FACES: row a = every face that lists a, once, ascending."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if kind == NEIGHBOURS:
        a = np.concatenate([faces[:, s] for s in range(3) for t in range(3) if s != t])
        b = np.concatenate([faces[:, t] for s in range(3) for t in range(3) if s != t])
        real = a != b
        return _rows_of_pairs(a[real], b[real], int(n_vertices))
    f = np.repeat(np.arange(faces.shape[0], dtype=np.int64), 3)
    return _rows_of_pairs(faces.reshape(-1), f, int(n_vertices))


def _ranked(offsets):
    """For j = 0, 1, ...: (rows that have a term j, the position of that term in the entries)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    length = np.diff(offsets)
    for j in range(int(length.max()) if length.size else 0):
        rows = np.flatnonzero(length > j)
        yield rows, offsets[rows] + j


def row_sums(offsets, terms):
    """The sequential float64 sum of every row's terms [E, ...] in entry order, starting from 0.0 -> [rows, ...]."""
    terms = np.asarray(terms, dtype=np.float64)
    total = np.zeros((len(offsets) - 1,) + terms.shape[1:], dtype=np.float64)
    for rows, at in _ranked(offsets):
        total[rows] = total[rows] + terms[at]
    return total


# ---- smoothing ----------------------------------------------------------------------------------------------------------
def smooth(vertices, offsets, neighbours, factors, weights=INVERSE_DISTANCE):
    """p' = p + factor * (S / W - p) per step, positions kept in float64 across the steps -> float32 [V,3]"""
    p = _f64(vertices).copy()
    offsets = np.asarray(offsets, dtype=np.int64)
    neighbours = np.asarray(neighbours, dtype=np.int64)
    has_row = np.diff(offsets) > 0
    for factor in factors:
        S = np.zeros_like(p)
        W = np.zeros(p.shape[0], dtype=np.float64)
        for rows, at in _ranked(offsets):
            pn = p[neighbours[at]]
            if weights == UNIFORM:
                w = np.ones(rows.size, dtype=np.float64)
            else:
                d = p[rows] - pn
                w = 1.0 / (np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + 1e-12)
            S[rows] = S[rows] + w[:, None] * pn
            W[rows] = W[rows] + w
        q = p.copy()
        q[has_row] = p[has_row] + np.float64(factor) * (S[has_row] / W[has_row][:, None] - p[has_row])
        p = q
    return p.astype(np.float32)


def laplacian(vertices, faces, iterations=1, lam=0.5, weights=INVERSE_DISTANCE):
    offsets, nb = vertex_rows(faces, np.asarray(vertices).reshape(-1, 3).shape[0], NEIGHBOURS)
    return smooth(vertices, offsets, nb, [lam] * iterations, weights)


def taubin(vertices, faces, iterations=1, lam=0.5, mu=-0.53, weights=INVERSE_DISTANCE):
    offsets, nb = vertex_rows(faces, np.asarray(vertices).reshape(-1, 3).shape[0], NEIGHBOURS)
    return smooth(vertices, offsets, nb, [lam, mu] * iterations, weights)


# ---- normals ------------------------------------------------------------------------------------------------------------
def vertex_normals(vertices, faces, offsets=None, face_rows=None):
    """Area-weighted: the float64 sum of (v1 - v0) x (v2 - v0) over the vertex's faces in ascending order, normalised,
    rounded to float32; a zero sum stays (0, 0, 0)."""
    v = _f64(vertices)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if offsets is None:
        offsets, face_rows = vertex_rows(faces, v.shape[0], FACES)
    e1, e2 = v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]
    fn = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).reshape(-1, 3)
    n = row_sums(offsets, fn[np.asarray(face_rows, dtype=np.int64)])
    sq = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    out = np.zeros_like(n)
    real = sq > 0
    out[real] = n[real] / np.sqrt(sq[real])[:, None]
    return out.astype(np.float32)


# ---- clustering ---------------------------------------------------------------------------------------------------------
def cluster_origin(vertices, voxel_size):
    v32 = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    if v32.shape[0] == 0:
        return np.zeros(3)
    return v32.min(axis=0).astype(np.float64) - 0.5 * float(voxel_size)


def rows_mean(offsets, members, values):
    """float64 sum of a row's values in member order / member count, rounded to float32; an empty row gives zeros"""
    values = _f64(values)
    total = row_sums(offsets, values[np.asarray(members, dtype=np.int64)])
    count = np.diff(np.asarray(offsets, dtype=np.int64)).astype(np.float64)
    out = np.zeros_like(total)
    real = count > 0
    out[real] = total[real] / count[real][:, None]
    return out.astype(np.float32)


def canonical(faces):
    """every triple rotated to start at its smallest index (the first such position)"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    s = np.argmin(faces, axis=1)
    i = np.arange(faces.shape[0])
    return np.stack([faces[i, (s + k) % 3] for k in range(3)], axis=1).reshape(-1, 3)


def cluster(vertices, faces, voxel_size, origin=None):
    """-> dict: vertex_cluster int32 [V]; offsets int32 [V' + 1] and members int32 [V] (ascending inside a cluster);
    new_faces int32 [F',3] and face_ids int32 [F']; n_degenerate, n_duplicates (what was dropped)."""
    v = _f64(vertices)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    voxel_size = float(voxel_size)
    if not voxel_size > 0 or not np.isfinite(voxel_size):
        raise ValueError("voxel_size must be positive")
    origin = cluster_origin(vertices, voxel_size) if origin is None else np.asarray(origin, dtype=np.float64)
    V = v.shape[0]
    cell = np.floor((v - origin) / voxel_size)
    if not np.isfinite(cell).all() or (cell < 0).any() or (cell >= MAX_CELLS).any():
        raise ValueError("a vertex lies outside the 2^21 cells of an axis")
    cell = cell.astype(np.int64)
    key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    _, raw = np.unique(key, return_inverse=True)
    raw = raw.reshape(-1)
    n = int(raw.max()) + 1 if V else 0
    first = np.full(n, V, dtype=np.int64)
    np.minimum.at(first, raw, np.arange(V))
    rank = np.empty(n, dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(n)
    vc = rank[raw] if V else np.zeros(0, dtype=np.int64)
    members = np.argsort(vc, kind="stable")
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(vc, minlength=n), out=offsets[1:])
    nf = vc[faces].reshape(-1, 3)
    real = (nf[:, 0] != nf[:, 1]) & (nf[:, 1] != nf[:, 2]) & (nf[:, 0] != nf[:, 2])
    ids = np.flatnonzero(real)
    if ids.size:
        _, firsts = np.unique(canonical(nf[ids]), axis=0, return_index=True)
        keep = np.sort(ids[firsts])
    else:
        keep = ids
    return {"vertex_cluster": vc.astype(np.int32), "offsets": offsets.astype(np.int32), "members": members.astype(np.int32),
            "new_faces": nf[keep].astype(np.int32).reshape(-1, 3), "face_ids": keep.astype(np.int32),
            "n_degenerate": int((~real).sum()), "n_duplicates": int(ids.size - keep.size)}


def simplify(vertices, faces, voxel_size, normals=None, colors=None):
    """simplify_vertex_clustering -> (vertices, faces, normals or None, colors or None, cluster dict): positions and
    colours are row means, normals are recomputed on the new mesh if there were any."""
    c = cluster(vertices, faces, voxel_size)
    nv = rows_mean(c["offsets"], c["members"], vertices)
    nc = None if colors is None else rows_mean(c["offsets"], c["members"], colors)
    nn = None if normals is None else vertex_normals(nv, c["new_faces"])
    return nv, c["new_faces"], nn, nc, c


# ---- test meshes --------------------------------------------------------------------------------------------------------
_SPHERES = {}


def spheres_mesh():
    """the three-sphere mesh of mesh_components_reference (1208 vertices, 2400 faces, 4 components), extracted once by
    the TSDF restatement: float32 vertices / normals / colours, int32 faces"""
    if not _SPHERES:
        values = mr.spheres_volume()
        colors = np.random.default_rng(2).uniform(0, 1, mr.SPHERES_DIMS + (3,)).astype(np.float32)
        m = tr.extract(values, colors, mr.SPHERES_LO, mr.SPHERES_HI)
        _SPHERES.update(vertices=m["vertices"].astype(np.float32), faces=m["faces"].astype(np.int32),
                        normals=m["normals"].astype(np.float32), colors=m["colors"].astype(np.float32))
        for a in _SPHERES.values():
            a.setflags(write=False)
    return _SPHERES


def with_unreferenced(vertices, faces, n=5, seed=21):
    """the mesh with n unreferenced vertices appended"""
    extra = np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32)
    return np.concatenate([np.asarray(vertices, dtype=np.float32), extra]), faces


def duplicate_case():
    """A face, its rotation, its reversal, and a face that collapses at voxel 1.0: vertices 0..3 sit in four different
    cells, vertex 4 shares vertex 3's cell.  -> vertices, faces, expected face_ids, expected new faces"""
    vertices = np.array([[0.2, 0.2, 0.2], [1.3, 0.2, 0.2], [0.2, 1.4, 0.2], [0.3, 0.3, 1.5], [0.6, 0.4, 1.6]],
                        dtype=np.float32)
    faces = np.array([[1, 2, 0], [2, 0, 1], [2, 1, 0], [0, 3, 4], [0, 1, 4], [4, 0, 1], [1, 0, 3]], dtype=np.int32)
    # face 1 rotates face 0 (dropped); face 2 reverses it (kept); face 3 collapses (3 and 4 merge); face 5 rotates face 4
    # once 4 -> 3; face 6 reverses it
    return vertices, faces, np.array([0, 2, 4, 6], dtype=np.int32), np.array([[1, 2, 0], [2, 1, 0], [0, 1, 3], [1, 0, 3]],
                                                                            dtype=np.int32)
