"""Float64 NumPy / SciPy restatement of the mesh-connectivity contract of include/fruitnerf_hip.h ("triangle-mesh
connectivity": components over shared edges, per-component statistics, order-preserving selection).  It shares no code with
the product; test_mesh_components_cpu.py pins it against a pure-Python flood fill.  Also the test meshes both suites use."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

EPS64 = 2.0 ** -52


# ---- connectivity -------------------------------------------------------------------------------------------------------
def edge_incidences(faces):
    """-> (keys int64 [E], face int64 [E]) of the incidences, sorted by key and, inside a key, by (face, slot); a slot
    with a == b has none."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a = faces.reshape(-1)
    b = faces[:, [1, 2, 0]].reshape(-1)
    face = np.repeat(np.arange(faces.shape[0], dtype=np.int64), 3)
    real = a != b
    a, b, face = a[real], b[real], face[real]
    keys = (np.minimum(a, b) << 32) | np.maximum(a, b)
    order = np.argsort(keys, kind="stable")
    return keys[order], face[order]


def _groups(keys):
    """start index of every run of equal keys, and the run of every entry"""
    if keys.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    new = np.concatenate([[True], keys[1:] != keys[:-1]])
    return np.flatnonzero(new), np.cumsum(new) - 1


def components(faces):
    """-> (face_component int32 [F], n_components): numbered by smallest face, component 0 holds face 0."""
    faces = np.asarray(faces).reshape(-1, 3)
    F = faces.shape[0]
    if F == 0:
        return np.zeros(0, dtype=np.int32), 0
    keys, face = edge_incidences(faces)
    starts, run = _groups(keys)
    first = face[starts][run] if keys.size else face
    graph = coo_matrix((np.ones(face.size, dtype=np.int8), (face, first)), shape=(F, F))
    n, raw = connected_components(graph, directed=False)
    # relabel by first face
    first_face = np.full(n, F, dtype=np.int64)
    np.minimum.at(first_face, raw, np.arange(F))
    rank = np.empty(n, dtype=np.int64)
    rank[np.argsort(first_face, kind="stable")] = np.arange(n)
    return rank[raw].astype(np.int32), int(n)


# ---- statistics ---------------------------------------------------------------------------------------------------------
def _cross(p, q, absolute):
    m = (lambda x, y: np.abs(x * y)) if absolute else (lambda x, y: x * y)
    s = 1.0 if absolute else -1.0
    return np.stack([m(p[:, 1], q[:, 2]) + s * m(p[:, 2], q[:, 1]),
                     m(p[:, 2], q[:, 0]) + s * m(p[:, 0], q[:, 2]),
                     m(p[:, 0], q[:, 1]) + s * m(p[:, 1], q[:, 0])], axis=1)


def face_terms(vertices, faces, absolute=False):
    """Per face, float64: area, signed volume term, moment [3].  absolute: every product replaced by its absolute
    value (and the differences inside the products' sums by sums) — what a term's rounding error is measured against."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    v0, v1, v2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    n = _cross(v1 - v0, v2 - v0, absolute)
    area = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) / 2.0
    c = _cross(v1, v2, absolute)
    a0 = np.abs(v0) if absolute else v0
    volume = ((a0[:, 0] * c[:, 0] + a0[:, 1] * c[:, 1]) + a0[:, 2] * c[:, 2]) / 6.0
    centre = ((np.abs(v0) + np.abs(v1)) + np.abs(v2)) / 3.0 if absolute else ((v0 + v1) + v2) / 3.0
    return area, volume, area[:, None] * centre


def stats(vertices, faces, labels, n_components):
    """dict of per-component arrays: n_faces, boundary_edges, nonmanifold_edges (int64); lo, hi (float32 [C,3]); area,
    volume (float64 [C]), moment (float64 [C,3]); and abs_area, abs_volume, abs_moment — the same sums over the
    absolute-value terms."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    labels = np.asarray(labels, dtype=np.int64)
    C = int(n_components)
    out = {"n_faces": np.bincount(labels, minlength=C).astype(np.int64)}
    keys, face = edge_incidences(faces)
    starts, run = _groups(keys)
    size = np.bincount(run, minlength=starts.size)
    owner = labels[face[starts]] if starts.size else np.zeros(0, dtype=np.int64)
    out["boundary_edges"] = np.bincount(owner[size == 1], minlength=C).astype(np.int64)
    out["nonmanifold_edges"] = np.bincount(owner[size >= 3], minlength=C).astype(np.int64)
    v32 = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    lo = np.full((C, 3), np.inf, dtype=np.float32)
    hi = np.full((C, 3), -np.inf, dtype=np.float32)
    for k in range(3):
        np.minimum.at(lo, labels, v32[faces[:, k]])
        np.maximum.at(hi, labels, v32[faces[:, k]])
    out["lo"], out["hi"] = lo, hi
    for prefix, absolute in (("", False), ("abs_", True)):
        area, volume, moment = face_terms(vertices, faces, absolute)
        out[prefix + "area"] = np.array([area[labels == c].sum() for c in range(C)], dtype=np.float64)
        out[prefix + "volume"] = np.array([volume[labels == c].sum() for c in range(C)], dtype=np.float64)
        out[prefix + "moment"] = np.array([moment[labels == c].sum(axis=0) for c in range(C)],
                                          dtype=np.float64).reshape(C, 3)
    return out


def sum_bound(n_faces, absolute_sum):
    """(n_c + 32) * 2^-52 * A_c: n_c - 1 additions in any order, each within half an ulp of the running absolute sum, on
    both sides of the comparison, plus a few roundings per term."""
    return (np.asarray(n_faces, dtype=np.float64).reshape((-1,) + (1,) * (np.ndim(absolute_sum) - 1)) + 32.0) * EPS64 \
        * np.asarray(absolute_sum)


# ---- selection ----------------------------------------------------------------------------------------------------------
def select(faces, n_vertices, face_keep):
    """-> new_faces int32 [F',3], vertex_ids int32 [V'] ascending, face_ids int32 [F'] ascending."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    face_ids = np.flatnonzero(np.asarray(face_keep) != 0)
    kept = faces[face_ids]
    used = np.zeros(int(n_vertices), dtype=bool)
    used[kept.reshape(-1)] = True
    vertex_ids = np.flatnonzero(used)
    new_index = np.cumsum(used) - 1
    return new_index[kept].astype(np.int32).reshape(-1, 3), vertex_ids.astype(np.int32), face_ids.astype(np.int32)


def vertex_mask_faces(faces, vertex_mask):
    """A face stays iff all three of its vertices pass."""
    return np.asarray(vertex_mask, dtype=bool)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)].all(axis=1)


def small_component_faces(faces, min_faces):
    """face mask of remove_small_components(min_faces)"""
    labels, n = components(faces)
    return (np.bincount(labels, minlength=n) >= min_faces)[labels] if n else np.zeros(0, dtype=bool)


def largest_component_faces(faces, k):
    """face mask of keep_largest_components(k): by face count, ties to the smaller component index"""
    labels, n = components(faces)
    if n == 0:
        return np.zeros(0, dtype=bool)
    order = np.argsort(-np.bincount(labels, minlength=n), kind="stable")[:max(k, 0)]
    keep = np.zeros(n, dtype=bool)
    keep[order] = True
    return keep[labels]


# ---- test meshes --------------------------------------------------------------------------------------------------------
_TET = ((0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2))             # the surface of a tetrahedron, outward for a right-handed one
_TET_VERTICES = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def hand_made():
    """name -> (vertices float32 [V,3], faces int32 [F,3], expected number of components)"""
    rng = np.random.default_rng(11)
    tet = np.array(_TET_VERTICES)
    meshes = {}
    # two tetrahedron surfaces sharing exactly one vertex (vertex 3 of the first is vertex 0 of the second)
    v = np.concatenate([tet, tet[1:] * 0.7 + tet[3]])
    second = np.array([3, 4, 5, 6])
    meshes["tets_sharing_a_vertex"] = (v, np.concatenate([np.array(_TET), second[np.array(_TET)]]), 2)
    # two tetrahedra sharing the edge {2, 3}
    v = np.concatenate([tet, [[-1.0, 0.3, 0.2], [-0.4, 1.1, 0.9]]])
    second = np.array([4, 5, 2, 3])
    meshes["tets_sharing_an_edge"] = (v, np.concatenate([np.array(_TET), second[np.array(_TET)]]), 1)
    # three triangles on the edge {0, 1}
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0.2], [0.5, 0.1, 1]], dtype=np.float64)
    meshes["three_on_one_edge"] = (v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]]), 1)
    # a face listed twice, beside an unrelated one
    v = rng.uniform(-1, 1, (6, 3))
    meshes["face_listed_twice"] = (v, np.array([[0, 1, 2], [3, 4, 5], [0, 1, 2]]), 2)
    # a face (a, a, b): its only edge {a, b} = {1, 2} ties it to the first face; (4, 4, 4) has no edge at all; the last two share only vertex 5
    v = rng.uniform(-1, 1, (7, 3))
    meshes["repeated_index"] = (v, np.array([[0, 1, 2], [1, 1, 2], [4, 4, 4], [1, 1, 5], [5, 6, 6]]), 4)
    # unreferenced vertices before, between and after the used ones
    v = rng.uniform(-1, 1, (12, 3))
    meshes["unreferenced_vertices"] = (v, np.array([[2, 3, 5], [5, 3, 7], [9, 10, 8]]), 2)
    return {k: (a.astype(np.float32), f.astype(np.int32), n) for k, (a, f, n) in meshes.items()}


def top_index_faces():
    """faces whose indices sit just below n_vertices = 2^31 - 1: a 32-bit key would confuse the edges {t-1, t-2} and
    {t-2, t-3} ...; three components: a pair over a shared edge, a single face, a pair over a shared edge"""
    n_vertices = 2 ** 31 - 1
    t = n_vertices - 1
    faces = np.array([[t, t - 1, t - 2], [0, 1, 2], [t - 1, t, t - 3], [t - 4, t - 5, 3], [3, t - 5, 4]], dtype=np.int64)
    return n_vertices, faces.astype(np.int32), 3


def strip(n_faces, cuts, seed):
    """A triangle strip of n_faces faces (face i = vertices i, i + 1, i + 2) with the faces in `cuts` deleted, the rest
    stored in a seeded random order with every index triple rotated.  -> vertices, faces, sorted piece sizes"""
    rng = np.random.default_rng(seed)
    i = np.arange(n_faces + 2)
    vertices = np.stack([0.01 * (i // 2), 0.01 * (i % 2) + 0.002 * rng.standard_normal(i.size),
                         0.003 * rng.standard_normal(i.size)], axis=1)
    f = np.arange(n_faces)
    faces = np.stack([f, f + 1, f + 2], axis=1)
    faces = np.delete(faces, list(cuts), axis=0)
    faces = faces[rng.permutation(faces.shape[0])]
    turn = rng.integers(0, 3, faces.shape[0])
    faces = np.stack([faces[np.arange(faces.shape[0]), (turn + k) % 3] for k in range(3)], axis=1)
    edges = [-1] + sorted(cuts) + [n_faces]
    pieces = sorted(b - a - 1 for a, b in zip(edges[:-1], edges[1:]))
    return vertices.astype(np.float32), faces.astype(np.int32), pieces


def triangles_and_fan(n_triangles=3001, fan=64, seed=5):
    """n_triangles mutually disjoint triangles with one open fan of `fan` faces in their middle"""
    rng = np.random.default_rng(seed)
    half = n_triangles // 2
    tri = np.arange(3 * n_triangles).reshape(-1, 3)
    centre = 3 * n_triangles
    rim = centre + 1 + np.arange(fan + 1)
    fan_faces = np.stack([np.full(fan, centre), rim[:-1], rim[1:]], axis=1)
    faces = np.concatenate([tri[:half], fan_faces, tri[half:]])
    vertices = rng.uniform(-1, 1, (centre + fan + 2, 3))
    return vertices.astype(np.float32), faces.astype(np.int32), n_triangles + 1


SPHERES_DIMS = (20, 18, 16)
SPHERES_LO, SPHERES_HI = (-1.0, -0.9, -0.8), (1.0, 0.9, 0.8)
SPHERES_CENTRES = ((-0.52, -0.41, -0.33), (0.47, 0.38, 0.29), (0.43, -0.44, -0.27))
SPHERES_RADII = (0.31, 0.27, 0.22)
SPHERES_SPECK = ((3, 14, 12), -0.37)
SPHERES_COUNTS = (1208, 2400)                   # vertices, faces
SPHERES_COMPONENT_FACES = (1080, 24, 524, 772)


def spheres_volume():
    """float32 node values [20,18,16]: three spheres, clip(min_i(|p - c_i| - r_i) / (5 voxel_x), -1, 1), and one inside
    node on its own (the speck)"""
    dims = np.array(SPHERES_DIMS)
    lo, hi = np.array(SPHERES_LO), np.array(SPHERES_HI)
    vs = (hi - lo) / dims
    grid = np.stack(np.meshgrid(*[lo[a] + np.arange(dims[a]) * vs[a] for a in range(3)], indexing="ij"), axis=-1)
    d = np.min([np.linalg.norm(grid - np.array(c), axis=-1) - r for c, r in zip(SPHERES_CENTRES, SPHERES_RADII)], axis=0)
    values = np.clip(d / (5.0 * vs[0]), -1.0, 1.0).astype(np.float32)
    values[SPHERES_SPECK[0]] = SPHERES_SPECK[1]
    return values
