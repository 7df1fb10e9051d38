"""Float64 NumPy restatement of the TSDF mesh export's contract (include/fruitnerf_hip.h: fnr_tsdf_volume, fnr_tsdf_integrate,
fnr_tsdf_mesh_count / _emit) and the fixtures its tests share.  It shares no code with the product (csrc/tsdf.hip,
fruitnerf_amd/export/tsdf.py): same split of a cell into six tetrahedra, same tie rules, written again.

Inputs are the float32 numbers the device sees, promoted; every operation then runs in float64."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
TIE_PIXELS = 1e-4        # a node-camera pair this close to a rounding tie of its pixel may be left out of a comparison
EDGE_DISTANCE = 1e-5     # ... or this close to one of the validity edges (z > 0, dist > -truncation)


def _f64(a):
    return np.asarray(np.asarray(a, dtype=np.float32), dtype=np.float64)


# ---- volume ------------------------------------------------------------------------------------------------------------
def voxel_size(lo, hi, dims):
    return (_f64(hi) - _f64(lo)) / np.asarray(dims, dtype=np.float64)


def node_positions(lo, hi, dims):
    """[nx,ny,nz,3]: node (i,j,k) at lo + (i,j,k) * voxel_size."""
    vs = voxel_size(lo, hi, dims)
    idx = np.stack(np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij"), axis=-1)
    return _f64(lo) + idx * vs


def empty_volume(dims):
    dims = tuple(int(d) for d in dims)
    return np.full(dims, -1.0), np.zeros(dims), np.zeros(dims + (3,))


def integrate(volume, lo, hi, c2w, intrinsics, depth, rgb, mask=None, depth_kind=1, truncation_margin=5.0,
              max_weight=1.0):
    """volume = (values, weights, colors), updated copies of which are returned with `near` [nx,ny,nz] bool: nodes with a
    camera closer than TIE_PIXELS to a pixel rounding tie or closer than EDGE_DISTANCE to a validity edge."""
    values, weights, colors = [np.array(a, dtype=np.float64) for a in volume]
    dims = values.shape
    P = node_positions(lo, hi, dims)
    truncation = truncation_margin * voxel_size(lo, hi, dims)[0]
    near = np.zeros(dims, dtype=bool)
    c2w, intrinsics, depth, rgb = _f64(c2w), _f64(intrinsics), _f64(depth), _f64(rgb)
    H, W = depth.shape[1:3]
    for c in range(c2w.shape[0]):
        R, t = c2w[c, :, :3], c2w[c, :, 3]
        fx, fy, cx, cy = intrinsics[c]
        q = (P - t) @ R                                     # R^T (p - t)
        z = -q[..., 2]
        front = z > 0
        zs = np.where(front, z, 1.0)
        a = fx * q[..., 0] / zs + cx - 0.5
        b = fy * (-q[..., 1]) / zs + cy - 0.5
        col, row = np.rint(a), np.rint(b)                   # ties to even
        tie = (np.abs(np.abs(a - np.floor(a)) - 0.5) < TIE_PIXELS) | (np.abs(np.abs(b - np.floor(b)) - 0.5) < TIE_PIXELS)
        inside = front & (col >= 0) & (col < W) & (row >= 0) & (row < H)
        ci = np.where(inside, col, 0).astype(np.int64)
        ri = np.where(inside, row, 0).astype(np.int64)
        sampled = np.where(inside, depth[c][ri, ci], 0.0)
        if mask is not None:
            sampled = np.where(np.asarray(mask[c])[ri, ci] != 0, sampled, 0.0)
        voxel_depth = z if depth_kind == 0 else np.linalg.norm(q, axis=-1)
        dist = sampled - voxel_depth
        valid = front & (sampled > 0) & (dist > -truncation)
        near |= (front & tie) | (np.abs(z) < EDGE_DISTANCE) | (front & (sampled > 0) &
                                                               (np.abs(dist + truncation) < EDGE_DISTANCE))
        s = np.clip(dist / truncation, -1.0, 1.0)
        w = weights
        values = np.where(valid, (values * w + s) / (w + 1.0), values)
        colors = np.where(valid[..., None], (colors * w[..., None] + rgb[c][ri, ci]) / (w[..., None] + 1.0), colors)
        weights = np.where(valid, np.minimum(w + 1.0, max_weight), w)
    return (values, weights, colors), near


def fusion_bound(lo, hi, dims, c2w, truncation_margin=5.0):
    """16 eps32 max|coordinate| / truncation: the float32 rounding of q, |q| and the division by the truncation (the
    running average does not amplify it)."""
    coordinate = max(float(np.abs(node_positions(lo, hi, dims)).max()), float(np.abs(_f64(c2w)[:, :, 3]).max()))
    return 16.0 * EPS32 * coordinate / (truncation_margin * voxel_size(lo, hi, dims)[0])


# ---- marching tetrahedra ----------------------------------------------------------------------------------------------
AXIS_ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def _corner_offset(corner):
    return np.array([corner & 1, (corner >> 1) & 1, (corner >> 2) & 1])


def tet_corners(t):
    """Corner ids (dx + 2 dy + 4 dz) on tetrahedron t's walk from corner 0 to corner 7."""
    a0, a1, _ = AXIS_ORDERS[t]
    return (0, 1 << a0, (1 << a0) | (1 << a1), 7)


def tet_triangles(t, case):
    """Triangles of tetrahedron t for `case` (bit p: the p-th corner of the walk is inside): a list of triples of
    (corner, corner) edges, wound so that the normal points from the inside corners to the outside ones."""
    corners = tet_corners(t)
    ins = [p for p in range(4) if (case >> p) & 1]
    outs = [p for p in range(4) if not (case >> p) & 1]
    if len(ins) == 1:
        tris = [[(ins[0], o) for o in outs]]
    elif len(ins) == 3:
        tris = [[(outs[0], i) for i in ins]]
    elif len(ins) == 2:
        quad = [(ins[0], outs[0]), (ins[0], outs[1]), (ins[1], outs[1]), (ins[1], outs[0])]
        tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    else:
        return []
    pos = [_corner_offset(c).astype(np.float64) for c in corners]
    towards = np.mean([pos[p] for p in outs], axis=0) - np.mean([pos[p] for p in ins], axis=0)
    result = []
    for tri in tris:
        m = [0.5 * (pos[a] + pos[b]) for a, b in tri]
        if np.dot(np.cross(m[1] - m[0], m[2] - m[0]), towards) < 0:
            tri = [tri[0], tri[2], tri[1]]
        result.append([(corners[a], corners[b]) for a, b in tri])
    return result


def gradient(values, vs):
    """Central differences of values in world units, one-sided at the border: [nx,ny,nz,3]."""
    g = np.zeros(values.shape + (3,))
    for a in range(3):
        v = np.moveaxis(values, a, 0)
        d = np.empty_like(v)
        d[1:-1] = (v[2:] - v[:-2]) / (2.0 * vs[a])
        d[0] = (v[1] - v[0]) / vs[a]
        d[-1] = (v[-1] - v[-2]) / vs[a]
        g[..., a] = np.moveaxis(d, 0, a)
    return g


def extract(values, colors, lo, hi):
    """-> dict: keys [V] int64 ascending (8 * index(a) + m), vertices / normals / colors [V,3], faces [F,3] (indices into
    keys, in the order cell, tetrahedron, triangle), face_keys [F,3], cases: the set of (tetrahedron case) seen."""
    values = _f64(values)
    colors = _f64(colors)
    dims = values.shape
    nx, ny, nz = dims
    vs = voxel_size(lo, hi, dims)
    P = node_positions(lo, hi, dims)
    G = gradient(values, vs)
    inside = values < 0
    index = lambda i, j, k: (i * ny + j) * nz + k      # noqa: E731
    verts = {}
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                for m in range(1, 8):
                    b = (i + (m & 1), j + ((m >> 1) & 1), k + (m >> 2))
                    if b[0] >= nx or b[1] >= ny or b[2] >= nz or inside[i, j, k] == inside[b]:
                        continue
                    va, vb = values[i, j, k], values[b]
                    t = (0.0 - va) / (vb - va)
                    n = G[i, j, k] + t * (G[b] - G[i, j, k])
                    length = np.linalg.norm(n)
                    verts[8 * index(i, j, k) + m] = (
                        P[i, j, k] + t * (P[b] - P[i, j, k]),
                        n / length if length > 0 else np.zeros(3),
                        colors[i, j, k] if abs(va) <= abs(vb) else colors[b])
    keys = np.array(sorted(verts), dtype=np.int64)
    rank = {int(k): r for r, k in enumerate(keys)}
    face_keys, cases = [], set()
    for i in range(nx - 1):
        for j in range(ny - 1):
            for k in range(nz - 1):
                for t in range(6):
                    case = 0
                    for p, corner in enumerate(tet_corners(t)):
                        o = _corner_offset(corner)
                        case |= int(inside[i + o[0], j + o[1], k + o[2]]) << p
                    cases.add(case)
                    for tri in tet_triangles(t, case):
                        row = []
                        for ca, cb in tri:
                            lower, m = min(ca, cb), ca ^ cb
                            o = _corner_offset(lower)
                            row.append(8 * index(i + o[0], j + o[1], k + o[2]) + m)
                        face_keys.append(row)
    face_keys = np.array(face_keys, dtype=np.int64).reshape(-1, 3)
    faces = np.array([[rank[int(k)] for k in row] for row in face_keys], dtype=np.int64).reshape(-1, 3)
    pick = lambda c: np.array([verts[int(k)][c] for k in keys], dtype=np.float64).reshape(-1, 3)   # noqa: E731
    return {"keys": keys, "vertices": pick(0), "normals": pick(1), "colors": pick(2), "faces": faces,
            "face_keys": face_keys, "cases": cases}


_FACE_TABLE = None


def _face_table():
    """tet_triangles as arrays: ntri [6,16], and per (tetrahedron, case, triangle, edge) the lower corner id and the
    direction code m of the edge, [6,16,2,3] each."""
    global _FACE_TABLE
    if _FACE_TABLE is None:
        ntri = np.zeros((6, 16), dtype=np.int64)
        lower = np.zeros((6, 16, 2, 3), dtype=np.int64)
        code = np.zeros((6, 16, 2, 3), dtype=np.int64)
        for t in range(6):
            for case in range(16):
                tris = tet_triangles(t, case)
                ntri[t, case] = len(tris)
                for q, tri in enumerate(tris):
                    for e, (ca, cb) in enumerate(tri):
                        lower[t, case, q, e], code[t, case, q, e] = min(ca, cb), ca ^ cb
        _FACE_TABLE = (ntri, lower, code)
    return _FACE_TABLE


def _shifted(dims, m):
    """Slices of the lower and the upper endpoint of every edge with direction code m."""
    d = (m & 1, (m >> 1) & 1, m >> 2)
    return (tuple(slice(0, n - s) for n, s in zip(dims, d)), tuple(slice(s, n) for n, s in zip(dims, d)))


def active_edges(values):
    """Node indices (a, b) and direction code m of every active edge, ascending by key 8 a + m: three int64 arrays."""
    values = _f64(values)
    dims = values.shape
    inside = values < 0
    index = np.arange(values.size, dtype=np.int64).reshape(dims)
    a, b, code = [], [], []
    for m in range(1, 8):
        sa, sb = _shifted(dims, m)
        act = inside[sa] != inside[sb]
        a.append(index[sa][act])
        b.append(index[sb][act])
        code.append(np.full(a[-1].shape, m, dtype=np.int64))
    a, b, code = np.concatenate(a), np.concatenate(b), np.concatenate(code)
    order = np.argsort(8 * a + code, kind="stable")
    return a[order], b[order], code[order]


def extract_fast(values, colors, lo, hi):
    """extract() in array operations, for volumes its loops cannot walk: the same dict (test_tsdf_cpu.py holds the two
    equal on every small fixture).  Vertices per direction code from two shifted views of the volume; faces per
    (tetrahedron, triangle slot) from a table built out of tet_triangles; ranks by searchsorted."""
    values = _f64(values)
    colors = _f64(colors).reshape(-1, 3)
    dims = values.shape
    nx, ny, nz = dims
    vs = voxel_size(lo, hi, dims)
    P = node_positions(lo, hi, dims).reshape(-1, 3)
    G = gradient(values, vs).reshape(-1, 3)
    flat = values.reshape(-1)
    a, b, code = active_edges(values)
    va, vb = flat[a], flat[b]
    t = (0.0 - va) / (vb - va)
    n = G[a] + t[:, None] * (G[b] - G[a])
    length = np.sqrt((n * n).sum(1))
    normals = np.where(length[:, None] > 0, n / np.where(length > 0, length, 1.0)[:, None], 0.0)
    keys = 8 * a + code
    vertices = P[a] + t[:, None] * (P[b] - P[a])
    vcolors = np.where((np.abs(va) <= np.abs(vb))[:, None], colors[a], colors[b])
    # faces
    ntri, lower, mcode = _face_table()
    inside = values < 0
    cell = np.arange(values.size, dtype=np.int64).reshape(dims)[:-1, :-1, :-1].reshape(-1)
    corner = lambda c: inside[(c & 1):nx - 1 + (c & 1), ((c >> 1) & 1):ny - 1 + ((c >> 1) & 1),       # noqa: E731
                              (c >> 2):nz - 1 + (c >> 2)].reshape(-1).astype(np.int64)
    step = lambda c: ((c & 1) * ny + ((c >> 1) & 1)) * nz + (c >> 2)                                   # noqa: E731
    rows, order_key, cases = [], [], set()
    for tet in range(6):
        case = sum(corner(c) << p for p, c in enumerate(tet_corners(tet)))
        cases.update(np.unique(case).tolist())
        for q in range(2):
            sel = ntri[tet][case] > q
            cs, base = case[sel], cell[sel]
            rows.append(np.stack([8 * (base + step(lower[tet, cs, q, e])) + mcode[tet, cs, q, e] for e in range(3)], axis=1))
            order_key.append(base * 12 + tet * 2 + q)
    face_keys = np.concatenate(rows).reshape(-1, 3)[np.argsort(np.concatenate(order_key), kind="stable")]
    faces = np.searchsorted(keys, face_keys)
    assert bool((keys[np.minimum(faces, keys.size - 1)] == face_keys).all()), "a face uses an edge that is not active"
    return {"keys": keys, "vertices": vertices, "normals": normals, "colors": vcolors, "faces": faces.astype(np.int64),
            "face_keys": face_keys, "cases": cases}


def normal_terms(values, lo, hi):
    """Per active edge, ascending by key: t, the unnormalised normal n = g_a + t (g_b - g_a) [V,3], and S [V,3], the
    sum per axis of the absolute values of the terms that enter n: (|v_hi| + |v_lo|) / span at a plus the same at b
    (t lies in [0, 1], and the rounding of t multiplies g_b - g_a, so both endpoints count in full)."""
    values = _f64(values)
    vs = voxel_size(lo, hi, values.shape)
    G = gradient(values, vs).reshape(-1, 3)
    A = np.zeros(values.shape + (3,))
    for ax in range(3):
        v = np.abs(np.moveaxis(values, ax, 0))
        d = np.empty_like(v)
        d[1:-1] = (v[2:] + v[:-2]) / (2.0 * vs[ax])
        d[0] = (v[1] + v[0]) / vs[ax]
        d[-1] = (v[-1] + v[-2]) / vs[ax]
        A[..., ax] = np.moveaxis(d, 0, ax)
    A = A.reshape(-1, 3)
    a, b, _ = active_edges(values)
    flat = values.reshape(-1)
    t = (0.0 - flat[a]) / (flat[b] - flat[a])
    return t, G[a] + t[:, None] * (G[b] - G[a]), A[a] + A[b]


def normal_condition(values, lo, hi):
    """cond = |S| / |n| per vertex (inf where n is the zero vector): how far an error of one unit relative to the terms
    of n turns the normalised normal."""
    _, n, S = normal_terms(values, lo, hi)
    length = np.sqrt((n * n).sum(1))
    return np.sqrt((S * S).sum(1)) / np.where(length > 0, length, 1.0) * np.where(length > 0, 1.0, np.inf)


def normals_float32(values, lo, hi):
    """The normal's formulas evaluated in float32 NumPy, one rounded operation at a time: the yardstick a float32 kernel
    is held to.  [V,3] float32, ascending by key."""
    f = np.float32
    values = np.asarray(values, dtype=f)
    dims = values.shape
    vs = (np.asarray(hi, dtype=f) - np.asarray(lo, dtype=f)) / np.asarray(dims, dtype=f)
    G = np.zeros(dims + (3,), dtype=f)
    for ax in range(3):
        v = np.moveaxis(values, ax, 0)
        d = np.empty_like(v)
        d[1:-1] = (v[2:] - v[:-2]) / (f(2.0) * vs[ax])
        d[0] = (v[1] - v[0]) / (f(1.0) * vs[ax])
        d[-1] = (v[-1] - v[-2]) / (f(1.0) * vs[ax])
        G[..., ax] = np.moveaxis(d, 0, ax)
    G = G.reshape(-1, 3)
    a, b, _ = active_edges(values)
    flat = values.reshape(-1)
    t = (f(0.0) - flat[a]) / (flat[b] - flat[a])
    n = G[a] + t[:, None] * (G[b] - G[a])
    length = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    assert n.dtype == f and length.dtype == f
    return np.where(length[:, None] > 0, n / np.where(length > 0, length, f(1.0))[:, None], f(0.0))


def normal_ratio(normals, reference_normals, cond):
    """Worst |normals - reference| / (eps32 cond) over the vertices with a finite cond (a non-zero reference normal)."""
    keep = np.isfinite(cond)
    err = np.sqrt(((np.asarray(normals, dtype=np.float64) - reference_normals) ** 2).sum(1))
    return float((err[keep] / (EPS32 * cond[keep])).max()) if keep.any() else 0.0


def block_of_key(keys, block=256):
    """The 256-node block that owns each edge key (the unit of the device's scan)."""
    return (np.asarray(keys, dtype=np.int64) // 8) // block


def oriented_faces(face_keys):
    """A face as an unordered triple with orientation: its rotation that starts at the smallest entry."""
    out = set()
    for row in np.asarray(face_keys).tolist():
        s = row.index(min(row))
        out.add((row[s], row[(s + 1) % 3], row[(s + 2) % 3]))
    return out


# ---- mesh properties ---------------------------------------------------------------------------------------------------
def mesh_report(vertices, faces):
    """Topology and volume of a triangle mesh: `closed_oriented` — every undirected edge lies in exactly two faces, once
    in each direction; `euler` = V - E + F; `degenerate` — faces that repeat an index; `volume` — the signed volume
    (positive when the faces' normals point outwards)."""
    vertices = np.asarray(vertices, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64)
    directed = {}
    for f in faces.tolist():
        for e in range(3):
            d = (f[e], f[(e + 1) % 3])
            directed[d] = directed.get(d, 0) + 1
    closed = all(n == 1 and directed.get((b, a), 0) == 1 for (a, b), n in directed.items())
    edges = {(min(a, b), max(a, b)) for a, b in directed}
    degenerate = int(sum(len(set(f)) < 3 for f in faces.tolist()))
    v0, v1, v2 = (vertices[faces[:, c]] for c in range(3))
    volume = float(np.einsum("ij,ij->i", v0, np.cross(v1, v2)).sum() / 6.0)
    return {"closed_oriented": closed, "euler": vertices.shape[0] - len(edges) + faces.shape[0],
            "degenerate": degenerate, "volume": volume, "used_vertices": int(np.unique(faces).size)}


# ---- fixtures ------------------------------------------------------------------------------------------------------------
SPHERE_DIMS = (17, 15, 13)
SPHERE_LO, SPHERE_HI = (-1.0, -0.9, -0.8), (1.0, 0.9, 0.8)
SPHERE_CENTER, SPHERE_RADIUS = (-0.043, 0.021, -0.037), 0.52


def sphere_volume():
    """The analytic sphere TSDF clamp((|p - c| - r) / truncation, -1, 1) as float32 values, with smooth float32 colours.
    c and r are off the lattice: no node value is 0, and the surface stays more than a cell clear of the border."""
    P = node_positions(SPHERE_LO, SPHERE_HI, SPHERE_DIMS)
    truncation = 5.0 * voxel_size(SPHERE_LO, SPHERE_HI, SPHERE_DIMS)[0]
    values = np.clip((np.linalg.norm(P - np.array(SPHERE_CENTER), axis=-1) - SPHERE_RADIUS) / truncation, -1.0, 1.0)
    colors = 0.5 + 0.5 * np.sin(P * np.array([3.0, 4.0, 5.0]) + np.array([0.1, 0.7, 1.3]))
    return values.astype(np.float32), colors.astype(np.float32)


def sphere_delta():
    """Sagitta of the longest cell diagonal as a chord of the sphere: how far a chord's interior lies from the surface."""
    chord = float(np.linalg.norm(voxel_size(SPHERE_LO, SPHERE_HI, SPHERE_DIMS)))
    return SPHERE_RADIUS - np.sqrt(SPHERE_RADIUS ** 2 - (0.5 * chord) ** 2)


FIELD_DIMS = (9, 8, 7)
FIELD_LO, FIELD_HI = (-0.9, -0.8, -0.7), (0.9, 0.8, 0.7)


def smooth_field(seed=7):
    """A few seeded sinusoids on 9 x 8 x 7 whose sign patterns reach all 16 tetrahedron cases; float32 values in (-1, 1)
    and float32 colours."""
    rng = np.random.default_rng(seed)
    P = node_positions(FIELD_LO, FIELD_HI, FIELD_DIMS)
    values = np.zeros(FIELD_DIMS)
    for _ in range(4):
        values += rng.uniform(0.3, 1.0) * np.sin(P @ rng.uniform(-6.0, 6.0, 3) + rng.uniform(0, 2 * np.pi))
    values = np.clip(values / 2.5, -0.999, 0.999)
    colors = rng.uniform(0.0, 1.0, FIELD_DIMS + (3,))
    return values.astype(np.float32), colors.astype(np.float32)


SCAN_LO, SCAN_HI = SPHERE_LO, SPHERE_HI
SCAN_BLOCKS_PER_TRIP = 1024             # the device scans the per-block counts 1024 blocks at a time
# dims -> (blocks of 256 nodes, trips of the block scan): one trip exactly full; a second trip of one block whose last
# block holds 251 nodes; three trips with a ragged last trip and block; the exporter's default, eight full trips
SCAN_DIMS = {(64, 64, 64): (1024, 1), (45, 343, 17): (1025, 2), (81, 81, 81): (2076, 3), (128, 128, 128): (8192, 8)}


def scan_volume(dims, seed=7):
    """smooth_field's four seeded waves on `dims` nodes over the box SCAN_LO..SCAN_HI, with smooth seeded colours that
    differ from node to node and from channel to channel; float32, as the device gets them."""
    rng = np.random.default_rng(seed)
    P = node_positions(SCAN_LO, SCAN_HI, dims)
    values = np.zeros(tuple(dims))
    for _ in range(4):
        values += rng.uniform(0.3, 1.0) * np.sin(P @ rng.uniform(-6.0, 6.0, 3) + rng.uniform(0, 2 * np.pi))
    values = np.clip(values / 2.5, -0.999, 0.999)
    colors = 0.5 + 0.5 * np.sin(P * rng.uniform(2.0, 9.0, 3) + P[..., ::-1] * rng.uniform(2.0, 9.0, 3)
                                + rng.uniform(0, 2 * np.pi, 3))
    return values.astype(np.float32), colors.astype(np.float32)


CHECKER_DIMS = (16, 16, 16)
CHECKER_LO, CHECKER_HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def checkerboard(dims=CHECKER_DIMS, magnitude=None, seed=11):
    """Sign (-1)^(i+j+k) times `magnitude`, or times a seeded magnitude in [0.25, 1] when it is None, with seeded colours:
    the most vertices and faces a volume can have (4 owned edges per interior node, 12 faces per cell).  With a constant
    magnitude every edge is a tie of |v_a| and |v_b|, t = 1/2, and every central difference is exactly 0."""
    rng = np.random.default_rng(seed)
    i, j, k = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    size = rng.uniform(0.25, 1.0, tuple(dims))
    values = np.where((i + j + k) % 2 == 0, 1.0, -1.0) * (size if magnitude is None else float(magnitude))
    colors = rng.uniform(0.0, 1.0, tuple(dims) + (3,))
    return values.astype(np.float32), colors.astype(np.float32)


def noise_volume(dims=CHECKER_DIMS, seed=13):
    """Seeded random signs and magnitudes in [0.25, 1]: every one of the 256 sign patterns of a cell occurs."""
    rng = np.random.default_rng(seed)
    values = np.where(rng.uniform(0.0, 1.0, tuple(dims)) < 0.5, -1.0, 1.0) * rng.uniform(0.25, 1.0, tuple(dims))
    colors = rng.uniform(0.0, 1.0, tuple(dims) + (3,))
    return values.astype(np.float32), colors.astype(np.float32)


def zeros_volume(seed=17):
    """smooth_field with a seeded 5 % of its nodes set to +0.0 and another 5 % to -0.0: both count as outside, and an
    active edge that ends on one has t = 0 or t = 1, its vertex on the node."""
    values, colors = smooth_field()
    rng = np.random.default_rng(seed)
    pick = rng.permutation(values.size)
    n = int(round(0.05 * values.size))
    flat = values.reshape(-1).copy()
    flat[pick[:n]] = np.float32(0.0)
    flat[pick[n:2 * n]] = np.float32(-0.0)
    return flat.reshape(values.shape), colors


def face_prefix_in_block(values, block=256):
    """Per node, the number of faces of the earlier cells of its block of 256 nodes (what the device packs into 13 bits)."""
    values = _f64(values)
    nx, ny, nz = values.shape
    ntri, _, _ = _face_table()
    inside = values < 0
    per_node = np.zeros(values.shape, dtype=np.int64)
    for tet in range(6):
        case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
        for p, c in enumerate(tet_corners(tet)):
            case |= inside[(c & 1):nx - 1 + (c & 1), ((c >> 1) & 1):ny - 1 + ((c >> 1) & 1),
                           (c >> 2):nz - 1 + (c >> 2)].astype(np.int64) << p
        per_node[:-1, :-1, :-1] += ntri[tet][case]
    flat = per_node.reshape(-1)
    padded = np.zeros(-(-flat.size // block) * block, dtype=np.int64)
    padded[:flat.size] = flat
    padded = padded.reshape(-1, block)
    return (np.cumsum(padded, axis=1) - padded).reshape(-1)[:flat.size]


FUSION_DIMS = (12, 10, 9)
FUSION_LO, FUSION_HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
FUSION_H, FUSION_W = 20, 24
FUSION_CENTER, FUSION_RADIUS, FUSION_WALL = (0.05, -0.03, 0.02), 0.6, 4.5
FUSION_OFFSET = (100.0, -200.0, 300.0)     # the translated scene: float32 coordinates a hundred times as long


def _look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """camera-to-world [3,4] of a camera at `eye` whose -z axis points at `target` (x right, y up)."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(np.asarray(up, dtype=np.float64), back)
    right /= np.linalg.norm(right)
    return np.concatenate([np.stack([right, np.cross(back, right), back], axis=1), eye[:, None]], axis=1)


def fusion_fixture(seed=3):
    """Three 24 x 20 cameras around a sphere of radius 0.6 inside the 12 x 10 x 9 volume, with analytic depth images (both
    kinds): camera 0 sees everything and its image has a block of zero depth; camera 1's narrow image leaves part of the
    volume outside; camera 2 stands inside the box with nodes behind it.  A ray that misses the sphere ends on a far wall
    (distance FUSION_WALL along the ray).  float32 arrays, as the device gets them; mask: seeded bytes, a fifth zero."""
    rng = np.random.default_rng(seed)
    c2w = np.stack([_look_at((0.013, -0.021, 3.0), (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)),
                    _look_at((2.9, 0.55, 0.31), (0.1, 0.0, 0.05)),
                    _look_at((0.11, -0.93, 0.07), (0.02, 0.4, 0.0))]).astype(np.float32)
    intrinsics = np.array([[20.3, 19.7, 11.71, 9.62], [41.0, 40.2, 12.37, 10.29], [14.1, 14.6, 11.83, 10.21]],
                          dtype=np.float32)
    R, t = _f64(c2w)[:, :, :3], _f64(c2w)[:, :, 3]
    rows, cols = np.meshgrid(np.arange(FUSION_H) + 0.5, np.arange(FUSION_W) + 0.5, indexing="ij")
    depth = np.zeros((2, 3, FUSION_H, FUSION_W))
    for c in range(3):
        fx, fy, cx, cy = _f64(intrinsics)[c]
        d_cam = np.stack([(cols - cx) / fx, -(rows - cy) / fy, -np.ones_like(cols)], axis=-1)
        scale = np.linalg.norm(d_cam, axis=-1)                              # ray distance per unit of z
        d = (d_cam / scale[..., None]) @ R[c].T
        oc = t[c] - np.array(FUSION_CENTER)
        b = d @ oc
        disc = b * b - (oc @ oc - FUSION_RADIUS ** 2)
        hit = (disc > 0) & (-b - np.sqrt(np.maximum(disc, 0.0)) > 0)
        along = np.where(hit, -b - np.sqrt(np.maximum(disc, 0.0)), FUSION_WALL)
        depth[1, c], depth[0, c] = along, along / scale
    depth[:, 0, 5:10, 8:14] = 0.0
    rgb = rng.uniform(0.0, 1.0, (3, FUSION_H, FUSION_W, 3))
    mask = (rng.uniform(0.0, 1.0, (3, FUSION_H, FUSION_W)) > 0.2).astype(np.uint8)
    return {"c2w": c2w, "intrinsics": intrinsics, "depth_z": depth[0].astype(np.float32),
            "depth_ray": depth[1].astype(np.float32), "rgb": rgb.astype(np.float32), "mask": mask}


def project(lo, hi, dims, c2w, intrinsics, H, W):
    """One camera's view of the nodes, in float64: front (z > 0), inside (front and the pixel lies in the image), and the
    pixel's row and column (0 where not inside), [nx,ny,nz] each."""
    c2w, intrinsics = _f64(c2w), _f64(intrinsics)
    q = (node_positions(lo, hi, dims) - c2w[:, 3]) @ c2w[:, :3]
    front = -q[..., 2] > 0
    z = np.where(front, -q[..., 2], 1.0)
    col = np.rint(intrinsics[0] * q[..., 0] / z + intrinsics[2] - 0.5)
    row = np.rint(intrinsics[1] * -q[..., 1] / z + intrinsics[3] - 0.5)
    inside = front & (col >= 0) & (col < W) & (row >= 0) & (row < H)
    return front, inside, np.where(inside, row, 0).astype(np.int64), np.where(inside, col, 0).astype(np.int64)


SPECIAL_DEPTHS = {"nan": np.float32(np.nan), "inf": np.float32(np.inf), "negative": np.float32(-1.0),
                  "negative zero": np.float32(-0.0), "tiny": np.float32(1e-30)}


def fusion_special_depths(fx, seed=5, per_kind=4):
    """fx with seeded pixels of camera 0's two depth images replaced by the SPECIAL_DEPTHS, per_kind pixels each, all
    among the pixels that nodes of the fusion volume project to and outside the block of zero depth.  -> the new fixture
    and {name: [(row, col), ...]}."""
    rng = np.random.default_rng(seed)
    _, inside, row, col = project(FUSION_LO, FUSION_HI, FUSION_DIMS, fx["c2w"][0], fx["intrinsics"][0], FUSION_H, FUSION_W)
    hit = np.unique(np.stack([row[inside], col[inside]], axis=1), axis=0)
    hit = hit[fx["depth_z"][0][hit[:, 0], hit[:, 1]] > 0]
    hit = hit[rng.permutation(hit.shape[0])]
    assert hit.shape[0] >= per_kind * len(SPECIAL_DEPTHS)
    out = dict(fx, depth_z=fx["depth_z"].copy(), depth_ray=fx["depth_ray"].copy())
    pixels = {}
    for n, (name, value) in enumerate(SPECIAL_DEPTHS.items()):
        pixels[name] = [tuple(int(x) for x in rc) for rc in hit[n * per_kind:(n + 1) * per_kind]]
        for r, c in pixels[name]:
            out["depth_z"][0, r, c] = out["depth_ray"][0, r, c] = value
    return out, pixels


def fusion_translated(fx, offset):
    """The fusion scene moved by `offset`: the box and the cameras' positions, rounded to float32 as the device gets
    them (so the moved scene is the original one up to that rounding); images and rotations are unchanged.
    -> the new fixture, lo, hi."""
    offset = np.asarray(offset, dtype=np.float64)
    c2w = fx["c2w"].astype(np.float64)
    c2w[:, :, 3] += offset
    lo = (np.asarray(FUSION_LO, dtype=np.float64) + offset).astype(np.float32)
    hi = (np.asarray(FUSION_HI, dtype=np.float64) + offset).astype(np.float32)
    return dict(fx, c2w=c2w.astype(np.float32)), tuple(float(x) for x in lo), tuple(float(x) for x in hi)
