"""CPU: the TSDF mesh export's ABI surface (entry points, struct, argument checks before any launch), the triangle-mesh
PLY round trip, Cameras.rescale_output_resolution, and the self-checks of the float64 reference (tests/tsdf_reference.py)
that the GPU suite (test_gpu_tsdf.py) measures the kernels against."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tsdf_reference as tr


def _volume(L, dims=(4, 4, 4), lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), margin=5.0, max_weight=1.0, ptr=8):
    v = L.fnr_tsdf_volume()
    v.dims[:], v.lo[:], v.hi[:] = dims, lo, hi
    v.truncation_margin, v.max_weight = margin, max_weight
    v.values = v.weights = v.colors = ptr          # never dereferenced on the host; every call below fails its checks
    return v


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    for name in ("fnr_tsdf_integrate", "fnr_tsdf_mesh_count", "fnr_tsdf_mesh_emit"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert C.sizeof(L.fnr_tsdf_volume) == 3 * 4 + 6 * 4 + 2 * 4 + 4 + 3 * 8      # 11 words padded to 48, three pointers
    hdr = open(L._HERE + "/../include/fruitnerf_hip.h").read()
    assert "#define FNR_TSDF_MESH_WORKSPACE_BYTES(n_nodes) (4 * (size_t)(n_nodes) + 16 * (((size_t)(n_nodes) + 255) / 256) + 16)" in hdr
    assert L.tsdf_mesh_workspace_bytes(64) == 4 * 64 + 16 + 16 and L.tsdf_mesh_workspace_bytes(257) == 4 * 257 + 32 + 16
    assert "#define FNR_TSDF_DEPTH_Z 0" in hdr and "#define FNR_TSDF_DEPTH_RAY 1" in hdr
    assert (L.FNR_TSDF_DEPTH_Z, L.FNR_TSDF_DEPTH_RAY) == (0, 1)
    err = lib.fnr_last_error
    p = 8

    def integrate(vol, n=1, c2w=p, intr=p, H=4, W=4, depth=p, rgb=p, mask=None, kind=1):
        return lib.fnr_tsdf_integrate(None if vol is None else C.byref(vol), n, c2w, intr, H, W, depth, rgb, mask, kind, None)

    assert integrate(None) == -1 and b"tsdf_integrate: null volume" in err()
    assert integrate(_volume(L, ptr=None)) == -1 and b"null volume array" in err()
    assert integrate(_volume(L, dims=(4, 1, 4))) == -1 and b"dims[1]" in err()
    assert integrate(_volume(L, dims=(4, 4, 4096))) == -1 and b"dims[2]" in err()
    assert integrate(_volume(L, lo=(1.0, -1.0, -1.0))) == -1 and b"lo[0] < hi[0]" in err()
    assert integrate(_volume(L, hi=(1.0, float("nan"), 1.0))) == -1 and b"lo[1] < hi[1]" in err()
    assert integrate(_volume(L, margin=0.0)) == -1 and b"truncation_margin" in err()
    assert integrate(_volume(L, max_weight=0.5)) == -1 and b"max_weight" in err()
    ok = _volume(L)
    assert integrate(ok, n=-1) == -1 and b"n_cameras" in err()
    assert integrate(ok, kind=2) == -1 and b"depth_kind" in err()
    assert integrate(ok, H=0) == -1 and b"image size" in err()
    assert integrate(ok, W=1 << 20) == -1 and b"image size" in err()
    for null in ("c2w", "intr", "depth", "rgb"):
        assert integrate(ok, **{null: None}) == -1 and b"tsdf_integrate: null argument" in err()
    assert integrate(ok, n=0, c2w=None, intr=None, depth=None, rgb=None) == 0         # an empty batch launches nothing

    need = L.tsdf_mesh_workspace_bytes(64)
    count = lambda vol, counts=p, ws=p, nbytes=need: lib.fnr_tsdf_mesh_count(    # noqa: E731
        None if vol is None else C.byref(vol), counts, ws, nbytes, None)
    assert count(None) == -1 and b"tsdf_mesh_count: null volume" in err()
    assert count(_volume(L, dims=(1, 4, 4))) == -1 and b"dims[0]" in err()
    assert count(ok, ws=None) == -1 and b"null workspace" in err()
    assert count(ok, ws=12) == -1 and b"8-byte aligned" in err()
    assert count(ok, nbytes=need - 1) == -1 and b"workspace" in err()
    assert count(ok, counts=None) == -1 and b"null counts" in err()

    def emit(vol, ws=p, nbytes=need, nv=3, nf=1, vertices=p, normals=p, colors=p, faces=p):
        return lib.fnr_tsdf_mesh_emit(None if vol is None else C.byref(vol), ws, nbytes, nv, nf, vertices, normals, colors,
                                      faces, None)

    assert emit(None) == -1 and b"tsdf_mesh_emit: null volume" in err()
    assert emit(ok, ws=None) == -1 and b"null workspace" in err()
    assert emit(ok, nbytes=0) == -1 and b"workspace" in err()
    assert emit(ok, nv=-1) == -1 and emit(ok, nf=-1) == -1
    assert emit(ok, nv=1 << 31) == -1 and b"int32" in err()
    for null in ("vertices", "normals", "colors"):
        assert emit(ok, **{null: None}) == -1 and b"null vertex array" in err()
    assert emit(ok, faces=None) == -1 and b"null faces" in err()
    assert emit(ok, nv=0, nf=0, vertices=None, normals=None, colors=None, faces=None) == 0   # an empty mesh: nothing to write


def test_entry_points_are_unrecordable_in_step_programs():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    for call, name in ((lambda: lib.fnr_tsdf_integrate(None, 0, None, None, 1, 1, None, None, None, 0, None), b"fnr_tsdf_integrate"),
                       (lambda: lib.fnr_tsdf_mesh_count(None, None, None, 0, None), b"fnr_tsdf_mesh_count"),
                       (lambda: lib.fnr_tsdf_mesh_emit(None, None, 0, 0, 0, None, None, None, None, None), b"fnr_tsdf_mesh_emit")):
        h = C.c_void_p()
        assert lib.fnr_program_create(C.byref(h)) == 0
        try:
            assert lib.fnr_program_begin(h) == 0
            assert call() == -1                                    # bad arguments: nothing is launched
            assert lib.fnr_program_end(h) == -2 and name in lib.fnr_last_error()
        finally:
            assert lib.fnr_program_destroy(h) == 0


def test_python_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from fruitnerf_amd import _kernels as K
    from fruitnerf_amd.export.tsdf import TSDF
    z = torch.zeros(4, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.TsdfVolumeArg(z, z.clone(), torch.zeros(4, 4, 4, 3), (-1, -1, -1), (1, 1, 1), 5.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        TSDF.from_aabb(torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 8, "cpu")
    with pytest.raises(ValueError, match="aabb"):
        TSDF.from_aabb(torch.zeros(3, 2), 8, "cpu")
    with pytest.raises(ValueError, match="volume_dims"):
        TSDF.from_aabb(torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), (8, 8), "cpu")


def test_triangle_mesh_ply_round_trip(tmp_path):
    from fruitnerf_amd.export import ply
    rng = np.random.default_rng(0)
    vertices = rng.standard_normal((37, 3)).astype(np.float32)
    normals = rng.standard_normal((37, 3)).astype(np.float32)
    colors = rng.uniform(-0.1, 1.1, (37, 3)).astype(np.float32)
    faces = rng.integers(0, 37, (52, 3)).astype(np.int32)
    path = str(tmp_path / "sub" / "mesh.ply")
    ply.write_triangle_mesh(path, vertices, faces, normals, colors)
    raw = open(path, "rb").read()
    header = raw[:raw.index(b"end_header\n") + 11].decode("ascii")
    assert header.startswith("ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\n")
    assert "property float nz\nproperty uchar red\n" in header
    assert header.endswith("element face 52\nproperty list uchar uint vertex_indices\nend_header\n")
    assert len(raw) == len(header) + 37 * 27 + 52 * 13
    v, f, n, c = ply.read_triangle_mesh(path)
    assert v.dtype == np.float32 and np.array_equal(v, vertices) and n.dtype == np.float32 and np.array_equal(n, normals)
    assert f.dtype == np.int32 and np.array_equal(f, faces)
    assert np.array_equal(c, np.rint(np.clip(colors.astype(np.float64), 0.0, 1.0) * 255.0) / 255.0)
    # an empty mesh is a valid file
    empty = str(tmp_path / "empty.ply")
    ply.write_triangle_mesh(empty, np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32), np.zeros((0, 3)), np.zeros((0, 3)))
    v, f, n, c = ply.read_triangle_mesh(empty)
    assert v.shape == n.shape == c.shape == (0, 3) and f.shape == (0, 3) and f.dtype == np.int32
    with pytest.raises(ValueError, match="face indices"):
        ply.write_triangle_mesh(empty, vertices, faces + 1, normals, colors)
    with pytest.raises(ValueError, match="normals"):
        ply.write_triangle_mesh(empty, vertices, faces, normals[:-1], colors)
    # the point-cloud reader / writer are untouched by the mesh layout, and do not read it
    ply.write_point_cloud(empty, vertices, np.clip(colors, 0, 1))
    with pytest.raises(ValueError, match="triangle mesh"):
        ply.read_triangle_mesh(empty)
    with open(empty, "wb") as fh:
        fh.write(raw[:-1])
    with pytest.raises(ValueError, match="bytes of data"):
        ply.read_triangle_mesh(empty)


def test_rescale_output_resolution_on_per_frame_intrinsics():
    from fruitnerf_amd.cameras.cameras import Cameras
    c2w = torch.eye(4)[:3].repeat(3, 1, 1)
    fx, fy = torch.tensor([400.0, 410.5, 399.25]), torch.tensor([401.0, 409.5, 398.75])
    cx, cy = torch.tensor([160.5, 158.0, 161.25]), torch.tensor([120.0, 121.5, 119.75])
    dist = torch.tensor([0.1, -0.02, 0.0, 0.0, 1e-3, -1e-3])
    cams = Cameras(c2w, fx, fy, cx, cy, width=321, height=243, distortion_params=dist)
    assert cams.rescale_output_resolution(0.5) is None                       # in place, like Nerfstudio's
    assert (cams.height, cams.width) == (121, 160)                           # floor(243 / 2), floor(321 / 2)
    for got, was in ((cams.fx, fx), (cams.fy, fy), (cams.cx, cx), (cams.cy, cy)):
        assert got.shape == (3, 1) and got.dtype == torch.float32 and torch.equal(got[:, 0], was * 0.5)
    assert torch.equal(cams.camera_to_worlds, c2w) and torch.equal(cams.distortion_params, dist[None].expand(3, 6))
    cams.rescale_output_resolution(1.0 / 3.0)
    assert (cams.height, cams.width) == (40, 53)
    assert torch.allclose(cams.fx[:, 0], fx / 6.0, rtol=1e-6, atol=0) and torch.allclose(cams.cy[:, 0], cy / 6.0, rtol=1e-6, atol=0)
    cams.rescale_output_resolution(2.0)
    assert (cams.height, cams.width) == (80, 106)
    scalar = Cameras(c2w, 100.0, 100.0, 16.0, 12.0, width=32, height=24)     # per-dataset intrinsics
    scalar.rescale_output_resolution(0.25)
    assert (scalar.height, scalar.width) == (6, 8) and torch.equal(scalar.cx, torch.full((3, 1), 4.0))
    for bad in (0.0, -1.0, float("nan"), 0.01):
        with pytest.raises(ValueError):
            scalar.rescale_output_resolution(bad)
    assert (scalar.height, scalar.width) == (6, 8)


# ---- self-checks of the reference --------------------------------------------------------------------------------------
def test_reference_tetrahedra_fill_the_cell_and_match_across_cells():
    """The six tetrahedra are the 3! walks from corner 0 to corner 7: each has volume 1/6, and every face of the unit cell
    is cut by the diagonal through its lowest corner, so that neighbouring cells agree."""
    offset = lambda c: np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)   # noqa: E731
    total = 0.0
    diagonals = set()
    for t in range(6):
        c = tr.tet_corners(t)
        assert c[0] == 0 and c[3] == 7 and bin(c[1]).count("1") == 1 and bin(c[2]).count("1") == 2 and c[1] & c[2] == c[1]
        p = [offset(x) for x in c]
        total += abs(np.linalg.det(np.stack([p[1] - p[0], p[2] - p[0], p[3] - p[0]]))) / 6.0
        for a in range(4):
            for b in range(a + 1, 4):
                if bin(c[a] ^ c[b]).count("1") == 2:
                    diagonals.add((c[a], c[b]))
    assert total == pytest.approx(1.0)
    assert len({tr.tet_corners(t) for t in range(6)}) == 6
    # one diagonal per cell face, each from the face's lowest corner: direction codes 3, 5, 6, on the near and the far face
    assert diagonals == {(0, 3), (0, 5), (0, 6), (4, 7), (2, 7), (1, 7)}
    for t in range(6):
        assert tr.tet_triangles(t, 0) == [] and tr.tet_triangles(t, 15) == []
        for case in range(1, 15):
            tris = tr.tet_triangles(t, case)
            assert len(tris) == (2 if bin(case).count("1") == 2 else 1)
            flipped = tr.tet_triangles(t, 15 - case)                  # the other side inside: same edges, turned round
            key = lambda tri: tuple(sorted(tuple(sorted(e)) for e in tri))     # noqa: E731
            assert sorted(key(x) for x in tris) == sorted(key(x) for x in flipped)


def test_reference_mesh_of_the_analytic_sphere():
    values, colors = tr.sphere_volume()
    assert values.shape == tr.SPHERE_DIMS and not bool((values == 0).any())
    inside = values < 0
    border = np.ones(tr.SPHERE_DIMS, dtype=bool)
    border[2:-2, 2:-2, 2:-2] = False
    assert bool(inside.any()) and not bool((inside & border).any())       # the surface stays clear of the border
    mesh = tr.extract(values, colors, tr.SPHERE_LO, tr.SPHERE_HI)
    V, F = mesh["vertices"].shape[0], mesh["faces"].shape[0]
    report = tr.mesh_report(mesh["vertices"], mesh["faces"])
    assert report["closed_oriented"] and report["degenerate"] == 0 and report["used_vertices"] == V
    assert report["euler"] == 2 and F == 2 * V - 4
    assert report["volume"] > 0
    delta = tr.sphere_delta()
    radius = np.linalg.norm(mesh["vertices"] - np.array(tr.SPHERE_CENTER), axis=1)
    print(f"[sphere] V {V} F {F} delta {delta:.6f} max |radius - r| {np.abs(radius - tr.SPHERE_RADIUS).max():.6f} "
          f"volume {report['volume']:.6f}")
    assert float(np.abs(radius - tr.SPHERE_RADIUS).max()) <= delta
    ball = lambda r: 4.0 / 3.0 * np.pi * r ** 3                           # noqa: E731
    assert ball(tr.SPHERE_RADIUS - 2 * delta) <= report["volume"] <= ball(tr.SPHERE_RADIUS + 2 * delta)
    # normals are unit and point outwards, colours are those of an endpoint
    assert np.allclose(np.linalg.norm(mesh["normals"], axis=1), 1.0, atol=1e-12)
    assert float(((mesh["vertices"] - np.array(tr.SPHERE_CENTER)) * mesh["normals"]).sum(1).min()) > 0
    flat = colors.reshape(-1, 3).astype(np.float64)
    a = mesh["keys"] // 8
    m = mesh["keys"] % 8
    b = a + ((m & 1) * tr.SPHERE_DIMS[1] + ((m >> 1) & 1)) * tr.SPHERE_DIMS[2] + (m >> 2)
    assert bool(((mesh["colors"] == flat[a]).all(1) | (mesh["colors"] == flat[b]).all(1)).all())
    assert bool((np.diff(mesh["keys"]) > 0).all())


def test_reference_smooth_field_reaches_every_case():
    values, colors = tr.smooth_field()
    assert values.shape == tr.FIELD_DIMS and not bool((values == 0).any())
    mesh = tr.extract(values, colors, tr.FIELD_LO, tr.FIELD_HI)
    assert mesh["cases"] == set(range(16))
    assert mesh["faces"].shape[0] > 0 and int(mesh["faces"].max()) == mesh["keys"].shape[0] - 1
    # an open surface (it runs into the border), still consistently oriented: no directed edge twice
    directed = [(f[e], f[(e + 1) % 3]) for f in mesh["faces"].tolist() for e in range(3)]
    assert len(set(directed)) == len(directed)
    assert len(tr.oriented_faces(mesh["face_keys"])) == mesh["faces"].shape[0]


# ---- the array reference and the fixtures of the large-volume GPU tests -----------------------------------------------
_SMALL = {"field": (tr.smooth_field, tr.FIELD_LO, tr.FIELD_HI),
          "sphere": (tr.sphere_volume, tr.SPHERE_LO, tr.SPHERE_HI),
          "zeros": (tr.zeros_volume, tr.FIELD_LO, tr.FIELD_HI),
          "checker": (tr.checkerboard, tr.CHECKER_LO, tr.CHECKER_HI),
          "checker_tie": (lambda: tr.checkerboard(magnitude=0.5), tr.CHECKER_LO, tr.CHECKER_HI),
          "noise": (tr.noise_volume, tr.CHECKER_LO, tr.CHECKER_HI)}
_small_cache = {}


def _small(name):
    """(values, colors, lo, hi, extract_fast's mesh) of a small fixture, computed once."""
    if name not in _small_cache:
        make, lo, hi = _SMALL[name]
        values, colors = make()
        _small_cache[name] = (values, colors, lo, hi, tr.extract_fast(values, colors, lo, hi))
    return _small_cache[name]


def _ulps64(a, b):
    """|a - b| in units of the float64 spacing at max(|a|, |b|, smallest normal)."""
    return np.abs(a - b) / np.spacing(np.maximum(np.maximum(np.abs(a), np.abs(b)), np.finfo(np.float64).tiny))


@pytest.mark.parametrize("name", sorted(_SMALL))
def test_extract_fast_equals_extract(name):
    """What lets the GPU tests trust extract_fast where extract cannot run: integers, positions and colours equal exactly,
    normals within 4 ulp of float64 (the norm is taken differently)."""
    values, colors, lo, hi, fast = _small(name)
    slow = tr.extract(values, colors, lo, hi)
    assert fast["keys"].size > 0 and fast["faces"].shape[0] > 0
    for k in ("keys", "faces", "face_keys"):
        assert fast[k].dtype == slow[k].dtype == np.int64 and np.array_equal(fast[k], slow[k]), k
    for k in ("vertices", "colors"):
        assert fast[k].dtype == np.float64 and np.array_equal(fast[k], slow[k]), k
    assert fast["cases"] == slow["cases"]
    worst = float(_ulps64(fast["normals"], slow["normals"]).max())
    print(f"[extract_fast {name}] V {fast['keys'].size} F {fast['faces'].shape[0]}; normals differ by {worst:.1f} ulp64")
    assert worst <= 4.0
    assert np.array_equal(fast["normals"] == 0, slow["normals"] == 0)
    # no exclusions: the unnormalised normal is non-zero on every vertex, except where the tie checkerboard makes it so
    cond = tr.normal_condition(values, lo, hi)
    assert cond.shape == (fast["keys"].size,) and bool((cond[np.isfinite(cond)] >= 1.0).all())
    if name != "checker_tie":
        assert bool(np.isfinite(cond).all())


@pytest.mark.parametrize("dims", [d for d in tr.SCAN_DIMS if d != (128, 128, 128)])
def test_scan_volumes_span_the_trips_of_the_block_scan(dims):
    blocks, trips = tr.SCAN_DIMS[dims]
    values, colors = tr.scan_volume(dims)
    assert values.dtype == colors.dtype == np.float32 and values.shape == dims and not bool((values == 0).any())
    assert -(-values.size // 256) == blocks and -(-blocks // tr.SCAN_BLOCKS_PER_TRIP) == trips
    if dims == (45, 343, 17):
        assert blocks % tr.SCAN_BLOCKS_PER_TRIP == 1 and values.size % 256 == 251
    if dims == (64, 64, 64):
        assert blocks == tr.SCAN_BLOCKS_PER_TRIP and values.size % 256 == 0
    # colours are not constant: not over the nodes, not over the channels
    flat = colors.reshape(-1, 3)
    assert float(flat.std(0).min()) > 0.1
    assert float((flat[:, 0] != flat[:, 1]).mean()) > 0.99 and float((flat[:, 1] != flat[:, 2]).mean()) > 0.99
    assert float((flat[1:] != flat[:-1]).any(1).mean()) > 0.99
    mesh = tr.extract_fast(values, colors, tr.SCAN_LO, tr.SCAN_HI)
    owners = np.unique(tr.block_of_key(mesh["keys"]))
    print(f"[scan {dims}] {blocks} blocks, {trips} trips; V {mesh['keys'].size} F {mesh['faces'].shape[0]}; "
          f"{owners.size} blocks own a vertex")
    assert 0.9 * blocks < owners.size < blocks                   # nearly every block offset is used, and some count zero
    assert int(owners.max()) // tr.SCAN_BLOCKS_PER_TRIP == trips - 1          # the last trip owns vertices too
    assert mesh["cases"] == set(range(16))
    assert bool(np.isfinite(tr.normal_condition(values, tr.SCAN_LO, tr.SCAN_HI)).all())
    expected = {(64, 64, 64): (82059, 161066, 1011), (45, 343, 17): (117089, 226716, 1002),
                (81, 81, 81): (132397, 260932, 2012)}[dims]
    assert (mesh["keys"].size, mesh["faces"].shape[0], owners.size) == expected


def test_checkerboard_fills_the_packed_word():
    """4 owned edges per interior node (direction codes 1, 2, 4, 7) and 12 faces per cell: the face prefix inside a block
    passes 2048, the top of the 13-bit field."""
    values, colors, lo, hi, mesh = _small("checker")
    n = tr.CHECKER_DIMS[0]
    assert float(np.abs(values).min()) >= 0.25 and float(np.abs(values).max()) <= 1.0 and np.unique(np.abs(values)).size > 1000
    assert mesh["faces"].shape[0] == 12 * (n - 1) ** 3 == 40500
    assert mesh["keys"].size == 14895
    owned = np.bincount(mesh["keys"] // 8, minlength=values.size).reshape(values.shape)
    assert bool((owned[:-1, :-1, :-1] == 4).all())
    assert set((mesh["keys"][np.isin(mesh["keys"] // 8, np.arange(values.size).reshape(values.shape)[:-1, :-1, :-1])] % 8)
               .tolist()) == {1, 2, 4, 7}
    prefix = tr.face_prefix_in_block(values)
    vertex_prefix = (np.cumsum(owned.reshape(-1, 256), axis=1) - owned.reshape(-1, 256))
    print(f"[checkerboard] largest face prefix in a block {int(prefix.max())}, largest vertex prefix {int(vertex_prefix.max())}")
    assert int(prefix.max()) > 2048 and int(prefix.max()) < 1 << 13 and int(vertex_prefix.max()) < 1 << 11


def test_tie_checkerboard_has_ties_and_zero_normals():
    values, colors, lo, hi, mesh = _small("checker_tie")
    assert bool((np.abs(values) == 0.5).all())
    a, b, m = tr.active_edges(values)
    assert a.size == mesh["keys"].size == 14895
    flat = colors.reshape(-1, 3).astype(np.float64)
    assert np.array_equal(mesh["colors"], flat[a]) and int((flat[a] != flat[b]).any(1).sum()) == a.size   # a tie goes to a
    P = tr.node_positions(lo, hi, values.shape).reshape(-1, 3)
    assert np.array_equal(mesh["vertices"], P[a] + 0.5 * (P[b] - P[a]))
    # an edge whose endpoints are interior on all three axes: both central differences are 0 - 0, the normal is (0, 0, 0);
    # an edge that touches the border has a one-sided, non-zero gradient
    ijk = lambda n: np.stack(np.unravel_index(n, values.shape), axis=1)                                  # noqa: E731
    interior = lambda n: ((ijk(n) > 0) & (ijk(n) < np.array(values.shape) - 1)).all(1)                   # noqa: E731
    both = interior(a) & interior(b)
    zero = (mesh["normals"] == 0).all(1)
    print(f"[tie checkerboard] {int(zero.sum())} zero normals, {int((~zero).sum())} others of {a.size}")
    assert bool(zero[both].all()) and int(both.sum()) > 1000 and int((~zero).sum()) > 1000
    assert bool((~both[~zero]).all())
    assert np.allclose(np.linalg.norm(mesh["normals"][~zero], axis=1), 1.0, atol=1e-12)


def test_noise_volume_reaches_every_cell_pattern():
    values, colors, lo, hi, mesh = _small("noise")
    inside = values < 0
    n = tr.CHECKER_DIMS[0]
    pattern = sum(inside[(c & 1):n - 1 + (c & 1), ((c >> 1) & 1):n - 1 + ((c >> 1) & 1), (c >> 2):n - 1 + (c >> 2)]
                  .astype(np.int64) << c for c in range(8))
    assert np.unique(pattern).size == 256
    assert float(np.abs(values).min()) >= 0.25 and mesh["cases"] == set(range(16))


def test_zeros_volume_puts_vertices_on_nodes():
    values, colors, lo, hi, mesh = _small("zeros")
    plain, _ = tr.smooth_field()
    flat = values.reshape(-1)
    positive, negative = (flat == 0) & ~np.signbit(flat), (flat == 0) & np.signbit(flat)
    assert int(positive.sum()) == int(negative.sum()) == round(0.05 * flat.size) and np.array_equal(colors, tr.smooth_field()[1])
    assert np.array_equal(flat[flat != 0], plain.reshape(-1)[flat != 0])
    a, b, m = tr.active_edges(values)
    t, _, _ = tr.normal_terms(values, lo, hi)
    va, vb = flat[a].astype(np.float64), flat[b].astype(np.float64)
    assert not bool((va == vb).any())                            # +0 and -0 are both outside: never an active edge
    for name, at_zero in (("+0.0", positive), ("-0.0", negative)):
        assert int(((t == 0) & at_zero[a]).sum()) > 0, f"no active edge leaves a node of {name}"
        assert int(((t == 1) & at_zero[b]).sum()) > 0, f"no active edge ends on a node of {name}"
    assert np.array_equal(t == 0, va == 0) and np.array_equal(t == 1, vb == 0)
    # a vertex with t = 0 or 1 lies on its node, and several edges meet there
    P = tr.node_positions(lo, hi, values.shape).reshape(-1, 3)
    on = np.where(t == 0, a, b)[(t == 0) | (t == 1)]
    assert np.array_equal(mesh["vertices"][(t == 0) | (t == 1)], P[on])
    assert int(np.bincount(on).max()) > 1
    assert np.array_equal(mesh["colors"][(t == 0) | (t == 1)], colors.reshape(-1, 3).astype(np.float64)[on])


def test_normal_yardstick_of_the_float32_evaluation():
    """The yardstick of the GPU normal test: the normal's formulas in float32 NumPy against extract_fast, as the worst of
    |error| / (eps32 cond) over the fixtures (cond = |S| / |n|, tr.normal_condition).  Measured: 0.51 to 0.67 per fixture
    (0.05 on the tie checkerboard, whose arithmetic is nearly exact), with cond up to 308 on the checkerboard; the kernel
    is granted 4 x the worst over the GPU module's fixtures."""
    worst = {}
    cases = [(name,) + _small(name)[:4] + (_small(name)[4]["normals"],) for name in sorted(_SMALL)]
    for dims in tr.SCAN_DIMS:
        if dims != (128, 128, 128):
            values, colors = tr.scan_volume(dims)
            cases.append((f"scan {dims}", values, colors, tr.SCAN_LO, tr.SCAN_HI,
                          tr.extract_fast(values, colors, tr.SCAN_LO, tr.SCAN_HI)["normals"]))
    for name, values, colors, lo, hi, normals in cases:
        cond = tr.normal_condition(values, lo, hi)
        got = tr.normals_float32(values, lo, hi)
        assert got.dtype == np.float32 and got.shape == normals.shape
        worst[name] = tr.normal_ratio(got, normals, cond)
        assert np.array_equal((got == 0).all(1), ~np.isfinite(cond))         # zero exactly where the reference is zero
        print(f"[normal yardstick {name}] float32 on the CPU: worst |error| / (eps32 cond) {worst[name]:.3f}; "
              f"largest cond {float(cond[np.isfinite(cond)].max()):.3g}; worst |error| "
              f"{float(np.abs(got - normals).max()):.3g}")
    print(f"[normal yardstick] worst over the fixtures {max(worst.values()):.3f}")
    # a float32 evaluation of a dozen operations whose error the condition number accounts for: a few eps32, not more
    assert 0.1 < max(worst.values()) < 4.0


def test_fusion_special_depths_reach_nodes():
    """NaN, +inf, negative, -0.0 and 1e-30 in camera 0's depth: nodes project onto each kind; +inf gives a valid sample
    with s = 1, the others give none; the nodes that may be left out stay under 1 %."""
    fx = tr.fusion_fixture()
    special, pixels = tr.fusion_special_depths(fx)
    assert set(pixels) == set(tr.SPECIAL_DEPTHS) and all(len(set(p)) == 4 for p in pixels.values())
    assert len({rc for p in pixels.values() for rc in p}) == 20
    n_nodes = int(np.prod(tr.FUSION_DIMS))
    _, inside, row, col = tr.project(tr.FUSION_LO, tr.FUSION_HI, tr.FUSION_DIMS, fx["c2w"][0], fx["intrinsics"][0],
                                     tr.FUSION_H, tr.FUSION_W)
    for kind in (0, 1):
        key = "depth_ray" if kind else "depth_z"
        changed = special[key] != fx[key]
        assert int(changed.sum()) == 20 and not bool(changed[1:].any())          # the old depths there are positive
        for name, value in tr.SPECIAL_DEPTHS.items():
            for r, c in pixels[name]:
                got = special[key][0, r, c]
                assert (np.isnan(got) if name == "nan" else got == value and np.signbit(got) == np.signbit(value))
        args = (tr.FUSION_LO, tr.FUSION_HI, fx["c2w"][:1], fx["intrinsics"][:1])
        (values, weights, _), near = tr.integrate(tr.empty_volume(tr.FUSION_DIMS), *args, special[key][:1], fx["rgb"][:1],
                                                  depth_kind=kind, max_weight=1e9)
        (_, before, _), _ = tr.integrate(tr.empty_volume(tr.FUSION_DIMS), *args, fx[key][:1], fx["rgb"][:1],
                                         depth_kind=kind, max_weight=1e9)
        for name in tr.SPECIAL_DEPTHS:
            on = np.zeros(tr.FUSION_DIMS, dtype=bool)
            for r, c in pixels[name]:
                on |= inside & (row == r) & (col == c)
            assert int(on.sum()) >= 4, f"{name}: no node projects there"
            if name == "inf":
                assert bool((weights[on] == 1.0).all()) and bool((values[on] == 1.0).all())
            else:
                assert bool((weights[on] == 0.0).all()) and bool((values[on] == -1.0).all())
                assert int((before[on] == 1.0).sum()) > 0 or name == "tiny"      # the pixel took a sample away
        for max_weight in (1.0, 1e9):
            for mask in (None, fx["mask"]):
                (values, weights, colors), near = tr.integrate(
                    tr.empty_volume(tr.FUSION_DIMS), tr.FUSION_LO, tr.FUSION_HI, fx["c2w"], fx["intrinsics"], special[key],
                    fx["rgb"], mask, depth_kind=kind, max_weight=max_weight)
                assert int(near.sum()) <= 0.01 * n_nodes
                assert bool(np.isfinite(values).all()) and bool(np.isfinite(colors).all()) and bool(np.isfinite(weights).all())


@pytest.mark.parametrize("max_weight", [2.0, 2.5])
def test_fusion_max_weight_between_one_and_the_cameras(max_weight):
    """With three cameras the clamp binds on the third only: a node seen twice has weight 2, a node seen three times has
    max_weight, and its value is the average that the clamped weight gives."""
    fx = tr.fusion_fixture()
    args = (tr.FUSION_LO, tr.FUSION_HI, fx["c2w"], fx["intrinsics"], fx["depth_ray"], fx["rgb"])
    (values, weights, _), near = tr.integrate(tr.empty_volume(tr.FUSION_DIMS), *args, max_weight=max_weight)
    (plain, seen, _), _ = tr.integrate(tr.empty_volume(tr.FUSION_DIMS), *args, max_weight=1e9)
    assert float(weights.max()) == max_weight and int(near.sum()) <= 0.01 * near.size
    assert int((seen == 2).sum()) > 0 and bool((weights[seen == 2] == 2.0).all())
    assert int((seen == 3).sum()) > 0 and bool((weights[seen == 3] == max_weight).all())
    assert np.array_equal(values, plain)          # the clamp acts after the last camera: nothing is averaged with it
    (two, w2, _), _ = tr.integrate(tr.empty_volume(tr.FUSION_DIMS), tr.FUSION_LO, tr.FUSION_HI, fx["c2w"][:2],
                                   fx["intrinsics"][:2], fx["depth_ray"][:2], fx["rgb"][:2], max_weight=max_weight)
    assert float(w2.max()) == 2.0 and int((w2 == 2.0).sum()) > 0


def test_fusion_translated_scene_stays_clear_of_ties():
    """The scene moved by (100, -200, 300): the bound grows with the coordinate, the share of nodes near a tie does not."""
    fx = tr.fusion_fixture()
    moved, lo, hi = tr.fusion_translated(fx, tr.FUSION_OFFSET)
    assert lo == (99.0, -201.0, 299.0) and hi == (101.0, -199.0, 301.0)
    assert np.array_equal(moved["c2w"][:, :, :3], fx["c2w"][:, :, :3])
    assert float(np.abs(moved["c2w"][:, :, 3].astype(np.float64) - fx["c2w"][:, :, 3] - np.array(tr.FUSION_OFFSET)).max()) \
        <= 0.5 * tr.EPS32 * 512
    for kind in (0, 1):
        for max_weight in (1.0, 1e9):
            for mask in (None, fx["mask"]):
                (values, weights, _), near = tr.integrate(
                    tr.empty_volume(tr.FUSION_DIMS), lo, hi, moved["c2w"], moved["intrinsics"],
                    moved["depth_ray" if kind else "depth_z"], moved["rgb"], mask, depth_kind=kind, max_weight=max_weight)
                assert int(near.sum()) <= 0.01 * near.size
                assert float(weights.max()) == (1.0 if max_weight == 1.0 else 3.0) and 0 < int((values < 0).sum()) < near.size
    bound = tr.fusion_bound(lo, hi, tr.FUSION_DIMS, moved["c2w"])
    assert 90 < bound / tr.fusion_bound(tr.FUSION_LO, tr.FUSION_HI, tr.FUSION_DIMS, fx["c2w"]) < 110


def test_reference_fusion_fixture_stays_clear_of_ties():
    """The fixture of the GPU comparison: every situation the issue names occurs, and the nodes that may be left out (near
    a rounding tie or a validity edge, in float64) stay under 1 % of the volume in every configuration."""
    fx = tr.fusion_fixture()
    n_nodes = int(np.prod(tr.FUSION_DIMS))
    assert fx["depth_z"].shape == (3, tr.FUSION_H, tr.FUSION_W) and bool((fx["depth_z"][0, 5:10, 8:14] == 0).all())
    assert bool((fx["depth_z"][1:] > 0).all()) and bool((fx["depth_z"] <= fx["depth_ray"]).all())
    P = tr.node_positions(tr.FUSION_LO, tr.FUSION_HI, tr.FUSION_DIMS)
    behind, outside = [], []
    for c in range(3):
        q = (P - fx["c2w"][c, :, 3].astype(np.float64)) @ fx["c2w"][c, :, :3].astype(np.float64)
        front = -q[..., 2] > 0
        z = np.where(front, -q[..., 2], 1.0)
        col = np.rint(fx["intrinsics"][c, 0] * q[..., 0] / z + fx["intrinsics"][c, 2] - 0.5)
        row = np.rint(fx["intrinsics"][c, 1] * -q[..., 1] / z + fx["intrinsics"][c, 3] - 0.5)
        behind.append(int((~front).sum()))
        outside.append(int((front & ~((col >= 0) & (col < tr.FUSION_W) & (row >= 0) & (row < tr.FUSION_H))).sum()))
    assert behind[0] == 0 and outside[0] == 0 and behind[1] == 0 and outside[1] > 100 and behind[2] > 50
    for kind in (0, 1):
        for max_weight in (1.0, 1e9):
            for mask in (None, fx["mask"]):
                (values, weights, colors), near = tr.integrate(
                    tr.empty_volume(tr.FUSION_DIMS), tr.FUSION_LO, tr.FUSION_HI, fx["c2w"], fx["intrinsics"],
                    fx["depth_ray" if kind else "depth_z"], fx["rgb"], mask, depth_kind=kind, max_weight=max_weight)
                assert int(near.sum()) <= 0.01 * n_nodes
                assert float(weights.max()) == (1.0 if max_weight == 1.0 else 3.0)
                assert bool(((weights == 0) == (values == -1.0)).all()) and bool((colors[weights == 0] == 0).all())
                assert bool((values[weights > 0] > -1.0).all()) and float(values.max()) == 1.0
                assert 0 < int((values < 0).sum()) < n_nodes
    # one call with three cameras is three calls with one
    whole, _ = tr.integrate(tr.empty_volume(tr.FUSION_DIMS), tr.FUSION_LO, tr.FUSION_HI, fx["c2w"], fx["intrinsics"],
                            fx["depth_ray"], fx["rgb"], fx["mask"], max_weight=1e9)
    parts = tr.empty_volume(tr.FUSION_DIMS)
    for c in range(3):
        parts, _ = tr.integrate(parts, tr.FUSION_LO, tr.FUSION_HI, fx["c2w"][c:c + 1], fx["intrinsics"][c:c + 1],
                                fx["depth_ray"][c:c + 1], fx["rgb"][c:c + 1], fx["mask"][c:c + 1], max_weight=1e9)
    assert all(np.array_equal(a, b) for a, b in zip(whole, parts))
    assert 1e-6 < tr.fusion_bound(tr.FUSION_LO, tr.FUSION_HI, tr.FUSION_DIMS, fx["c2w"]) < 1e-5
