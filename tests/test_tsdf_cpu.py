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
