"""GPU: the mesh filters (csrc/mesh_filters.hip through fruitnerf_amd/export/mesh.py, export_tsdf_mesh and
export_fruit_meshes) against the float64 restatement of their contract, tests/mesh_filters_reference.py (whose own checks
run in test_mesh_filters_cpu.py).  Every comparison is exact: np.array_equal on integer arrays and on the bytes of float
arrays.  The contract defines every sum as a sequential sum of rounded float64 operations, so there is no tolerance."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mesh_components_reference as mr
from tests import mesh_filters_reference as fr
from tests import util

pytestmark = pytest.mark.gpu


def _mesh(dev, vertices, faces, normals=None, colors=None):
    from fruitnerf_amd.export.mesh import TriangleMesh
    put = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)        # noqa: E731
    return TriangleMesh(put(vertices), put(faces), put(normals), put(colors))


def _same(tag, got, ref):
    """a device tensor and the reference's array: same dtype, shape and bytes"""
    got = got.cpu().numpy()
    ref = np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{tag}: {got.dtype} {got.shape} vs {ref.dtype} {ref.shape}"
    if got.dtype.kind == "f" and not np.array_equal(got.view(np.uint8), ref.view(np.uint8)):
        wrong = np.flatnonzero((got != ref).reshape(got.shape[0], -1).any(axis=1))
        print(f"[{tag}] {wrong.size} rows differ; first {wrong[:5].tolist()}: {got[wrong[:5]].tolist()} vs "
              f"{ref[wrong[:5]].tolist()}")
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), f"{tag}: the bits differ"


def _check_rows(tag, mesh, vertices, faces):
    V = vertices.shape[0]
    rows = {}
    for name, kind, method in (("neighbours", fr.NEIGHBOURS, mesh.vertex_adjacency), ("faces", fr.FACES, mesh.vertex_faces)):
        ref = fr.vertex_rows(faces, V, kind)
        got = method()
        assert method()[0] is got[0]                            # cached
        _same(f"{tag} {name} offsets", got[0], ref[0])
        _same(f"{tag} {name} entries", got[1], ref[1])
        rows[name] = ref
    return rows


def _check_filters(tag, mesh, vertices, faces, steps=True):
    rows = _check_rows(tag, mesh, vertices, faces)
    nb = rows["neighbours"]
    if steps:
        for weights, code in (("uniform", fr.UNIFORM), ("inverse_distance", fr.INVERSE_DISTANCE)):
            got = mesh.filter_smooth_laplacian(1, 0.5, weights=weights)
            _same(f"{tag} laplacian {weights}", got.vertices, fr.smooth(vertices, *nb, [0.5], code))
            assert got.faces is mesh.faces or torch.equal(got.faces, mesh.faces)
            got = mesh.filter_smooth_taubin(3, weights=weights)
            _same(f"{tag} taubin {weights}", got.vertices, fr.smooth(vertices, *nb, [0.5, -0.53] * 3, code))
    _same(f"{tag} normals", mesh.compute_vertex_normals().normals, fr.vertex_normals(vertices, faces, *rows["faces"]))


def _check_clustering(tag, mesh, vertices, faces, voxel_size, normals=None, colors=None):
    nv, nf, nn, nc, c = fr.simplify(vertices, faces, voxel_size, normals, colors)
    from fruitnerf_amd import _kernels as K
    origin = fr.cluster_origin(vertices, voxel_size)
    raw = K.mesh_cluster(mesh.vertices, mesh.faces, voxel_size, origin.tolist())
    for k in ("vertex_cluster", "offsets", "members", "new_faces", "face_ids"):
        _same(f"{tag} cluster {k}", raw[k], c[k])
    got = mesh.simplify_vertex_clustering(voxel_size)
    _same(f"{tag} clustered vertices", got.vertices, nv)
    _same(f"{tag} clustered faces", got.faces, nf)
    _same(f"{tag} vertex_cluster", got.vertex_cluster, c["vertex_cluster"])
    for name, ref in (("normals", nn), ("colors", nc)):
        assert (getattr(got, name) is None) == (ref is None)
        if ref is not None:
            _same(f"{tag} clustered {name}", getattr(got, name), ref)
    return got, c


# ---- 1. hand-made meshes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 5])
@pytest.mark.parametrize("name", sorted(mr.hand_made()))
def test_hand_made_meshes(dev, name, extra):
    vertices, faces, _ = mr.hand_made()[name]
    if extra:
        vertices, faces = fr.with_unreferenced(vertices, faces, extra)
    rng = np.random.default_rng(4)
    colors = rng.uniform(0, 1, vertices.shape).astype(np.float32)
    normals = rng.standard_normal(vertices.shape).astype(np.float32)
    mesh = _mesh(dev, vertices, faces, normals, colors)
    _check_filters(name, mesh, vertices, faces)
    smoothed = mesh.filter_smooth_taubin(1)
    assert torch.equal(smoothed.normals, mesh.normals) and torch.equal(smoothed.colors, mesh.colors)
    for voxel_size in (0.45, 1.1):
        _check_clustering(f"{name} {voxel_size}", mesh, vertices, faces, voxel_size, normals, colors)
    _check_clustering(f"{name} bare", _mesh(dev, vertices, faces), vertices, faces, 0.45)


# ---- 2. a row longer than a wave, a workgroup and any per-thread buffer -------------------------------------------------
def test_a_hub_of_a_thousand_neighbours(dev):
    vertices, faces, _ = mr.triangles_and_fan(301, 1000, seed=6)
    mesh = _mesh(dev, vertices, faces)
    offsets, _ = fr.vertex_rows(faces, vertices.shape[0], fr.NEIGHBOURS)
    assert int(np.diff(offsets).max()) == 1001
    _check_filters("fan", mesh, vertices, faces)
    _check_clustering("fan", mesh, vertices, faces, 0.3)


# ---- 3. more than 2^16 vertices: the sort's third byte -------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_strip():
    vertices, faces, _ = mr.strip(70001, (17000,), seed=3)
    assert vertices.shape[0] > 1 << 16 and faces.shape[0] % 64 != 0 and (6 * faces.shape[0]) % 256 != 0
    nb = fr.vertex_rows(faces, vertices.shape[0], fr.NEIGHBOURS)
    return SimpleNamespace(vertices=vertices, faces=faces, nb=nb, taubin=fr.smooth(vertices, *nb, [0.5, -0.53] * 2))


def test_a_long_strip(dev, long_strip):
    s = long_strip
    mesh = _mesh(dev, s.vertices, s.faces)
    _check_filters("strip", mesh, s.vertices, s.faces, steps=False)
    _same("strip taubin", mesh.filter_smooth_taubin(2).vertices, s.taubin)
    _check_clustering("strip", mesh, s.vertices, s.faces, 0.025)


# ---- 4. three spheres and a speck, through the TSDF ---------------------------------------------------------------------
def test_spheres_through_the_tsdf(dev):
    from fruitnerf_amd.export.tsdf import TSDF
    tsdf = TSDF.from_aabb(torch.tensor([mr.SPHERES_LO, mr.SPHERES_HI]), mr.SPHERES_DIMS, dev)
    tsdf.values.copy_(torch.as_tensor(mr.spheres_volume()))
    tsdf.colors.copy_(torch.rand(mr.SPHERES_DIMS + (3,), generator=torch.Generator().manual_seed(2)))
    mesh = tsdf.get_triangle_mesh()
    vertices, faces, normals, colors = [t.cpu().numpy() for t in (mesh.vertices, mesh.faces, mesh.normals, mesh.colors)]
    assert (vertices.shape[0], faces.shape[0]) == mr.SPHERES_COUNTS
    _check_filters("spheres", mesh, vertices, faces)
    # ten Taubin pairs: exact, and the topology is what it was
    smoothed = mesh.filter_smooth_taubin(10)
    ref = fr.taubin(vertices, faces, 10)
    _same("spheres taubin 10", smoothed.vertices, ref)
    before, after = mesh.component_stats(), smoothed.component_stats()
    assert smoothed.connected_components()[1] == mesh.connected_components()[1] == 4
    assert bool(after.closed.all()) and torch.equal(after.n_faces, before.n_faces)
    labels = smoothed.connected_components()[0].cpu().numpy()
    for c in range(4):
        n_c = int(after.n_faces[c])
        assert np.unique(faces[labels == c]).size - 3 * n_c // 2 + n_c == 2
    ratio = (after.volume / before.volume).cpu().numpy()[[0, 3, 2]]
    print("[spheres] Taubin volume ratios", ratio.tolist())
    assert (np.abs(ratio - 1.0) < 0.02).all()
    # clustering: the identity at a tiny voxel, the reference's arrays at one cell
    same, _ = _check_clustering("spheres 1e-4", mesh, vertices, faces, 1e-4, normals, colors)
    assert torch.equal(same.vertices, mesh.vertices) and torch.equal(same.faces, mesh.faces)
    assert torch.equal(same.colors, mesh.colors)
    coarse, c = _check_clustering("spheres 0.1", mesh, vertices, faces, 0.1, normals, colors)
    assert (coarse.n_vertices, coarse.n_faces, c["n_duplicates"]) == (340, 674, 2)


# ---- 5. the duplicate and degenerate rules -------------------------------------------------------------------------------
def test_duplicates_and_collapsing_faces(dev):
    from fruitnerf_amd import _kernels as K
    vertices, faces, face_ids, new_faces = fr.duplicate_case()
    mesh = _mesh(dev, vertices, faces)
    out = K.mesh_cluster(mesh.vertices, mesh.faces, 1.0, fr.cluster_origin(vertices, 1.0).tolist())
    _same("face_ids", out["face_ids"], face_ids)
    _same("new_faces", out["new_faces"], new_faces)
    assert out["vertex_cluster"].tolist() == [0, 1, 2, 3, 3] and out["offsets"].tolist() == [0, 1, 2, 3, 5]
    _check_clustering("duplicates", mesh, vertices, faces, 1.0)
    # the mean of a hand-made row set, an empty row included
    offsets = torch.tensor([0, 2, 2, 5], dtype=torch.int32, device=dev)
    members = torch.tensor([4, 0, 1, 2, 3], dtype=torch.int32, device=dev)
    _same("rows_mean", K.mesh_rows_mean(offsets, members, mesh.vertices),
          fr.rows_mean(offsets.cpu().numpy(), members.cpu().numpy(), vertices))


# ---- 6. determinism ------------------------------------------------------------------------------------------------------
def test_face_order_and_runs(dev, long_strip):
    s = long_strip
    order = np.random.default_rng(9).permutation(s.faces.shape[0])
    moved = _mesh(dev, s.vertices, s.faces[order])
    _same("permuted offsets", moved.vertex_adjacency()[0], s.nb[0])
    _same("permuted neighbours", moved.vertex_adjacency()[1], s.nb[1])
    _same("permuted taubin", moved.filter_smooth_taubin(2).vertices, s.taubin)
    runs = []
    for _ in range(2):
        mesh = _mesh(dev, s.vertices, s.faces[order])
        clustered = mesh.simplify_vertex_clustering(0.025)
        runs.append([*mesh.vertex_adjacency(), *mesh.vertex_faces(), mesh.filter_smooth_taubin(2).vertices,
                     mesh.compute_vertex_normals().normals, clustered.vertices, clustered.faces, clustered.vertex_cluster])
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))


# ---- 7. empty ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vertices", [0, 5])
def test_empty_meshes(dev, n_vertices):
    from fruitnerf_amd import _lib as L
    vertices = np.random.default_rng(1).uniform(-1, 1, (n_vertices, 3)).astype(np.float32)
    faces = np.zeros((0, 3), dtype=np.int32)
    mesh = _mesh(dev, vertices, faces)
    log = L.begin_call_log()
    try:
        rows = [mesh.vertex_adjacency(), mesh.vertex_faces()]
    finally:
        names = L.end_call_log(log)
    assert names == []                                           # no faces: no call at all
    for offsets, entries in rows:
        assert offsets.dtype == entries.dtype == torch.int32 and entries.shape == (0,)
        assert offsets.shape == (n_vertices + 1,) and not offsets.any()
    for out in (mesh.filter_smooth_laplacian(2), mesh.filter_smooth_taubin(2)):
        assert out.faces.shape == (0, 3) and out.normals is None
        _same("empty smoothing", out.vertices, vertices)
    normals = mesh.compute_vertex_normals().normals
    assert normals.dtype == torch.float32 and normals.shape == (n_vertices, 3) and not normals.any()
    got, c = _check_clustering("empty", mesh, vertices, faces, 0.5)
    assert got.faces.shape == (0, 3) and got.faces.dtype == torch.int32 and got.vertices.dtype == torch.float32
    assert got.vertex_cluster.shape == (n_vertices,) and got.vertex_cluster.dtype == torch.int32


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_library_usable(dev):
    from fruitnerf_amd import _kernels as K
    vertices, faces, _ = mr.hand_made()["tets_sharing_an_edge"]
    mesh = _mesh(dev, vertices, faces)
    for voxel_size in (0.0, -0.5, float("nan")):
        with pytest.raises(RuntimeError, match="voxel_size"):
            mesh.simplify_vertex_clustering(voxel_size)
    bad = vertices.copy()
    bad[3, 1] = np.nan
    with pytest.raises(RuntimeError, match="finite"):
        _mesh(dev, bad, faces).simplify_vertex_clustering(0.5)
    with pytest.raises(RuntimeError, match="finite"):           # the same vertex against a finite origin: found on the device
        K.mesh_cluster(torch.as_tensor(bad, device=dev), mesh.faces, 0.5, [-2.0, -2.0, -2.0])
    with pytest.raises(RuntimeError, match="cells"):            # 2^21 cells on an axis, and a negative cell
        K.mesh_cluster(mesh.vertices, mesh.faces, 2.0 ** -21, [0.0, 0.0, 0.0])
    with pytest.raises(RuntimeError, match="cells"):
        K.mesh_cluster(mesh.vertices, mesh.faces, 0.5, [0.5, 0.5, 0.5])
    outside = faces.copy()
    outside[2, 1] = vertices.shape[0]
    for kind in (K.MESH_ROWS_NEIGHBOURS, K.MESH_ROWS_FACES):
        with pytest.raises(RuntimeError, match="outside"):
            K.mesh_vertex_rows(torch.as_tensor(outside, device=dev), vertices.shape[0], kind)
    with pytest.raises(RuntimeError, match="outside"):
        _mesh(dev, vertices, outside).simplify_vertex_clustering(0.5)
    negative = faces.copy()
    negative[0, 0] = -1
    with pytest.raises(RuntimeError, match="outside"):
        _mesh(dev, vertices, negative).vertex_adjacency()
    # rows that are not rows of this mesh
    offsets, nb = mesh.vertex_adjacency()
    with pytest.raises(RuntimeError, match="rows"):
        K.mesh_smooth(mesh.vertices, offsets, nb + 100, [0.5])
    with pytest.raises(RuntimeError, match="rows"):
        K.mesh_smooth(mesh.vertices, offsets.flip(0).contiguous(), nb, [0.5])
    with pytest.raises(ValueError):
        mesh.filter_smooth_taubin(1, weights="cotangent")
    _check_filters("after the refusals", mesh, vertices, faces)
    _check_clustering("after the refusals", mesh, vertices, faces, 0.5)


# ---- 9. the exporters, end to end -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    from fruitnerf_amd.cameras.cameras import Cameras
    from fruitnerf_amd.data import synthetic_apple as sa
    n_cam, HW = 3, 16
    focal = 1111.0 * HW / 800
    # density_boost 0: the rendered depth ends inside the box, so the fused volume has nodes on both sides of a surface
    oracle = util.randomize_(util.make_oracle(util.small_config(log2=4), num_images=n_cam, randomize=False), 1,
                             density_boost=0.0)
    model = util.make_hip_like(oracle, dev)
    model.eval()
    c2w = sa.make_cameras(n_cam, seed=0, device=dev).float()
    fx = torch.tensor([focal, 1.05 * focal, 0.97 * focal])
    cy = torch.tensor([8.1, 7.6, 8.3])
    cameras = Cameras(c2w, fx, focal, 8.2, cy, width=HW, height=HW,
                      distortion_params=torch.tensor([0.2, -0.05, 0.0, 0.0, 1e-2, -1e-2]))
    pipeline = SimpleNamespace(model=model, datamanager=SimpleNamespace(train_dataset=SimpleNamespace(cameras=cameras)))
    return SimpleNamespace(model=model, cameras=cameras, pipeline=pipeline, dev=dev)


_EXPORT = dict(downscale_factor=1, resolution=8, batch_size=2)
_FILTERS = dict(smooth_iterations=2, simplify_voxel_size=2.0 * 2.0 / 8)         # two cells of the 8-node volume over [-1, 1]
_NO_FILTERS = dict(smooth_iterations=None, smooth_lambda=0.5, smooth_mu=-0.53, simplify_voxel_size=None)


def _reference_filters(vertices, faces, normals, colors):
    """the exporters' filters restated: two Taubin pairs, clustering, normals from the faces"""
    smoothed = fr.taubin(vertices, faces, 2)
    nv, nf, _, nc, _ = fr.simplify(smoothed, faces, _FILTERS["simplify_voxel_size"], None, colors)
    return nv, nf, fr.vertex_normals(nv, nf), nc


def test_export_tsdf_mesh_filters(scene, tmp_path):
    from fruitnerf_amd.export import ply
    from fruitnerf_amd.export.exporter_utils import export_tsdf_mesh
    export_tsdf_mesh(scene.pipeline, tmp_path / "plain", **_EXPORT)
    tsdf = export_tsdf_mesh(scene.pipeline, tmp_path / "none", **_NO_FILTERS, **_EXPORT)
    plain = (tmp_path / "plain" / "tsdf_mesh.ply").read_bytes()
    assert plain == (tmp_path / "none" / "tsdf_mesh.ply").read_bytes() and len(plain) > 0
    tsdf.export(str(tmp_path / "direct.ply"))
    assert plain == (tmp_path / "direct.ply").read_bytes()
    again = export_tsdf_mesh(scene.pipeline, tmp_path / "filtered", **_FILTERS, **_EXPORT)
    assert torch.equal(again.values, tsdf.values)
    vertices, faces, normals, colors = [t.cpu().numpy() for t in tsdf.get_mesh()]
    nv, nf, nn, nc = _reference_filters(vertices, faces, normals, colors)
    print(f"[export] {vertices.shape[0]} vertices / {faces.shape[0]} faces -> {nv.shape[0]} / {nf.shape[0]}")
    assert 0 < nf.shape[0] < faces.shape[0]
    ply.write_triangle_mesh(str(tmp_path / "ref.ply"), nv, nf, nn, nc)
    assert (tmp_path / "filtered" / "tsdf_mesh.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes()


def test_export_fruit_meshes_filters(scene, tmp_path):
    from fruitnerf_amd.export import ply
    from fruitnerf_amd.export.exporter_utils import export_fruit_meshes
    first = export_fruit_meshes(scene.pipeline, tmp_path / "probe", semantic_threshold=0.0, min_component_faces=1, **_EXPORT)
    middle = float(first.vertex_probability.median())
    arguments = dict(semantic_threshold=middle, min_component_faces=1, **_EXPORT)
    plain = export_fruit_meshes(scene.pipeline, tmp_path / "plain", **arguments)
    none = export_fruit_meshes(scene.pipeline, tmp_path / "none", **_NO_FILTERS, **arguments)
    for name in ("fruit_mesh.ply", "fruits.json"):
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "none" / name).read_bytes()
    assert 0 < plain.mesh.n_faces < plain.full.n_faces and torch.equal(none.mesh.vertices, plain.mesh.vertices)
    result = export_fruit_meshes(scene.pipeline, tmp_path / "filtered", **_FILTERS, **arguments)
    assert torch.equal(result.full.vertices, plain.full.vertices) and torch.equal(result.full.faces, plain.full.faces)
    assert torch.equal(result.vertex_probability, plain.vertex_probability) and torch.equal(result.tsdf.values, plain.tsdf.values)
    # the filtered fruit mesh is the restatement applied to the unfiltered one
    vertices, faces, normals, colors = [t.cpu().numpy() for t in (plain.mesh.vertices, plain.mesh.faces, plain.mesh.normals,
                                                                  plain.mesh.colors)]
    nv, nf, nn, nc = _reference_filters(vertices, faces, normals, colors)
    for name, ref in (("vertices", nv), ("faces", nf), ("normals", nn), ("colors", nc)):
        _same(f"fruit {name}", getattr(result.mesh, name), ref)
    ply.write_triangle_mesh(str(tmp_path / "ref.ply"), nv, nf, nn, nc)
    assert (tmp_path / "filtered" / "fruit_mesh.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes()
    # components and statistics are those of the filtered mesh
    labels, n = mr.components(nf)
    ref = mr.stats(nv, nf, labels, n)
    assert np.array_equal(result.face_component.cpu().numpy(), labels) and len(result) == n
    stats = result.stats
    records = json.loads((tmp_path / "filtered" / "fruits.json").read_text())
    assert len(records) == n
    for c, record in enumerate(records):
        assert sorted(record) == ["area", "centroid", "closed", "faces", "hi", "lo", "volume"]
        assert record["faces"] == int(ref["n_faces"][c]) == int(stats.n_faces[c])
        assert record["closed"] == bool(ref["boundary_edges"][c] == 0 and ref["nonmanifold_edges"][c] == 0)
        assert record["area"] == float(stats.area[c]) and record["volume"] == float(stats.volume[c])
        for k in ("area", "volume"):
            assert abs(record[k] - ref[k][c]) <= mr.sum_bound(ref["n_faces"], ref["abs_" + k])[c]
        assert np.array_equal(np.float32(record["lo"]), ref["lo"][c]) and np.array_equal(np.float32(record["hi"]), ref["hi"][c])
    assert scene.model.training is False
