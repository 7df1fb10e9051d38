"""GPU: mesh connectivity (csrc/mesh.hip through fruitnerf_amd/export/mesh.py, TSDF.get_triangle_mesh, export_tsdf_mesh and
export_fruit_meshes) against the float64 restatement of its contract, tests/mesh_components_reference.py (whose own checks
run in test_mesh_components_cpu.py).  Labels, counts, integer statistics, boxes and selected arrays are compared exactly; a
float64 sum of component c within (n_c + 32) * 2^-52 * A_c, A_c the reference's sum of the absolute-value terms (the
summation-order bound of n_c - 1 additions on either side plus a few roundings per term; derived, not measured)."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mesh_components_reference as mr
from tests import util

pytestmark = pytest.mark.gpu

_SUMS = ("area", "volume", "moment")


def _mesh(dev, vertices, faces):
    from fruitnerf_amd.export.mesh import TriangleMesh
    return TriangleMesh(torch.as_tensor(vertices, device=dev), torch.as_tensor(faces, device=dev))


def _stats_arrays(stats):
    return {k: getattr(stats, k).cpu().numpy() for k in ("n_faces", "boundary_edges", "nonmanifold_edges", "lo", "hi",
                                                         "area", "volume", "moment", "centroid", "closed")}


def _compare(tag, mesh, vertices, faces, expected_components=None):
    """the device's labels and statistics against the reference's; -> (labels, reference statistics, device statistics)"""
    ref_labels, n = mr.components(faces)
    labels, n_dev = mesh.connected_components()
    assert labels.dtype == torch.int32 and labels.shape == (faces.shape[0],)
    assert n_dev == n and np.array_equal(labels.cpu().numpy(), ref_labels), f"{tag}: components differ"
    if expected_components is not None:
        assert n == expected_components
    ref = mr.stats(vertices, faces, ref_labels, n)
    got = _stats_arrays(mesh.component_stats())
    for k in ("n_faces", "boundary_edges", "nonmanifold_edges"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), f"{tag}: {k} differ"
    for k in ("lo", "hi"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k], ref[k]), f"{tag}: {k} differ"
    for k in _SUMS:
        bound = mr.sum_bound(ref["n_faces"], ref["abs_" + k])
        err = np.abs(got[k] - ref[k])
        worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if err.size else 0.0
        print(f"[{tag}] {k}: max |error| {float(err.max()) if err.size else 0.0:.3g}, largest share of the bound {worst:.3g}")
        assert got[k].dtype == np.float64 and bool((err <= bound).all()), f"{tag}: {k} outside the bound"
    assert np.array_equal(got["closed"], (ref["boundary_edges"] == 0) & (ref["nonmanifold_edges"] == 0))
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(got["centroid"], got["moment"] / got["area"][:, None], equal_nan=True)
    triple = mesh.cluster_connected_triangles()
    assert np.array_equal(triple[0].cpu().numpy(), ref_labels) and np.array_equal(triple[1].cpu().numpy(), ref["n_faces"])
    assert triple[2].dtype == torch.float64 and np.array_equal(triple[2].cpu().numpy(), got["area"])
    return ref_labels, ref, got


def _compare_selection(tag, mesh, selected, vertices, faces, keep):
    new_faces, vertex_ids, face_ids = mr.select(faces, vertices.shape[0], keep)
    assert np.array_equal(selected.faces.cpu().numpy(), new_faces), f"{tag}: selected faces differ"
    assert np.array_equal(selected.vertices.cpu().numpy(), vertices[vertex_ids]), f"{tag}: selected vertices differ"
    for name in ("normals", "colors"):
        whole, part = getattr(mesh, name), getattr(selected, name)
        assert (whole is None) == (part is None)
        if whole is not None:
            assert np.array_equal(part.cpu().numpy(), whole.cpu().numpy()[vertex_ids]), f"{tag}: selected {name} differ"
    return new_faces, vertex_ids, face_ids


# ---- 1. hand-made meshes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mr.hand_made()))
def test_hand_made_meshes(dev, name):
    from fruitnerf_amd import _kernels as K
    vertices, faces, expected = mr.hand_made()[name]
    mesh = _mesh(dev, vertices, faces)
    labels, ref, _ = _compare(name, mesh, vertices, faces, expected)
    if name == "three_on_one_edge":
        assert ref["nonmanifold_edges"].tolist() == [1]
    # selection: every second face; the raw arrays of the kernel wrapper, then the mesh method
    keep = np.arange(faces.shape[0]) % 2 == 0
    new_faces, vertex_ids, face_ids = mr.select(faces, vertices.shape[0], keep)
    got = [t.cpu().numpy() for t in K.mesh_select(mesh.faces, mesh.n_vertices, torch.as_tensor(keep, device=dev))]
    assert all(a.dtype == np.int32 for a in got)
    assert np.array_equal(got[0], new_faces) and np.array_equal(got[1], vertex_ids) and np.array_equal(got[2], face_ids)
    _compare_selection(name, mesh, mesh.select_by_face_mask(torch.as_tensor(keep, device=dev)), vertices, faces, keep)
    vmask = np.arange(vertices.shape[0]) != int(faces[0, 0])
    _compare_selection(name + " by vertex", mesh, mesh.select_by_vertex_mask(torch.as_tensor(vmask, device=dev)), vertices,
                       faces, mr.vertex_mask_faces(faces, vmask))


def test_labels_with_indices_near_2_to_the_31(dev):
    """n_vertices = 2^31 - 1 and no vertex array: the edge keys have to be 64 bits wide"""
    from fruitnerf_amd import _kernels as K
    n_vertices, faces, expected = mr.top_index_faces()
    ref_labels, n = mr.components(faces)
    labels, n_dev, _ = K.mesh_components(torch.as_tensor(faces, device=dev), n_vertices)
    assert n_dev == n == expected and np.array_equal(labels.cpu().numpy(), ref_labels)
    with pytest.raises(RuntimeError, match="outside"):              # the same faces over too few vertices: refused
        K.mesh_components(torch.as_tensor(faces, device=dev), 1000)


# ---- 2. strips: deep union-find trees, sizes that are no multiple of 64 or 256, components longer than 64 blocks ---------
@pytest.mark.parametrize("total,cuts", [(4101, (1200, 2900)), (20003, (17000,))])
def test_cut_strip(dev, total, cuts):
    vertices, faces, pieces = mr.strip(total, cuts, seed=3)
    assert faces.shape[0] == total - len(cuts) and faces.shape[0] % 64 != 0
    mesh = _mesh(dev, vertices, faces)
    _, ref, got = _compare(f"strip {total}", mesh, vertices, faces, len(cuts) + 1)
    assert sorted(got["n_faces"].tolist()) == pieces
    assert np.array_equal(got["boundary_edges"], got["n_faces"] + 2) and not got["nonmanifold_edges"].any()
    keep = mr.largest_component_faces(faces, 1)
    _compare_selection("strip largest", mesh, mesh.keep_largest_components(1), vertices, faces, keep)


# ---- 3. many components --------------------------------------------------------------------------------------------------
def test_disjoint_triangles_and_a_fan(dev):
    vertices, faces, expected = mr.triangles_and_fan()
    mesh = _mesh(dev, vertices, faces)
    _, ref, got = _compare("triangles and fan", mesh, vertices, faces, expected)
    assert int((got["n_faces"] == 1).sum()) == 3001 and got["boundary_edges"][got["n_faces"] == 64].tolist() == [66]
    _compare_selection("fan alone", mesh, mesh.remove_small_components(2), vertices, faces, mr.small_component_faces(faces, 2))


# ---- 4. three spheres and a speck, through the TSDF ---------------------------------------------------------------------
def test_spheres_through_the_tsdf(dev):
    from fruitnerf_amd.export.tsdf import TSDF
    tsdf = TSDF.from_aabb(torch.tensor([mr.SPHERES_LO, mr.SPHERES_HI]), mr.SPHERES_DIMS, dev)
    tsdf.values.copy_(torch.as_tensor(mr.spheres_volume()))
    tsdf.colors.copy_(torch.rand(mr.SPHERES_DIMS + (3,), generator=torch.Generator().manual_seed(2)))
    mesh = tsdf.get_triangle_mesh()
    for a, b in zip((mesh.vertices, mesh.faces, mesh.normals, mesh.colors), tsdf.get_mesh()):
        assert torch.equal(a, b)
    vertices, faces = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    assert (vertices.shape[0], faces.shape[0]) == mr.SPHERES_COUNTS
    _, ref, got = _compare("spheres", mesh, vertices, faces, 4)
    assert tuple(got["n_faces"].tolist()) == mr.SPHERES_COMPONENT_FACES
    assert bool(got["closed"].all()) and bool((got["volume"] > 0).all())
    labels = mesh.connected_components()[0].cpu().numpy()
    for c in range(4):                                     # closed and oriented: Euler characteristic 2
        n_c = int(got["n_faces"][c])
        assert np.unique(faces[labels == c]).size - 3 * n_c // 2 + n_c == 2
    ball = 4.0 / 3.0 * np.pi * np.array(mr.SPHERES_RADII) ** 3
    print("[spheres] volumes", got["volume"].tolist(), "balls", ball.tolist())
    # components 0, 3, 2 are the spheres of radius 0.31, 0.27, 0.22 (by first face), a little inside their balls
    assert bool((got["volume"][[0, 3, 2]] < ball).all()) and bool((got["volume"][[0, 3, 2]] > 0.8 * ball).all())
    assert got["volume"][1] < 1e-2 * got["volume"][2]
    cleaned = mesh.remove_small_components(25)
    assert cleaned.n_faces == 2376 and cleaned.connected_components()[1] == 3
    _compare_selection("spheres cleaned", mesh, cleaned, vertices, faces, mr.small_component_faces(faces, 25))
    _compare_selection("spheres largest two", mesh, mesh.keep_largest_components(2), vertices, faces,
                       mr.largest_component_faces(faces, 2))


# ---- 5. determinism ------------------------------------------------------------------------------------------------------
def test_runs_agree_bit_for_bit_and_permutations_within_the_bound(dev):
    rng = np.random.default_rng(9)
    strip_v, strip_f, _ = mr.strip(20003, (17000,), seed=4)
    fan_v, fan_f, _ = mr.triangles_and_fan(301, 64, seed=6)
    vertices = np.concatenate([strip_v, fan_v])
    faces = np.concatenate([strip_f, fan_f + strip_v.shape[0]])[rng.permutation(strip_f.shape[0] + fan_f.shape[0])]
    first = _mesh(dev, vertices, faces)
    second = _mesh(dev, vertices, faces)
    a, b = _stats_arrays(first.component_stats()), _stats_arrays(second.component_stats())
    assert torch.equal(first.connected_components()[0], second.connected_components()[0])
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{k}: two runs differ in their bits"
    # the same faces in another order: the same partition, the same statistics after matching the components
    order = rng.permutation(faces.shape[0])
    moved = _mesh(dev, vertices, faces[order])
    labels = first.connected_components()[0].cpu().numpy()
    moved_labels = moved.connected_components()[0].cpu().numpy()
    assert moved.connected_components()[1] == first.connected_components()[1]
    match = np.full(a["n_faces"].shape[0], -1)
    match[labels[order]] = moved_labels                       # component c of the first mesh is match[c] of the moved one
    assert np.array_equal(match[labels[order]], moved_labels) and np.unique(match).size == match.size
    c = _stats_arrays(moved.component_stats())
    for k in ("n_faces", "boundary_edges", "nonmanifold_edges", "lo", "hi"):
        assert np.array_equal(a[k], c[k][match])
    ref = mr.stats(vertices, faces, labels, match.size)
    for k in _SUMS:
        assert bool((np.abs(a[k] - c[k][match]) <= mr.sum_bound(ref["n_faces"], ref["abs_" + k])).all())


# ---- 6. empty ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vertices", [0, 5])
def test_empty_meshes(dev, n_vertices):
    mesh = _mesh(dev, np.zeros((n_vertices, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32))
    labels, n = mesh.connected_components()
    assert n == 0 and labels.shape == (0,) and labels.dtype == torch.int32
    stats = mesh.component_stats()
    assert len(stats) == 0 and stats.n_faces.dtype == torch.int32 and stats.area.dtype == torch.float64
    assert stats.lo.shape == stats.hi.shape == stats.moment.shape == stats.centroid.shape == (0, 3)
    assert stats.lo.dtype == torch.float32 and stats.closed.dtype == torch.bool
    triple = mesh.cluster_connected_triangles()
    assert [t.shape for t in triple] == [(0,), (0,), (0,)] and triple[2].dtype == torch.float64
    for selected in (mesh.select_by_face_mask(torch.zeros(0, dtype=torch.bool, device=dev)), mesh.remove_small_components(3),
                     mesh.keep_largest_components(2),
                     mesh.select_by_vertex_mask(torch.ones(n_vertices, dtype=torch.bool, device=dev))):
        assert selected.vertices.shape == (0, 3) and selected.faces.shape == (0, 3) and selected.faces.dtype == torch.int32
    # a mesh whose faces are all dropped
    one = _mesh(dev, np.eye(3, dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32))
    none = one.select_by_face_mask(torch.zeros(1, dtype=torch.bool, device=dev))
    assert none.vertices.shape == (0, 3) and none.faces.shape == (0, 3)


# ---- 7. the exporters, end to end -------------------------------------------------------------------------------------
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


def test_export_tsdf_mesh_cleans_components(scene, tmp_path):
    from fruitnerf_amd.export import ply
    from fruitnerf_amd.export.exporter_utils import export_tsdf_mesh
    export_tsdf_mesh(scene.pipeline, tmp_path / "plain", **_EXPORT)
    tsdf = export_tsdf_mesh(scene.pipeline, tmp_path / "none", min_component_faces=None, largest_components=None, **_EXPORT)
    plain = (tmp_path / "plain" / "tsdf_mesh.ply").read_bytes()
    assert plain == (tmp_path / "none" / "tsdf_mesh.ply").read_bytes() and len(plain) > 0
    vertices, faces, normals, colors = [t.cpu().numpy() for t in tsdf.get_mesh()]
    labels, n = mr.components(faces)
    sizes = np.bincount(labels, minlength=n)
    print(f"[export] {faces.shape[0]} faces in {n} components of {sorted(sizes.tolist())} faces")
    assert faces.shape[0] > 0
    threshold = int(sizes.max())                         # keeps the largest component(s), drops every smaller one
    for tag, kw, keep in (("min", dict(min_component_faces=threshold), mr.small_component_faces(faces, threshold)),
                          ("largest", dict(largest_components=1), mr.largest_component_faces(faces, 1))):
        again = export_tsdf_mesh(scene.pipeline, tmp_path / tag, **kw, **_EXPORT)
        assert torch.equal(again.values, tsdf.values)
        new_faces, vertex_ids, _ = mr.select(faces, vertices.shape[0], keep)
        ply.write_triangle_mesh(str(tmp_path / (tag + "_ref.ply")), vertices[vertex_ids], new_faces, normals[vertex_ids],
                                colors[vertex_ids])
        assert (tmp_path / tag / "tsdf_mesh.ply").read_bytes() == (tmp_path / (tag + "_ref.ply")).read_bytes()


def test_export_fruit_meshes(scene, tmp_path):
    from fruitnerf_amd.export import ply
    from fruitnerf_amd.export.exporter_utils import export_fruit_meshes, export_tsdf_mesh
    from fruitnerf_amd.fruit_field import FieldHeadNames
    from fruitnerf_amd.rays import Frustums, RaySamples
    dev = scene.dev
    tsdf = export_tsdf_mesh(scene.pipeline, tmp_path / "scene", **_EXPORT)
    full = tsdf.get_triangle_mesh()
    V, F = full.n_vertices, full.n_faces
    # the vertex probabilities, recomputed through model.field
    directions = -full.normals
    directions[(full.normals == 0).all(1)] = torch.tensor([0.0, 0.0, -1.0], device=dev)
    zeros = torch.zeros(V, 1, device=dev)
    samples = RaySamples(Frustums(full.vertices, directions, zeros, zeros, zeros),
                         camera_indices=torch.zeros(V, 1, dtype=torch.int32, device=dev))
    with torch.no_grad():
        probability = torch.sigmoid(scene.model.field(samples)[FieldHeadNames.SEMANTICS].reshape(V))
    middle = float(probability.median())
    result = export_fruit_meshes(scene.pipeline, tmp_path / "fruit", semantic_threshold=middle, min_component_faces=1,
                                 **_EXPORT)
    assert torch.equal(result.vertex_probability, probability) and torch.equal(result.tsdf.values, tsdf.values)
    assert torch.equal(result.full.faces, full.faces)
    expected = full.select_by_vertex_mask(probability >= middle)
    kept = expected.n_faces
    print(f"[fruit] threshold {middle:.4f}: {kept} of {F} faces kept, {len(result)} components")
    assert 0 < kept < F
    for name in ("vertices", "faces", "normals", "colors"):
        assert torch.equal(getattr(result.mesh, name), getattr(expected, name)), name
    # ... which is the reference's selection of the full mesh
    vertices, faces = full.vertices.cpu().numpy(), full.faces.cpu().numpy()
    keep = mr.vertex_mask_faces(faces, (probability >= middle).cpu().numpy())
    new_faces, _, _ = _compare_selection("fruit", full, result.mesh, vertices, faces, keep)
    # components, statistics and the JSON agree with the reference on that mesh
    fruit_vertices = result.mesh.vertices.cpu().numpy()
    labels, ref, got = _compare("fruit components", result.mesh, fruit_vertices, new_faces)
    assert np.array_equal(result.face_component.cpu().numpy(), labels) and len(result) == ref["n_faces"].shape[0]
    records = json.loads((tmp_path / "fruit" / "fruits.json").read_text())
    assert len(records) == len(result)
    for c, record in enumerate(records):
        assert sorted(record) == ["area", "centroid", "closed", "faces", "hi", "lo", "volume"]
        assert record["faces"] == int(ref["n_faces"][c]) and record["closed"] == bool(got["closed"][c])
        assert record["area"] == got["area"][c] and record["volume"] == got["volume"][c]
        assert np.array_equal(np.array(record["centroid"]), got["centroid"][c], equal_nan=True)
        assert np.array_equal(np.float32(record["lo"]), ref["lo"][c]) and np.array_equal(np.float32(record["hi"]), ref["hi"][c])
    file_vertices, file_faces, _, _ = ply.read_triangle_mesh(str(tmp_path / "fruit" / "fruit_mesh.ply"))
    assert np.array_equal(file_vertices, fruit_vertices) and np.array_equal(file_faces, new_faces)
    # min_component_faces drops the small components of the kept faces
    sizes = ref["n_faces"]
    threshold = int(sizes.max())
    fewer = export_fruit_meshes(scene.pipeline, tmp_path / "fewer", semantic_threshold=middle,
                                min_component_faces=threshold, **_EXPORT)
    assert len(fewer) == int((sizes >= threshold).sum()) and fewer.mesh.n_faces == int(sizes[sizes >= threshold].sum())
    assert scene.model.training is False
